"""The read filter by flags and mapping quality (--min-mapq Q --exclude-flags F --require-flags F) and the read census on the CPU:
the rule in its three statements, tools/subsample_bam.py as the oracle, the host encoders and the Python reader on X with the flags
against themselves on X' = the filtered file without, the host census against numpy counts, every refusal of the tools, the new
symbols, and the stand-alone sanitizer program.  UNPINNED against samtools itself (none offline): the rule is the one line
``(flag & F) == 0 and (flag & f) == f and mapq >= q`` of its manual."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import bamio, loader, read_filter
from tests import pileup_cases as PC
from tests import read_filter_cases as RC
from tests import subsample_cases as SC

ROOT = RC.ROOT
pytestmark = pytest.mark.skipif(not loader.available(), reason="libdl4vc_loader.so not built")
NEW = {"pe": ("pe_set_read_filter", "pe_set_read_stats", "pe_get_read_stats", "pe_read_filter_passes"),
       "pg": ("pg_set_read_filter", "pg_set_read_stats", "pg_get_read_stats"),
       "cg": ("cg_set_read_filter", "cg_set_read_stats", "cg_get_read_stats")}


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return RC.write_fixture(tmp_path_factory.mktemp("read_filter_host"))


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_the_three_statements_of_the_rule_agree_on_the_grid():
    flags = [0, 0xffff] + [1 << k for k in range(12)]
    for ex, rq in ((0, 0), (0x704, 0), (0x900, 0x1), (0, 0x3), (0xf00, 0x63), (0xfffe, 0x1)):
        for q in (0, 1, 20, 60, 254, 255):
            flt = (ex, rq, q)
            rule = bamio.ReadFilter(*flt)
            for mapq in sorted({0, 1, max(q - 1, 0), q, min(q + 1, 255), 254, 255}):
                for flag in flags:
                    want = RC.predicate(flag, mapq, flt)
                    assert rule.passes(flag, mapq) == want, (flt, flag, mapq)
                    assert loader.read_filter_passes(flag, mapq, *flt) == want, (flt, flag, mapq)
    assert loader.read_filter_passes(0, 20, 0, 0, 20) and not loader.read_filter_passes(0, 19, 0, 0, 20)      # MAPQ == Q is kept


def test_off_keeps_everything():
    assert bamio.ReadFilter.of(None) is None and bamio.ReadFilter.of((0, 0, 0)) is None
    for flag in (0, 0x704, 0xffff):
        for mapq in (0, 255):
            assert loader.read_filter_passes(flag, mapq) and bamio.ReadFilter().passes(flag, mapq)


@pytest.mark.parametrize("bad,text", [((0x10000, 0, 0), "excluded flags"), ((-1, 0, 0), "excluded flags"), ((0, 0x10000, 0), "required flags"),
                                      ((0, 0, 256), "mapping quality"), ((0, 0, -1), "mapping quality"), ((0x5, 0x4, 0), "both excluded and required")])
def test_the_python_rule_and_the_native_setter_refuse_with_the_reason(tmp_path, bad, text):
    with pytest.raises(ValueError, match=text):
        bamio.ReadFilter(*bad)
    with pytest.raises(ValueError):
        loader.read_filter_passes(0, 0, *bad)
    bam, fa = PC.write_case(tmp_path, PC.get_case("qualities"))
    lib = loader.load_library()
    with loader.NativePileupEncoder(bam, fa, 16, 50, 10, 50) as enc:
        assert lib.pe_set_read_filter(enc._h, *bad) != 0 and lib.pe_last_error(enc._h).decode().startswith("pe_set_read_filter: ")
        assert lib.pe_set_read_filter(enc._h, 0x704, 0, 20) == 0 and lib.pe_set_read_filter(enc._h, 0, 0, 0) == 0   # (off again)


# ---- the fixture and tools/subsample_bam.py ---------------------------------------------------------------------------------------
def test_the_fixture_holds_what_the_issue_asks_for(fx):
    recs = RC.parsed(fx["bam"])
    assert {r.flag for r in recs} >= set(RC.FLAGS) and {r.mapq for r in recs} == set(RC.MAPQS)
    layout = SC.block_layout(fx["bam"])
    assert layout[0] >= 20 and layout[1] >= 10, layout
    # a record straddling a block boundary that each filter drops
    dropped = {flt: 0 for flt in RC.FILTERS}
    with bamio.BamFile(fx["bam"], index="") as b:
        b.r.seek(b.first_record)
        while True:
            at = b.r.tell()
            nx = b._next()
            if nx is None:
                break
            end = b.r.tell()
            if (at >> 16) != (end >> 16) and (end & 0xffff) > 0:
                for flt in RC.FILTERS:
                    dropped[flt] += not RC.predicate(nx[1].flag, nx[1].mapq, flt)
    assert all(v >= 1 for v in dropped.values()), dropped
    for flt in RC.FILTERS:
        island = [r for r in recs if r.name.startswith("island")]
        assert len(island) == 8 and any(RC.predicate(r.flag, r.mapq, flt) for r in island) == (flt not in RC.ISLAND_DROPPED)
        for tid in (0, 1):                                    # the first and the last record of a run of ~25x reads
            run = [r for r in recs if r.tid == tid and r.name.startswith("r")]
            assert not RC.predicate(run[0].flag, run[0].mapq, flt) and not RC.predicate(run[-1].flag, run[-1].mapq, flt)
    deep = [r for r in recs if r.name.startswith("deep")]
    assert len(deep) == 1060 and sum(bool(r.flag & 0x400) for r in deep) > 10 and sum(bool(r.flag & 0x800) for r in deep) == 22


@pytest.mark.parametrize("flt", RC.FILTERS)
def test_subsample_bam_with_the_filter_writes_the_records_a_python_filter_keeps(fx, flt):
    before = SC.raw_records(fx["bam"])
    keep = [r for r in before if RC.predicate(r[14] | r[15] << 8, r[9], flt)]
    assert 0 < len(keep) < len(before)
    assert SC.raw_records(RC.filtered(fx["bam"], flt)) == keep
    rule = bamio.SampleRule(*RC.SUBSAMPLE)
    both = SC.raw_records(RC.filtered(fx["bam"], flt, RC.SUBSAMPLE))
    assert both == [r for r in keep if rule.keeps_record(r)] and 0 < len(both) < len(keep)
    with bamio.BamFile(RC.filtered(fx["bam"], flt)) as b:
        assert b.index is not None
    r = SC.run_tool("subsample_bam.py", fx["bam"], fx["bam"] + ".tmp.bam", "--read-stats", *RC.flags_of(flt))
    want = RC.census_numpy([RC.parsed(fx["bam"])], flt)
    line = "read filter: %d records seen, %d dropped by flags, %d dropped by MAPQ, %d kept" % tuple(want[k] for k in read_filter.TOTALS)
    assert r.returncode == 0 and line in r.stdout and "read census:" in r.stdout and "DUP" in r.stdout and "  MAPQ 255 " in r.stdout, r.stdout
    assert want["seen"] == want["dropped_flags"] + want["dropped_mapq"] + want["kept"]


def test_subsample_bam_without_the_new_flags_writes_the_file_it_wrote_before(fx):
    """Its output under --subsample alone is the file of the tool as it was: the kept records as they lie, under the input's header,
    at compression level 6 -- rebuilt here record by record and compared by its SHA-256."""
    out = SC.subsampled(fx["bam"], *RC.SUBSAMPLE)
    rule = bamio.SampleRule(*RC.SUBSAMPLE)
    mine = fx["bam"] + ".rebuilt.bam"
    with bamio.BamFile(fx["bam"], index="") as b, \
            bamio.BamWriter(mine, list(zip(b.references, b.lengths)), header_text=b.header_text, level=6) as w:
        for body in b.raw_records():
            if rule.keeps_record(body):
                w.write_raw(body)
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()   # noqa: E731
    assert sha(out) == sha(mine)
    r = SC.run_tool("subsample_bam.py", fx["bam"], fx["bam"] + ".tmp2.bam", "--subsample", RC.SUBSAMPLE[0], "--subsample-seed", RC.SUBSAMPLE[1])
    assert r.returncode == 0 and "read" not in r.stdout and r.stdout.startswith("subsample: "), r.stdout


# ---- the host encoders and the Python reader ------------------------------------------------------------------------------------
def native(bam, fa, case, flt=None, subsample=None, read_stats=False, locs=None):
    locs = case.locs if locs is None else locs
    with loader.NativePileupEncoder.from_options(bam, fa, RC.options(case, flt, subsample, read_stats)) as enc:
        return enc.encode([l.contig for l in locs], [l.pos for l in locs], 2), enc.read_stats()


@pytest.mark.parametrize("subsample", [None, RC.SUBSAMPLE])
@pytest.mark.parametrize("flt", RC.FILTERS)
def test_the_host_encoders_on_x_with_the_flags_are_themselves_on_the_filtered_file(fx, flt, subsample):
    bam, fa, case = fx["bam"], fx["fasta"], fx["case"]
    prime = RC.filtered(bam, flt, subsample)
    plain, off_stats = native(bam, fa, case)
    got, stats = native(bam, fa, case, flt, subsample)
    want, _ = native(prime, fa, case)
    SC.same_planes(got, want, (flt, subsample))
    # not vacuous -- except for -F 0x704 alone, the mask the pileup encoders drop by themselves: there the planes must not move
    assert any(not np.array_equal(a, b) for a, b in zip(got, plain)) == (flt != (0x704, 0, 0) or subsample is not None)
    island = [i for i, l in enumerate(case.locs) if l.pos == RC.ISLAND][0]
    assert plain[5][island] == 1 and got[5][island] == want[5][island]
    assert (got[5][island] == 0) == (flt in RC.ISLAND_DROPPED)                # a location all of whose reads are dropped
    assert not any(off_stats.values())                                        # the census off leaves the stats zero
    # the census of the call: every record of a location's window, once per location
    assert read_filter.census_of(stats) == RC.census_numpy(RC.window_records(bam, case), flt, subsample)
    # the Python builder, location by location, and the Python reader
    for l in case.locs[:3] + case.locs[-2:-1]:
        loc = SC.location(l)
        assert SC.python_result(bam, fa, loc, RC.options(case, flt, subsample)) == SC.python_result(prime, fa, loc, RC.options(case)), (flt, l.pos)
    with bamio.BamFile(bam, read_filter=flt, subsample=subsample) as a, bamio.BamFile(prime) as b:
        for tid, start, stop in ((0, 0, 4000), (0, 990, 1010), (1, 2000, 3000), (1, RC.ISLAND - 5, RC.ISLAND + 5)):
            assert [(r.pos, r.name) for r in a.fetch(tid, start, stop)] == [(r.pos, r.name) for r in b.fetch(tid, start, stop)]
        wa, wb = bamio.WindowReader(a), bamio.WindowReader(b)
        for start in (100, 180, 1500, 3700):
            assert [r.name for r in wa.reads(0, start, start + 40)] == [r.name for r in wb.reads(0, start, start + 40)]


def test_the_host_census_without_a_filter_and_setting_the_filter_off(fx):
    bam, fa, case = fx["bam"], fx["fasta"], fx["case"]
    plain, _ = native(bam, fa, case)
    got, stats = native(bam, fa, case, read_stats=True)
    SC.same_planes(got, plain, "the census changes no plane")
    want = RC.census_numpy(RC.window_records(bam, case))
    assert read_filter.census_of(stats) == want and want["seen"] == want["kept"] > 1000
    # a record in two windows counts twice: two locations 10 bases apart see most records twice
    near = [PC.Loc("ctgA", 500, 1), PC.Loc("ctgA", 510, 1)]
    _, twice = native(bam, fa, case, read_stats=True, locs=near)
    once = RC.census_numpy(RC.window_records(bam, case, near))
    assert read_filter.census_of(twice) == once and once["seen"] > len({r.name for w in RC.window_records(bam, case, near) for r in w})
    off, _ = native(bam, fa, case, (0, 0, 0))
    SC.same_planes(off, plain, "a filter of zeros is no filter")


def test_a_corrupt_record_is_an_error_whether_or_not_the_filter_would_drop_it(tmp_path):
    bam, fa, loc = RC.corrupt_bam(tmp_path)
    for flt in (None, (0x400, 0, 0), (0, 0, 20)):
        with loader.NativePileupEncoder(bam, fa, 16, 50, 10, 50, read_filter=flt) as enc:
            with pytest.raises(RuntimeError, match="l_seq"):
                enc.encode([loc.contig], [loc.pos], 1)


# ---- the refusals, through the tools as processes --------------------------------------------------------------------------------
def main_py(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + list(argv), capture_output=True, text=True, timeout=300)


REFUSALS = [
    (["--min-mapq", "256"], "lies in [0, 255]"),
    (["--min-mapq", "-1"], "lies in [0, 255]"),
    (["--exclude-flags", "65536"], "must lie in [0, 0xFFFF]"),
    (["--require-flags", "0x10000"], "must lie in [0, 0xFFFF]"),
    (["--exclude-flags", "-4"], "must lie in [0, 0xFFFF]"),
    (["--exclude-flags", "dup"], "is not a number"),
    (["--exclude-flags", "0x704", "--require-flags", "0x404"], "no read could pass"),
]


@pytest.mark.parametrize("flags,text", REFUSALS)
def test_every_tool_refuses_with_the_reason(tmp_path, flags, text):
    bam = str(tmp_path / "x.bam")
    tools = [("candidate_generator.py", ["--input", bam, "--output", str(tmp_path / "o.vcf")]),
             ("convert_bam_single_reads.py", ["--input", bam, "--output", str(tmp_path / "o.hdf"), "--save-q-scores", "--save-strand"]),
             ("subsample_bam.py", [bam, str(tmp_path / "o.bam")]),
             ("candgen_rate.py", ["--bam", bam]), ("pileup_inflate_rate.py", ["--dir", str(tmp_path)]),
             ("score_bam_rate.py", ["--dir", str(tmp_path / "sbr")])]
    for tool, argv in tools:
        r = SC.run_tool(tool, *(argv + flags))
        assert r.returncode != 0 and text in r.stderr, (tool, flags, r.stderr[-600:])
    r = main_py("--test_bam", bam, "--test_fasta", "x.fa", "--sample_vcf", "x.vcf", "--modelload", "m", *flags)
    assert r.returncode != 0 and text in r.stderr, (flags, r.stderr[-600:])
    assert not any(os.path.exists(str(tmp_path / f)) for f in ("o.vcf", "o.bam", "o.hdf", "sbr"))


def test_the_converter_prints_the_counts_of_its_native_encoder(fx, tmp_path):
    import dataclasses
    bam, fa = fx["bam"], fx["fasta"]
    # the candidate file's reader knows windows of 201 columns: the converter's default window, away from the contigs' ends
    case = dataclasses.replace(fx["case"], w=100, max_reads=20, locs=[l for l in fx["case"].locs if l.pos < 3000 - 200])
    flt = RC.FILTERS[0]
    vcf = str(tmp_path / "locs.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        f.write("".join("%s\t%d\t.\tA\tC\t50\t.\t.\n" % (l.contig, l.pos) for l in case.locs))
    common = ["--fp_vcf", vcf, "--fasta-input", fa, "--max-reads", case.max_reads, "--window-size", case.w, "--num-processes", 2,
              "--save-q-scores", "--save-strand"]
    a = SC.run_tool("convert_bam_single_reads.py", "--input", bam, "--output", tmp_path / "a.hdf", "--read-stats", *(common + RC.flags_of(flt)))
    b = SC.run_tool("convert_bam_single_reads.py", "--input", RC.filtered(bam, flt), "--output", tmp_path / "b.hdf", *common)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-1500:], b.stderr[-1500:])
    want = RC.census_numpy(RC.window_records(bam, case), flt)
    line = "read filter: %d records seen, %d dropped by flags, %d dropped by MAPQ, %d kept" % tuple(want[k] for k in read_filter.TOTALS)
    assert line in a.stdout and "read census:" in a.stdout, a.stdout[-1500:]
    assert "read filter" not in b.stdout and "read census" not in b.stdout
    from dl4vc_amd import hdf5io
    with hdf5io.CandidateFile(str(tmp_path / "a.hdf")) as ha, hdf5io.CandidateFile(str(tmp_path / "b.hdf")) as hb:
        assert len(ha) == len(hb) > 3 and ha.read(0, len(ha)).tobytes() == hb.read(0, len(hb)).tobytes()


def test_main_py_refuses_the_flags_where_no_bam_is_read():
    for argv in (["--test_file", "x.hdf", "--modelload", "m"], ["--train_file", "t.hdf", "--test_file", "x.hdf"]):
        for flags in (["--min-mapq", "20"], ["--exclude-flags", "0x704"], ["--require-flags", "1"], ["--read-stats"]):
            r = main_py(*argv, *flags)
            assert r.returncode != 0 and "this run reads none" in r.stderr, r.stderr[-600:]
    assert "read filter" not in main_py("--test_file", "x.hdf").stdout       # (the flags leave no trace when absent)


def test_the_shell_scripts_take_the_letters_and_refuse_them_without_a_bam(tmp_path):
    cv = os.path.join(ROOT, "call_variants.sh")
    for letter, value in (("-q", "20"), ("-F", "0x704"), ("-R", "1")):
        r = subprocess.run(["bash", cv, "-m", "m", "-o", str(tmp_path), letter, value], capture_output=True, text=True)
        assert r.returncode == 1 and "give -i BAM as well" in r.stdout, r.stdout
    for script in (cv, os.path.join(ROOT, "tools", "make_training_data.sh")):
        text = open(script).read()
        assert "q:F:R:" in text and '--min-mapq "$MINMAPQ"' in text and '--exclude-flags "$EXCLUDE"' in text and '--require-flags "$REQUIRE"' in text
        assert text.count('"${SUBFLAGS[@]}"') >= 2              # candidate generation and the pileup stage get the same flags


# ---- headers = exports = bindings --------------------------------------------------------------------------------------------
def test_headers_exports_and_bindings_agree_on_the_new_symbols():
    from dl4vc_amd import candgen, pileup_gpu
    inc = os.path.join(ROOT, "include")
    for prefix, header, mod, lib_path in (("pe", "dl4vc_loader.h", loader, loader.LIB_PATH), ("pg", "dl4vc_pileup_gpu.h", pileup_gpu, pileup_gpu.LIB_PATH),
                                          ("cg", "dl4vc_candgen.h", candgen, candgen.LIB_PATH)):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, header)).read(), flags=re.S)
        declared = set(re.findall(r"\b(%s_[a-z_]+)\s*\(" % prefix, text))
        assert set(NEW[prefix]) <= declared and set(NEW[prefix]) <= set(mod.SYMBOLS)
        if not os.path.isfile(lib_path):
            continue
        out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if l.split()}
        assert set(NEW[prefix]) <= exported, (prefix, set(NEW[prefix]) - exported)
    # the one shared struct: 256 + 16 + 4 words of 64 bits, the header's order
    import ctypes as C
    assert C.sizeof(read_filter.ReadStats) == 8 * 276
    body = re.search(r"typedef struct dl4vc_read_stats \{(.*?)\} dl4vc_read_stats;", open(os.path.join(inc, "dl4vc_loader.h")).read(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"uint64_t\s+([a-z_]+)(?:\[\d+\])?\s*;", body) == [f[0] for f in read_filter.ReadStats._fields_]


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------
def test_the_rule_and_the_host_census_run_clean_under_the_sanitizers(tmp_path):
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_read_filter.sh"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "asan_read_filter: OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
