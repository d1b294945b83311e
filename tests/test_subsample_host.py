"""Read subsampling by name hash (--subsample F --subsample-seed S) on the CPU: the rule against its worked values and the native
definition, tools/subsample_bam.py, the host encoders on X with the option against themselves on X' = subsample_bam(X) without,
every refusal of the tools, and the stand-alone sanitizer program.  UNPINNED against samtools itself: the table is the issue's
restatement of htslib's X31 / Wang hash, not samtools' output.

The kept share is asserted to lie in [0.35, 0.65] at F = 0.5 for every fixture of 200 reads or more (three standard deviations of
a fair coin over 200 draws are 0.106, so a correct rule stays inside with room; a fixture of 6 or 30 reads cannot be held to a band)
and for the grid pooled."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import bamio, loader
from dl4vc_amd import pileup_encoder as PE
from tests import pileup_cases as PC
from tests import subsample_cases as SC
from tests import train_bam_cases as TC

ROOT = SC.ROOT
pytestmark = pytest.mark.skipif(not loader.available(), reason="libdl4vc_loader.so not built")
F = SC.FRACTION


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_the_worked_values_of_the_rule():
    for name, seed, x31, mixed, low in SC.WORKED:
        assert bamio.name_hash(name) == x31, name
        assert bamio.wang(x31 ^ seed) == mixed, (name, seed)
        assert bamio.wang(bamio.name_hash(name) ^ seed) & 0xffffff == low
        for f, thr in SC.THRESHOLDS:                          # the native rule gives the same answer at every threshold
            assert loader.subsample_keeps(name + b"\x00", f, seed) == (low < thr), (name, seed, f)
    for f, thr in SC.THRESHOLDS:
        assert bamio.SampleRule(f).threshold == thr, f
    assert bamio.name_hash(b"") == 0 and bamio.name_hash(b"\x00abc") == 0
    assert bamio.name_hash(b"ab\x00cd") == bamio.name_hash(b"ab")
    assert bamio.name_hash(b"\xff") == 0xffffffff              # a byte >= 0x80 is widened as a signed char
    assert bamio.name_hash(b"a\x80") == (97 * 31 - 128) & 0xffffffff


def test_the_python_rule_is_the_native_rule_on_random_names():
    rng = np.random.default_rng(5)
    names = [bytes(rng.integers(1, 256, int(rng.integers(1, 255)), dtype=np.uint8)) for _ in range(5000)]
    names[:4] = [b"a", b"\x80", b"Z" * 254, bytes([200]) * 254]
    kept = {}
    for seed in (0, 1, (1 << 32) - 1):
        for f in (1e-9, 0.3, 0.5, 1.0):
            rule = bamio.SampleRule(f, seed)
            want = [rule.keeps(n) for n in names]
            got = [loader.subsample_keeps(n + b"\x00", f, seed) for n in names]
            assert got == want, (seed, f, [n for n, a, b in zip(names, want, got) if a != b][:3])
            kept[(seed, f)] = sum(want)
        assert kept[(seed, 1.0)] == len(names)                 # F = 1.0 keeps all
        assert 0.45 < kept[(seed, 0.5)] / len(names) < 0.55 and 0.26 < kept[(seed, 0.3)] / len(names) < 0.34
    # a name field without a NUL inside l_read_name: at most l_read_name - 1 bytes are read
    assert loader.subsample_keeps(b"abcd", 0.5, 3) == bamio.SampleRule(0.5, 3).keeps(b"abc")


def test_mates_get_one_answer_and_the_seed_matters():
    case = SC.named_case()
    for seed in SC.SEEDS:
        rule = bamio.SampleRule(F, seed)
        by_name = {}
        for r in case.reads:
            body = bamio.pack_record(r.tid, r.pos, r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist())[4:]
            by_name.setdefault(r.name, set()).add(rule.keeps_record(body))
        assert all(len(v) == 1 for v in by_name.values())
        # names of 1 and of 254 characters are among the kept and among the dropped
        for group in (SC.ONE_CHAR, SC.LONG):
            answers = {next(iter(by_name[n])) for n in group}
            assert answers == {True, False}, (seed, group[0][:3])
    a, b = bamio.SampleRule(F, 0), bamio.SampleRule(F, 7)
    assert any(a.keeps(r.name.encode()) != b.keeps(r.name.encode()) for r in case.reads)


@pytest.mark.parametrize("bad", [0.0, -0.1, 1.0000001, float("nan"), float("inf")])
def test_the_python_rule_refuses_a_fraction_outside_the_interval(bad):
    with pytest.raises(ValueError, match="fraction"):
        bamio.SampleRule(bad, 0)


def test_the_seed_and_the_native_setters_refuse_with_the_reason(tmp_path):
    for seed in (-1, 1 << 32, 1.5):
        with pytest.raises(ValueError, match="seed"):
            bamio.SampleRule(0.5, seed)
    bam, fa = PC.write_case(tmp_path, PC.get_case("qualities"))
    lib = loader.load_library()
    with loader.NativePileupEncoder(bam, fa, 16, 50, 10, 50) as enc:
        for bad in (-0.5, 1.5, float("nan")):
            assert lib.pe_set_subsample(enc._h, bad, 0) != 0
            assert "fraction must lie in [0, 1]" in lib.pe_last_error(enc._h).decode()
        assert lib.pe_set_subsample(enc._h, 0.5, 7) == 0 and lib.pe_set_subsample(enc._h, 0.0, 0) == 0     # (0 turns it off again)
    with pytest.raises(ValueError):
        loader.subsample_keeps(b"", 0.5, 0)


# ---- tools/subsample_bam.py ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    return SC.write_block_bams(tmp_path_factory.mktemp("subsample_blocks"))


def test_subsample_bam_writes_the_kept_records_as_they_are(blocks):
    src = blocks["md"]
    layout = SC.block_layout(src)
    assert layout[0] >= 3 and layout[1] >= 1, layout         # the device-inflate arms need blocks and records across their ends
    before = SC.raw_records(src)
    for seed in SC.SEEDS:
        rule = bamio.SampleRule(F, seed)
        out = SC.subsampled(src, F, seed)
        after = SC.raw_records(out)
        assert after == [r for r in before if rule.keeps_record(r)]          # the kept subsequence, in order, equal bytes
        assert 0.35 <= len(after) / len(before) <= 0.65
        with bamio.BamFile(src) as a, bamio.BamFile(out) as b:
            assert (a.header_text, a.references, a.lengths) == (b.header_text, b.references, b.lengths)
            assert b.index is not None                        # OUT.bam.bai loads
            for start, stop in ((0, 30000), (5000, 5100), (16384, 16385), (28990, 30000)):
                got = [(r.pos, r.name) for r in b.fetch(0, start, stop)]
                scan = [(r.pos, r.name) for r in b if r.pos < stop and r.reference_end > start]
                assert got == scan and (len(got) > 0 or start > 29100), (start, stop)
                # ... and it is what fetch on X with the rule returns
                with bamio.BamFile(src, subsample=(F, seed)) as c:
                    assert [(r.pos, r.name) for r in c.fetch(0, start, stop)] == got
    assert SC.raw_records(SC.subsampled(src, 1.0, 0)) == before
    assert SC.raw_records(SC.subsampled(src, F, 0)) != SC.raw_records(SC.subsampled(src, F, 7))
    r = SC.run_tool("subsample_bam.py", src, src + ".tmp.bam", "--subsample", 0.5, "--subsample-seed", 7)
    kept = len(SC.raw_records(SC.subsampled(src, F, 7)))
    assert r.returncode == 0 and "subsample: %d records seen, %d kept" % (len(before), kept) in r.stdout and "seed 7" in r.stdout, r.stdout


# ---- the host encoders ---------------------------------------------------------------------------------------------------------
def native(bam, fa, case, contigs, pos, subsample=None):
    with loader.NativePileupEncoder.from_options(bam, fa, SC.options(case, subsample)) as enc:
        return enc.encode(contigs, pos, 2)


@pytest.mark.parametrize("name", PC.CASE_NAMES + ["subsample_names"])
def test_the_host_encoders_on_x_with_the_option_are_themselves_on_x_prime(tmp_path, name):
    case = SC.named_case() if name == "subsample_names" else PC.get_case(name)
    bam, fa = PC.write_case(tmp_path, case)
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    plain = native(bam, fa, case, contigs, pos)
    SC.same_planes(native(bam, fa, case, contigs, pos, (1.0, 3)), plain, "F = 1.0 keeps all")
    differs = False
    for seed in SC.SEEDS:
        if len(case.reads) >= 200:
            assert 0.35 <= SC.kept_share(bam, F, seed) <= 0.65, (name, seed)
        sub = SC.subsampled(bam, F, seed)
        if not case.index and os.path.isfile(sub + ".bai"):   # (kept records that are not sorted get no index from the tool)
            os.remove(sub + ".bai")                           # the case runs without an index: so does its X'
        with_option = native(bam, fa, case, contigs, pos, (F, seed))
        SC.same_planes(with_option, native(sub, fa, case, contigs, pos), (name, seed))
        differs = differs or any(not np.array_equal(a, b) for a, b in zip(with_option, plain))
        for l in case.locs:                                   # the Python builder, location by location
            loc = SC.location(l)
            assert SC.python_result(bam, fa, loc, SC.options(case, (F, seed))) == SC.python_result(sub, fa, loc, SC.options(case)), \
                (name, seed, l.pos, l.note)
    if len(case.reads) >= 200:
        assert differs, "the sampled planes equal the unsampled ones: the test would pass with the rule ignored"


def test_the_grid_pooled_keeps_about_half():
    for seed in SC.SEEDS:
        rule = bamio.SampleRule(F, seed)
        reads = [r for n in PC.CASE_NAMES for r in PC.get_case(n).reads]
        assert 0.35 <= sum(rule.keeps(r.name.encode()) for r in reads) / len(reads) <= 0.65


def test_the_labelled_fixture_through_encode_locations(tmp_path):
    """``encode_locations`` (pe_encode, then the Python builder for what it declines: the ``twin`` pair) with ``subsample=`` on the
    labelled BAM of the training tests equals itself on X'; the 1 100-track site and the deep sites change."""
    fx = TC.labelled_fixture(tmp_path)
    opt = PE.EncoderOptions(window_size=100, max_reads=200, max_insert_length=10, max_insert_length_variant=50)
    locs = TC.locations(fx, "train") + TC.locations(fx, "test")
    plain, plain_errors = PE.encode_locations(fx["bam"], fx["fasta"], locs, opt, threads=2)
    for seed in SC.SEEDS:
        assert 0.35 <= SC.kept_share(fx["bam"], F, seed) <= 0.65
        sub = SC.subsampled(fx["bam"], F, seed)
        got, errors = PE.encode_locations(fx["bam"], fx["fasta"], locs, opt, threads=2, subsample=(F, seed))
        want, want_errors = PE.encode_locations(sub, fx["fasta"], locs, opt, threads=2)
        assert errors == want_errors and got.tobytes() == want.tobytes(), seed
        assert got.tobytes() != plain.tobytes()
        assert int(got["num_reads"].max()) <= int(plain["num_reads"].max())
    assert plain_errors <= errors                             # fewer reads: no location gains a record


# ---- the refusals, through the tools as processes --------------------------------------------------------------------------------
def main_py(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, "main.py")] + list(argv), capture_output=True, text=True, timeout=300)


REFUSALS = [
    (["--subsample", "0"], "fraction must lie in (0, 1]"),
    (["--subsample", "1.5"], "fraction must lie in (0, 1]"),
    (["--subsample", "-0.2"], "fraction must lie in (0, 1]"),
    (["--subsample", "nan"], "fraction must lie in (0, 1]"),
    (["--subsample", "0.5", "--subsample-seed", "-1"], "seed must lie in [0, 2^32)"),
    (["--subsample", "0.5", "--subsample-seed", "4294967296"], "seed must lie in [0, 2^32)"),
    (["--subsample-seed", "3"], "without --subsample"),
]


@pytest.mark.parametrize("flags,text", REFUSALS)
def test_every_tool_refuses_with_the_reason(tmp_path, flags, text):
    bam = str(tmp_path / "x.bam")
    tools = [("candidate_generator.py", ["--input", bam, "--output", str(tmp_path / "o.vcf")]),
             ("convert_bam_single_reads.py", ["--input", bam, "--output", str(tmp_path / "o.hdf"), "--save-q-scores", "--save-strand"]),
             ("subsample_bam.py", [bam, str(tmp_path / "o.bam")])]
    for tool, argv in tools:
        r = SC.run_tool(tool, *(argv + flags))
        assert r.returncode != 0 and text in r.stderr, (tool, flags, r.stderr[-600:])
    r = main_py("--test_bam", bam, "--test_fasta", "x.fa", "--sample_vcf", "x.vcf", "--modelload", "m", *flags)
    assert r.returncode != 0 and text in r.stderr, (flags, r.stderr[-600:])
    assert not os.path.exists(str(tmp_path / "o.vcf")) and not os.path.exists(str(tmp_path / "o.bam"))


def test_main_py_refuses_the_flag_where_no_bam_is_read():
    for argv in (["--test_file", "x.hdf", "--modelload", "m"], ["--train_file", "t.hdf", "--test_file", "x.hdf"]):
        r = main_py(*argv, "--subsample", "0.5")
        assert r.returncode != 0 and "this run reads no BAM" in r.stderr, r.stderr[-600:]
        r = main_py(*argv, "--subsample-seed", "1")
        assert r.returncode != 0 and "without --subsample" in r.stderr, r.stderr[-600:]
    assert "subsample" not in main_py("--test_file", "x.hdf").stdout        # (the flags leave no trace when absent)


def test_the_shell_scripts_refuse_a_seed_without_a_fraction_and_a_fraction_without_a_bam(tmp_path):
    cv = os.path.join(ROOT, "call_variants.sh")
    r = subprocess.run(["bash", cv, "-m", "m", "-o", str(tmp_path), "-S", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "-S is the seed of -s" in r.stdout
    r = subprocess.run(["bash", cv, "-m", "m", "-o", str(tmp_path), "-s", "0.5"], capture_output=True, text=True)
    assert r.returncode == 1 and "give -i BAM as well" in r.stdout
    mt = os.path.join(ROOT, "tools", "make_training_data.sh")
    r = subprocess.run(["bash", mt, "-i", "x.bam", "-r", "r.fa", "-t", "t.vcf", "-o", str(tmp_path), "-S", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and "-S is the seed of -s" in r.stdout


# ---- the stand-alone sanitizer program ------------------------------------------------------------------------------------------
def test_the_rule_runs_clean_under_the_sanitizers(tmp_path):
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_subsample.sh"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "asan_subsample: OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
