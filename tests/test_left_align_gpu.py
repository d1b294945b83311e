"""Left-alignment of candidate indels against the FASTA on the MI355X (``left_align=True``).

The oracle is the method of --subsample: BAM X with the option == its twin X' without it (tests/left_align_cases.py: the same
SEQs with every eligible indel placed where the Python restatement of the rule puts it), VCF body byte for byte and tuples equal
as doubles.  The fixture holds no other allele inside a shifted window, so DP is equal as well (the case builder asserts it)."""
import os

import pytest

from dl4vc_amd import candidates as C
from dl4vc_amd.candgen import CandidateCounter
from tests import candidates_reference_cases as K
from tests import left_align_cases as L

pytestmark = pytest.mark.gpu
FLAGS = dict(threads=4, snp_min_freq=0.075, indel_min_freq=0.02, keep_multialleles=True)
COUNTERS = ("observations", "shifted", "bases_shifted", "clamped", "not_eligible")


def _body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("#")]


def _generate(bam, out, **kw):
    stats = C.generate(bam, str(out), **{**FLAGS, **kw})
    return _body(str(out)), stats


def _counters(stats):
    return {k: stats["left_align_" + k] for k in COUNTERS}


def _subs(chunk_size):
    return C.split_subregions([(n, 0, l) for n, l, _ in K.CONTIGS], chunk_size * 1000)


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    d = tmp_path_factory.mktemp("leftalign")
    case, bare = L.build(), L.build(md=False)
    (d / "fai").mkdir()
    (d / "scan").mkdir()
    x, twin = L.write_case(case, d)
    bx, btwin = L.write_case(bare, d, md=False)
    open(str(d / "in.bed"), "w").write(L.BED)
    return dict(dir=d, case=case, bare=bare, x=x, twin=twin, bare_x=bx, bare_twin=btwin, bed=str(d / "in.bed"),
                fasta={True: K.write_fasta(case["genome"], str(d / "fai" / "ref.fa"), True),
                       False: K.write_fasta(case["genome"], str(d / "scan" / "ref.fa"), False)})


# ---- 1. X with the option == X' without it ------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [1, 1000])
@pytest.mark.parametrize("fai", [True, False])
def test_option_on_x_equals_twin_without_it(fx, chunk_size, fai):
    d = fx["dir"]
    want, st_t = _generate(fx["twin"], d / "twin.vcf", chunk_size=chunk_size, reference=fx["fasta"][fai])
    got, st_x = _generate(fx["x"], d / "x.vcf", chunk_size=chunk_size, reference=fx["fasta"][fai], left_align=True)
    assert got == want and len(want) > 20
    assert _counters(st_x) == L.expected_counters(fx["case"], _subs(chunk_size))
    assert st_x["left_align_shifted"] == 18 and st_x["left_align_clamped"] == 1 and st_x["left_align_not_eligible"] == 3
    assert "left_align_observations" not in st_t
    for k in ("reads", "reads_malformed", "reads_deletions_dropped", "allele_events"):
        assert st_x[k] == st_t[k], k
    # by hand (POS is 1-based): one record with count 3 of 5 for the three placements, the rotated insertion counted twice, the
    # shift of 10 with L = 4, the read that starts inside its repeat, position 0, the stops behind N and R, REF of 60 shifted
    ref = fx["case"]["refs"]["ctgA"]
    for line in ("ctgA\t200\t.\tGT\tG\t50\t.\tDP=5;AF=0.6\tGT:GQ\t1:50", "ctgA\t400\t.\tGAC\tG\t50\t.\tDP=4;AF=0.5\tGT:GQ\t1:50",
                 "ctgA\t400\t.\tGACAC\tG\t50\t.\tDP=4;AF=0.25\tGT:GQ\t1:50", "ctgA\t600\t.\tG\tGAC\t50\t.\tDP=4;AF=0.5\tGT:GQ\t1:50",
                 "ctgA\t600\t.\tG\tGACAC\t50\t.\tDP=4;AF=0.25\tGT:GQ\t1:50", "ctgA\t804\t.\tAA\tA\t50\t.\tDP=3;AF=0.333333\tGT:GQ\t1:50",
                 "ctgA\t800\t.\tGA\tG\t50\t.\tDP=2;AF=0.5\tGT:GQ\t1:50", "ctgA\t1\t.\tGA\tG\t50\t.\tDP=2;AF=0.5\tGT:GQ\t1:50",
                 "ctgA\t996\t.\tGT\tG\t50\t.\tDP=3;AF=0.666667\tGT:GQ\t1:50", "ctgA\t2307\t.\tAA\tA\t50\t.\tDP=2;AF=0.5\tGT:GQ\t1:50",
                 "ctgA\t2407\t.\tTT\tT\t50\t.\tDP=2;AF=0.5\tGT:GQ\t1:50", "ctgA\t2603\t.\tAC\tA\t50\t.\tDP=2;AF=0.5\tGT:GQ\t1:50",
                 "ctgA\t3100\t.\t%s\tA\t50\t.\tDP=2;AF=1\tGT:GQ\t1:50" % ref[3099:3159],
                 "ctgB\t1500\t.\tGA\tG\t50\t.\tDP=60;AF=0.0333333\tGT:GQ\t1:50"):
        assert line in got, line
    assert sum(l.startswith("ctgA\t996\t") for l in got) == 1                     # once, in the subregion left of 1000
    assert not [l for l in got if len(l.split("\t")[3]) > 60] and [l for l in got if len(l.split("\t")[3]) == 60]


def test_tuples_equal_as_doubles_and_reads_without_md(fx):
    subs = _subs(1)
    regs = [(L.NAMES.index(c), s, e) for c, s, e in subs]
    kw = dict(threads=4, snp_min_freq=0.075, indel_min_freq=0.02, reference=fx["fasta"][True])
    for x, twin, case in ((fx["x"], fx["twin"], fx["case"]), (fx["bare_x"], fx["bare_twin"], fx["bare"])):
        with CandidateCounter(twin, **kw) as cc:
            want, _ = cc.run(regs)
        with CandidateCounter(x, left_align=True, **kw) as cc:
            got, st = cc.run(regs)
            again, st2 = cc.run(regs)                                             # the counters are of the last run
        assert sorted(got) == sorted(want) == sorted(again) and len(want) > 20
        assert sorted(C.candidate_tuples(subs, got, True)) == sorted(C.candidate_tuples(subs, want, True))
        assert _counters(st) == _counters(st2) == L.expected_counters(case, subs)
    assert st["reference_reads"] == st["reads"] and st["left_align_not_eligible"] == 2       # (no MD: the FASTA is the only source)


# ---- 2. records framed on the device; shards --------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [1, 1000])
def test_device_framed_records_give_the_same_bytes_and_counters(fx, chunk_size):
    d = fx["dir"]
    kw = dict(chunk_size=chunk_size, reference=fx["fasta"][True], left_align=True)
    host, st_h = _generate(fx["x"], d / "h.vcf", **kw)
    dev, st_d = _generate(fx["x"], d / "d.vcf", inflate_device="gpu", **kw)
    assert open(str(d / "h.vcf"), "rb").read() == open(str(d / "d.vcf"), "rb").read() and len(host) > 20
    assert st_d["inflate_records"] > 0 and _counters(st_d) == _counters(st_h) == L.expected_counters(fx["case"], _subs(chunk_size))


def test_two_shards_merged_give_the_one_process_file(fx):
    d = fx["dir"]
    kw = dict(chunk_size=1, reference=fx["fasta"][True], left_align=True)
    _, st = _generate(fx["x"], d / "one.vcf", **kw)
    for g in range(2):
        C.generate(fx["x"], str(d / "two.vcf"), shard=(g, 2), **{**FLAGS, **kw})
    total = C.merge_parts(str(d / "two.vcf"), 2)
    assert open(str(d / "one.vcf"), "rb").read() == open(str(d / "two.vcf"), "rb").read()
    assert _counters(total) == _counters(st)


# ---- 3. the option off ----------------------------------------------------------------------------------------------------------
def test_reference_without_the_option_is_todays_arm(fx):
    d = fx["dir"]
    md_arm, _ = _generate(fx["x"], d / "md.vcf", chunk_size=1)
    ref_arm, st = _generate(fx["x"], d / "ref.vcf", chunk_size=1, reference=fx["fasta"][True])
    assert ref_arm == md_arm and "left_align_observations" not in st
    # the placements stay apart: the three deletions of the homopolymer are three records
    for pos in (200, 202, 204):
        assert [l for l in md_arm if l.startswith("ctgA\t%d\t.\t%sT\t" % (pos, "G" if pos == 200 else "T"))], pos
    on, _ = _generate(fx["x"], d / "on.vcf", chunk_size=1, reference=fx["fasta"][True], left_align=True)
    assert on != ref_arm


def test_threshold_case_exists_only_with_the_option(fx):
    d = fx["dir"]
    at = "ctgB\t%d\t" % (L.THRESHOLD_POS + 1)
    off, _ = _generate(fx["x"], d / "off.vcf", chunk_size=1000, reference=fx["fasta"][True])
    on, _ = _generate(fx["x"], d / "on.vcf", chunk_size=1000, reference=fx["fasta"][True], left_align=True)
    assert not [l for l in off if l.startswith("ctgB\t")]                          # 1 / 60 < 0.02 at either placement
    assert [l for l in on if l.startswith("ctgB\t")] == [at + ".\tGA\tG\t50\t.\tDP=60;AF=0.0333333\tGT:GQ\t1:50"]


def test_bed_interval_takes_the_shifted_position(fx):
    d = fx["dir"]
    kw = dict(chunk_size=1000, bedfile=fx["bed"], reference=fx["fasta"][True])
    want, _ = _generate(fx["twin"], d / "bt.vcf", **kw)
    on, st = _generate(fx["x"], d / "bx.vcf", left_align=True, **kw)
    off, _ = _generate(fx["x"], d / "bo.vcf", **kw)
    assert on == want
    indels = lambda lines: sorted(int(l.split("\t")[1]) for l in lines if len(l.split("\t")[3]) != len(l.split("\t")[4]))
    assert indels(on) == [2097] and indels(off) == [2004]          # 2103 shifts in to 2096, 2003 shifts out to 1995 (0-based)
    assert _counters(st) == L.expected_counters(fx["case"], [("ctgA", 2000, 2100)])


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_left_align_without_a_reference_is_refused_and_the_handle_stays_usable(fx):
    regs = [(0, 0, 1000)]
    with CandidateCounter(fx["x"], threads=2) as cc:
        assert cc.lib.cg_set_left_align(cc.h, 1) != 0
        assert "no reference is set" in cc.lib.cg_last_error().decode()
        before, _ = cc.run(regs)
        assert cc.lib.cg_set_reference(cc.h, os.fsencode(fx["fasta"][True])) == 0 and cc.lib.cg_set_left_align(cc.h, 1) == 0
        assert cc.lib.cg_set_reference(cc.h, None) != 0 and "switch it off first" in cc.lib.cg_last_error().decode()
        on, _ = cc.run(regs)
        assert cc.lib.cg_set_left_align(cc.h, 0) == 0 and cc.lib.cg_set_reference(cc.h, None) == 0
        after, _ = cc.run(regs)
    assert sorted(before) == sorted(after) != sorted(on) and len(before) > 5
    assert [t for t in on if t[2] == 199 and t[6] == 3] and not [t for t in before if t[6] == 3]
    with pytest.raises(ValueError, match="left_align needs reference"):
        CandidateCounter(fx["x"], left_align=True)
