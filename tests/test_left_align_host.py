"""Left-alignment of indels, the parts that need no GPU: the C++ rule of dl4vc_amd/csrc/cand_left_align.h on the CPU
(``cg_left_align_host``) against its Python restatement (``truthset.left_align_letters``) over the enumerated grid and the
fixture of tests/left_align_cases.py; ``truthset.left_align_record`` and the pairing with ``--left-align``; the command lines'
refusals and the ``-L`` of the two scripts."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import truthset as T
from tests import candidates_reference_cases as K
from tests import left_align_cases as L

CODES = K.CODES


@pytest.fixture(scope="module")
def candgen():
    from dl4vc_amd import candgen
    if not os.path.isfile(candgen.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return candgen


def _codes(letters):
    return np.array([CODES.index(c) for c in letters], np.uint8)


def _host(candgen, letters, kind, a, anchor, bases, floor, aligned=True):
    pos, code, out, flags = candgen.left_align_host(_codes(letters), kind, aligned, a, CODES.index(anchor), _codes(bases), floor)
    return pos, CODES[code], "".join(CODES[c] for c in out), bool(flags & candgen.LEFT_ALIGN_ELIGIBLE), bool(flags & candgen.LEFT_ALIGN_CLAMPED)


# ---- 1. the C++ rule == the Python restatement ----------------------------------------------------------------------------------
def test_host_rule_equals_the_restatement_over_the_grid(candgen):
    lib = candgen.load_library()
    n = shifted = clamped = beyond_l = 0
    pos, flags = ctypes.c_int64(), ctypes.c_int32()
    out = np.zeros(8, np.uint8)
    last, codes = None, None
    for g, kind, a, anchor, bases, floor in L.grid():
        if g is not last:
            last, codes = g, _codes(g)
        b = _codes(bases)
        assert lib.cg_left_align_host(codes.ctypes.data, len(g), kind, 1, a, CODES.index(anchor), b.ctypes.data, len(b), floor,
                                      ctypes.byref(pos), out.ctypes.data, ctypes.byref(flags)) == 0
        got = (pos.value, CODES[out[0]], "".join(CODES[c] for c in out[1:1 + len(b)]), bool(flags.value & 1), bool(flags.value & 2))
        want = T.left_align_letters(lambda i: g[i], len(g), kind, a, anchor, bases, floor)
        assert got == want, (g, kind, a, anchor, bases, floor)
        n += 1
        shifted += want[0] != a
        clamped += want[4]
        beyond_l += a - want[0] > len(bases)
    assert n > 100000 and shifted > 5000 and clamped > 1000 and beyond_l > 500, (n, shifted, clamped, beyond_l)


def test_host_rule_equals_the_restatement_over_the_fixture(candgen):
    case = L.build()
    moved = 0
    for letters, kind, a, anchor, bases, floor, aligned in L.observations(case):
        want = T.left_align_letters(lambda i: letters[i], len(letters), kind, a, anchor, bases, floor, aligned)
        assert _host(candgen, letters, kind, a, anchor, bases, floor, aligned) == want, (kind, a, bases)
        moved += want[0] != a
    assert moved == 20            # (18 that are counted and the two deletions of 60 bases that the length limit then drops)
    # by hand: the three placements of the homopolymer deletion, the rotated insertion, the shift of 10 with L = 4
    ref = case["refs"]["ctgA"]
    for a in (199, 201, 203):
        assert _host(candgen, ref, T.LA_DEL, a, "T" if a > 199 else "G", "T", 150)[:3] == (199, "G", "T")
    assert _host(candgen, ref, T.LA_INS, 604, "A", "CA", 540)[:3] == _host(candgen, ref, T.LA_INS, 607, "C", "AC", 545)[:3] == (599, "G", "AC")
    assert _host(candgen, ref, T.LA_INS, 609, "C", "ACAC", 550)[:3] == (599, "G", "ACAC")
    assert _host(candgen, ref, T.LA_DEL, 806, "A", "A", 803) == (803, "A", "A", True, True)
    assert _host(candgen, ref, T.LA_DEL, 4, "A", "A", 0) == (0, "G", "A", True, False)
    assert _host(candgen, ref, T.LA_DEL, 2308, "A", "A", 2250)[:2] == (2306, "A")          # the N at 2305
    assert _host(candgen, ref, T.LA_DEL, 2408, "T", "T", 2350)[:2] == (2406, "T")          # the R at 2405


def test_host_rule_reads_nothing_outside_the_contig(candgen):
    g = "ACACACAC"
    for a in (-1, 8, 1 << 40):
        assert _host(candgen, g, T.LA_DEL, a, "A", "C", 0)[3] is False
    assert _host(candgen, g, T.LA_DEL, 5, "C", "AC", 0) == (0, "A", "CA", True, False)      # a + L = length - 1
    assert _host(candgen, g, T.LA_DEL, 6, "A", "CA", 0)[3] is False                          # a + L = length
    assert _host(candgen, g, T.LA_DEL, 7, "C", "A", 0)[3] is False
    assert _host(candgen, g, T.LA_INS, 7, "C", "AC", -5) == (0, "A", "CA", True, False)     # a negative floor is 0
    rep = "G" + "AC" * 60
    for bases in (("CA" * 32)[:63], "AC" * 31, ("AC" * 32)[:63]):                            # L = 63 and 62: shifts beyond L, or none
        want = T.left_align_letters(lambda i: rep[i], len(rep), T.LA_INS, 120, "C", bases, 0)
        assert _host(candgen, rep, T.LA_INS, 120, "C", bases, 0) == want and want[3]
    assert T.left_align_letters(lambda i: rep[i], len(rep), T.LA_INS, 120, "C", "AC" * 31, 0)[0] == 0      # a shift of 120 with L = 62
    long = "CA" * 32                                                                         # 64 bases: no key holds it
    assert _host(candgen, rep, T.LA_INS, 120, "C", long, 0) == (120, "C", long, False, False)


# ---- 2. truthset.left_align_record and the pairing -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fasta(tmp_path_factory):
    from dl4vc_amd.bamio import FastaFile
    d = tmp_path_factory.mktemp("lafasta")
    path = K.write_fasta(L.make_genome(), str(d / "ref.fa"), True)
    return path, FastaFile(path)


def test_left_align_record(fasta):
    _, fa = fasta
    assert T.left_align_record(fa, "ctgA", 204, "TT", "T") == (200, "GT", "G")              # POS is 1-based
    assert T.left_align_record(fa, "ctgA", 204, "TT", ("T",)) == (200, "GT", ("G",))
    assert T.left_align_record(fa, "ctgA", 608, "C", "CAC") == (600, "G", "GAC")
    assert T.left_align_record(fa, "ctgA", 610, "C", "CACAC") == (600, "G", "GACAC")
    assert T.left_align_record(fa, "ctgA", 5, "AA", "A") == (1, "GA", "G")
    assert T.left_align_record(fa, "ctgA", 200, "GT", "G") == (200, "GT", "G")              # left-aligned already
    assert T.left_align_record(fa, "ctgA", 2309, "AA", "A") == (2307, "AA", "A")            # stops behind the N
    for rec in ((204, "T", "G"), (204, "TT", "GG"), (204, "TTT", "TG"), (204, "TT", ("T", "TTT")), (204, "TT", "T,TTT"),
                (204, "TT", "G"), (204, "TT", "."), (204, "TT", ()), (204, "TN", "T"), (204, "TA", "T"), (5001, "AA", "A")):
        assert T.left_align_record(fa, "ctgA", *rec) == rec, rec
    assert T.left_align_record(fa, "absent", 204, "TT", "T") == (204, "TT", "T")


def _vcf(path, records):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for chrom, pos, ref, alt in records:
            f.write("%s\t%d\t.\t%s\t%s\t50\t.\t.\n" % (chrom, pos, ref, alt))
    return str(path)


def test_isec_pairs_a_right_placed_candidate_only_with_the_flag(fasta, tmp_path):
    fa_path, _ = fasta
    truth = _vcf(tmp_path / "truth.vcf", [("ctgA", 200, "GT", "G"), ("ctgA", 300, "A", "C"), ("ctgA", 600, "G", "GAC")])
    cand = _vcf(tmp_path / "cand.vcf", [("ctgA", 204, "TT", "T"), ("ctgA", 300, "A", "C"), ("ctgA", 608, "C", "CAC"), ("ctgA", 700, "A", "T")])
    assert [len(o) for o in T.isec(truth, cand)] == [2, 3, 1, 1]
    outs = T.isec(truth, cand, left_align=fa_path)
    assert [len(o) for o in outs] == [0, 1, 3, 3]
    assert [r[2] for r in outs[T.SHARED_B]] == [204, 300, 608]                               # the lines are the inputs' own
    tool = os.path.join(ROOT, "tools", "vcf_isec.py")
    for flag, want in (([], "2 private to A, 3 private to B, 1 shared"), (["--left-align", fa_path], "0 private to A, 1 private to B, 3 shared")):
        r = subprocess.run([sys.executable, tool, "-p", str(tmp_path / "isec")] + flag + [truth, cand], capture_output=True, text=True)
        assert r.returncode == 0 and want in r.stderr, r.stderr
    assert "\t204\t.\tTT\tT\t" in open(str(tmp_path / "isec" / "0003.vcf")).read()
    metrics = os.path.join(ROOT, "tools", "called_variant_metrics.py")
    for flag, want in (([], "Indel Recall = 0.0"), (["--left-align", fa_path], "Indel Recall = 1.0")):
        r = subprocess.run([sys.executable, metrics, "--truth_variants", truth, "--called_variants", cand] + flag, capture_output=True, text=True)
        assert r.returncode == 0 and want in r.stdout, (r.stdout, r.stderr)


# ---- 3. the command lines -------------------------------------------------------------------------------------------------------
def test_left_align_without_reference_is_refused_before_any_device_work(tmp_path):
    tool = os.path.join(ROOT, "tools", "candidate_generator.py")
    r = subprocess.run([sys.executable, tool, "--input", str(tmp_path / "absent.bam"), "--output", str(tmp_path / "o.vcf"), "--left-align"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--left-align needs --reference" in r.stderr and not (tmp_path / "o.vcf").exists()
    from dl4vc_amd import candidates as C
    with pytest.raises(ValueError, match="left_align needs reference"):
        C.generate(str(tmp_path / "absent.bam"), str(tmp_path / "o.vcf"), left_align=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "candgen_rate.py"), "--bam", str(tmp_path / "absent.bam"), "--left-align"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--left-align needs --reference" in r.stderr and not (tmp_path / "absent.bam").exists()


def _fake_python(tmp_path):
    """A ``python`` that records its arguments, one call per line, and succeeds."""
    bindir = tmp_path / "bin"
    bindir.mkdir()
    log = tmp_path / "calls.txt"
    (bindir / "python").write_text("#!/bin/bash\necho \"$@\" >> %s\n" % log)
    (bindir / "python").chmod(0o755)
    return dict(os.environ, PATH="%s:%s" % (bindir, os.environ["PATH"])), log


def test_scripts_pass_L_on_to_the_tools(tmp_path):
    env, log = _fake_python(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "make_training_data.sh"), "-i", "x.bam", "-r", "ref.fa", "-t", "truth.vcf", "-o", str(out),
                        "-L", "-n"], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    calls = log.read_text().splitlines()
    gen = [c for c in calls if "candidate_generator.py" in c]
    isec = [c for c in calls if "vcf_isec.py" in c]
    assert len(gen) == 1 and "--reference ref.fa" in gen[0] and "--left-align" in gen[0]
    assert len(isec) == 1 and "--left-align ref.fa truth.vcf" in isec[0]
    log.unlink()
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "make_training_data.sh"), "-i", "x.bam", "-r", "ref.fa", "-t", "truth.vcf",
                        "-o", str(tmp_path / "out2"), "-n"], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "--left-align" not in log.read_text() and "--reference" not in log.read_text()
    log.unlink()
    # call_variants.sh: the fake python writes no candidates.vcf, so the script stops behind the first stage
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", "model", "-o", str(tmp_path / "cv"), "-i", "x.bam", "-r", "ref.fa", "-L"],
                       env=env, capture_output=True, text=True)
    gen = [c for c in log.read_text().splitlines() if "candidate_generator.py" in c]
    assert len(gen) == 1 and "--reference ref.fa" in gen[0] and "--left-align" in gen[0]
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", "model", "-o", str(tmp_path / "cv2"), "-i", "x.bam", "-L"],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 1 and "-L left-aligns" in r.stdout


def test_header_binding_and_struct_agree(candgen):
    import re
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dl4vc_candgen.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} cg_left_align_stats;", text).group(1)
    assert re.findall(r"int64_t\s+([a-z_]+)\s*;", body) == [f[0] for f in candgen.LeftAlignStats._fields_]
    lib = candgen.load_library()
    for name in ("cg_set_left_align", "cg_get_left_align_stats", "cg_left_align_host"):
        assert name in candgen.SYMBOLS and hasattr(lib, name)
