"""Comparison against a truth VCF (dl4vc_amd/truthset.py, tools/vcf_isec.py, tools/called_variant_metrics.py,
tools/threshold.py), host only.

threshold.py's and called_variant_metrics.py's printed text, count_variant_types' tuples and the precision-recall curve are
pinned to the reference's own scripts (tests/golden/evaluation_*.json.gz, written by tools/gen_golden_evaluation.py with a
scikit-learn 0.22 stand-in and with the installed scikit-learn).  The isec pairing rule is NOT pinned by those fixtures:
there is no bcftools here, so its cases below are hand-written from the bcftools manual's rule for the default collapse
mode ("only records with identical REF and ALT alleles are compatible")."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import truthset as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("random1", "random2", "nopos", "badcanon")


def load(name):
    with gzip.open(os.path.join(GOLDEN, "evaluation_%s.json.gz" % name), "rt") as f:
        return json.load(f)


def tool(name, args, cwd):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", name)] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=300)


def write_inputs(fx, d):
    for fn, key in (("truth.vcf", "truth"), ("calls.vcf", "calls"), ("scored.vcf", "scored"), ("r.bed", "bed")):
        (d / fn).write_text(fx[key])


# --- threshold.py ----------------------------------------------------------------------------------------------------------

def _threshold_cases():
    for name in NAMES:
        for mode in ("truncate", "full"):
            yield pytest.param(name, mode, id="%s-%s" % (name, mode))


@pytest.mark.parametrize("name,mode", list(_threshold_cases()))
def test_threshold_prints_what_the_reference_prints(name, mode, tmp_path):
    fx = load(name)
    want = fx["threshold"].get(mode)
    if want is None:
        pytest.skip("fixture generated without scikit-learn installed: no full-curve output recorded")
    write_inputs(fx, tmp_path)
    args = ["--input_file", "scored.vcf", "--truth_file", "truth.vcf"]
    if mode == "full":
        args.append("--no_truncate_at_full_recall")
    r = tool("threshold.py", args, tmp_path)
    assert r.stdout == want["stdout"]
    if want["error"] is None:
        assert r.returncode == 0, r.stderr[-2000:]
    else:
        assert r.returncode != 0 and want["error"] in r.stderr, r.stderr[-2000:]


def test_the_two_curve_modes_differ_on_a_fixture():
    fx = load("nopos")
    assert fx["threshold"]["truncate"]["stdout"] != fx["threshold"]["full"]["stdout"]


def test_truncated_curve_of_the_issue_example():
    p, r, t = T.precision_recall_curve([1, 1, 0, 0], [.9, .8, .3, .1])
    assert list(t) == [.8, .9] and list(p) == [1, 1, 1] and list(r) == [1, .5, 0]
    p, r, t = T.precision_recall_curve([1, 1, 0, 0], [.9, .8, .3, .1], truncate_at_full_recall=False)
    assert list(t) == [.1, .3, .8, .9]


def test_full_curve_equals_installed_sklearn_on_ties():
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for trial in range(60):
        n = int(rng.integers(1, 400))
        scores = np.round(rng.random(n), int(rng.integers(1, 3)))          # many ties
        labels = rng.random(n) < rng.random()
        if trial % 10 == 0:
            labels[:] = True
        for lab in (labels, labels.astype(np.int64)):
            want = sk.precision_recall_curve(lab, scores)
            got = T.precision_recall_curve(lab, scores, truncate_at_full_recall=False)
            for g, w in zip(got, want):
                assert g.shape == w.shape and np.array_equal(g, w), trial


def test_curve_refuses_empty_input():
    with pytest.raises(ValueError):
        T.precision_recall_curve(np.zeros(0, bool), np.zeros(0))


# --- called_variant_metrics.py ---------------------------------------------------------------------------------------------

def _region_args(region):
    if region is None:
        return None, None, None
    c, s, e = region.split(":")
    return c, int(s), int(e)


@pytest.mark.parametrize("name", NAMES)
def test_count_variant_types_matches_reference(name, tmp_path):
    fx = load(name)
    write_inputs(fx, tmp_path)
    outs = T.isec(str(tmp_path / "truth.vcf"), str(tmp_path / "calls.vcf"))
    for c in fx["counts"]:
        printed = []
        got = T.count_variant_types([r[1:] for r in outs[c["file"]]], *_region_args(c["region"]), out=printed.append)
        assert list(got) == c["tuple"], c
        assert "".join(p + "\n" for p in printed) == c["stdout"], c


@pytest.mark.parametrize("name", NAMES)
def test_called_variant_metrics_prints_what_the_reference_prints(name, tmp_path):
    fx = load(name)
    write_inputs(fx, tmp_path)
    for m in fx["metrics"]:
        if m["bed"]:
            continue
        args = ["--truth_variants", "truth.vcf", "--called_variants", "calls.vcf"]
        if m["region"]:
            args += ["--region", m["region"]]
        r = tool("called_variant_metrics.py", args, tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        if m["error"] is None:
            assert r.stdout == m["stdout"], m["region"]
        else:
            # the reference stops with ZeroDivisionError; here every ratio whose denominator is 0 is printed as nan
            assert m["error"] == "ZeroDivisionError"
            assert r.stdout.startswith(m["stdout"])
            tail = r.stdout[len(m["stdout"]):].splitlines()
            assert [l.split(" = ")[0] for l in tail[:4]] == ["SNP Recall", "SNP Precision", "Indel Recall", "Indel Precision"]
            assert "nan" in [l.split(" = ")[1] for l in tail[:4]] and tail[4] == "Cleaning up"


@pytest.mark.parametrize("name", NAMES)
def test_regions_bed_equals_the_reference_on_prefiltered_inputs(name, tmp_path):
    fx = load(name)
    write_inputs(fx, tmp_path)
    want = [m for m in fx["metrics"] if m["bed"]][0]
    assert want["error"] is None
    r = tool("called_variant_metrics.py", ["--truth_variants", "truth.vcf", "--called_variants", "calls.vcf",
                                           "--regions_bed", "r.bed"], tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == want["stdout"]
    plain = [m for m in fx["metrics"] if not m["bed"] and m["region"] is None][0]
    assert r.stdout != plain["stdout"]                     # the BED really removes records


def test_bed_regions_are_zero_based_half_open(tmp_path):
    (tmp_path / "r.bed").write_text("track name=x\nchr1\t10\t20\nchr1\t15\t30\nchr2\t0\t1\n")
    bed = T.BedRegions(str(tmp_path / "r.bed"))
    assert [p for p in range(1, 40) if bed.contains("chr1", p)] == list(range(11, 31))
    assert bed.contains("chr2", 1) and not bed.contains("chr2", 2) and not bed.contains("chr3", 1)


# --- isec: hand-written cases of the rule (NOT pinned to bcftools, which does not exist here) ------------------------------

HA = "##fileformat=VCFv4.2\n##source=A\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
HB = "##fileformat=VCFv4.2\n##source=B\n##contig=<ID=c1>\n##contig=<ID=c2>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def rec(chrom, pos, ref, alt, filt="PASS", info="."):
    return "%s\t%d\t.\t%s\t%s\t50\t%s\t%s\n" % (chrom, pos, ref, alt, filt, info)


def run_isec(tmp_path, a_lines, b_lines, ha=HA, hb=HB):
    a, b = tmp_path / "a.vcf", tmp_path / "b.vcf"
    a.write_text(ha + "".join(a_lines))
    b.write_text(hb + "".join(b_lines))
    r = tool("vcf_isec.py", ["-p", "out", "a.vcf", "b.vcf"], tmp_path)
    assert r.returncode == 0, r.stderr
    return [(tmp_path / "out" / ("%04d.vcf" % i)).read_text() for i in range(4)]


def test_isec_pairs_exact_keys_and_keeps_headers_and_order(tmp_path):
    a = [rec("c1", 5, "A", "G"), rec("c1", 9, "AT", "A", filt="LowQual"), rec("c2", 3, "C", "CT"), rec("c2", 7, "G", "T")]
    b = [rec("c1", 5, "A", "G", filt="RefCall", info="DP=3"), rec("c1", 9, "AT", "A"), rec("c1", 12, "T", "C"),
         rec("c2", 3, "C", "CTT"), rec("c2", 7, "G", "T")]
    o = run_isec(tmp_path, a, b)
    assert o[0] == HA + a[2]                                # private to A (CTT is not CT)
    assert o[1] == HB + b[2] + b[3]                         # private to B, in B's order
    assert o[2] == HA + a[0] + a[1] + a[3]                  # A's shared records, A's text (FILTER ignored)
    assert o[3] == HB + b[0] + b[1] + b[4]                  # B's shared records, B's text
    readme = (tmp_path / "out" / "README.txt").read_text()
    assert "0000.vcf\tfor records private to\ta.vcf" in readme and "0003.vcf\tfor records from b.vcf shared by both" in readme


def test_isec_multiallelic_pairs_only_the_same_alt_set(tmp_path):
    a = [rec("c1", 5, "A", "G,T"), rec("c1", 8, "C", "A,G")]
    b = [rec("c1", 5, "A", "G"), rec("c1", 5, "A", "T"), rec("c1", 8, "C", "G,A")]
    o = run_isec(tmp_path, a, b)
    assert o[0] == HA + a[0] and o[1] == HB + b[0] + b[1]
    assert o[2] == HA + a[1] and o[3] == HB + b[2]


def test_isec_duplicates_pair_one_for_one_in_file_order(tmp_path):
    a = [rec("c1", 5, "A", "G", info="a1"), rec("c1", 5, "A", "G", info="a2"), rec("c1", 5, "A", "G", info="a3")]
    b = [rec("c1", 5, "A", "G", info="b1"), rec("c1", 5, "A", "G", info="b2")]
    o = run_isec(tmp_path, a, b)
    assert o[2] == HA + a[0] + a[1] and o[0] == HA + a[2]
    assert o[3] == HB + b[0] + b[1] and o[1] == HB
    o = run_isec(tmp_path, b, a, ha=HA, hb=HA)
    assert o[2] == HA + b[0] + b[1] and o[3] == HA + a[0] + a[1] and o[1] == HA + a[2]


def test_isec_copies_record_bytes_and_reads_bgzf(tmp_path):
    from dl4vc_amd.vcfpost import bgzf_compress
    a = [rec("c1", 5, "A", "G").replace("\n", "\r\n"), rec("c1", 6, "T", "C")]
    (tmp_path / "a.vcf.gz").write_bytes(bgzf_compress((HA + "".join(a)).encode()))
    (tmp_path / "b.vcf.gz").write_bytes(gzip.compress((HB + rec("c1", 5, "A", "G")).encode()))
    r = tool("vcf_isec.py", ["-p", "o", "a.vcf.gz", "b.vcf.gz"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o" / "0002.vcf").read_bytes() == (HA + a[0]).encode()
    assert (tmp_path / "o" / "0000.vcf").read_bytes() == (HA + a[1]).encode()


@pytest.mark.parametrize("lines,hdr,what", [
    ([rec("c1", 9, "A", "G"), rec("c1", 5, "A", "G")], HA, "c1:5 comes after c1:9"),
    ([rec("c1", 5, "A", "G"), rec("c2", 5, "A", "G"), rec("c1", 9, "A", "G")], HA, "contig c1 comes after c2"),
    ([rec("c2", 5, "A", "G"), rec("c1", 9, "A", "G")], HB, "contig c1 comes after c2"),
])
def test_isec_refuses_unsorted_input(tmp_path, lines, hdr, what):
    (tmp_path / "a.vcf").write_text(hdr + "".join(lines))
    (tmp_path / "b.vcf").write_text(HB + rec("c1", 5, "A", "G"))
    for args in (["a.vcf", "b.vcf"], ["b.vcf", "a.vcf"]):
        r = tool("vcf_isec.py", ["-p", "out"] + args, tmp_path)
        assert r.returncode != 0 and what in r.stderr and "a.vcf" in r.stderr, r.stderr
        assert not (tmp_path / "out" / "0000.vcf").exists()


def test_isec_accepts_header_contig_order(tmp_path):
    hb = HB.replace("##contig=<ID=c1>\n##contig=<ID=c2>\n", "##contig=<ID=c2,length=9>\n##contig=<ID=c1,length=9>\n")
    o = run_isec(tmp_path, [rec("c1", 5, "A", "G")], [rec("c2", 5, "A", "G"), rec("c1", 5, "A", "G")], hb=hb)
    assert o[2] == HA + rec("c1", 5, "A", "G") and o[1] == hb + rec("c2", 5, "A", "G")


def test_bcf_is_refused(tmp_path):
    (tmp_path / "a.bcf").write_bytes(gzip.compress(b"BCF\x02\x02" + b"\x00" * 32))
    (tmp_path / "b.vcf").write_text(HB)
    r = tool("vcf_isec.py", ["-p", "out", "a.bcf", "b.vcf"], tmp_path)
    assert r.returncode != 0 and "BCF" in r.stderr and "a.bcf" in r.stderr
    with pytest.raises(T.VcfError, match="BCF"):
        list(T.VcfReader(str(tmp_path / "a.bcf")))


@pytest.mark.parametrize("flag", [["-c", "all"], ["-n=2"], ["-w1"], ["-f", "PASS"], ["-O", "z"], ["-C"], ["--collapse", "snps"],
                                  ["-r", "c1"]])
def test_vcf_isec_refuses_other_bcftools_options(tmp_path, flag):
    (tmp_path / "a.vcf").write_text(HA)
    (tmp_path / "b.vcf").write_text(HB)
    r = tool("vcf_isec.py", ["-p", "out"] + flag + ["a.vcf", "b.vcf"], tmp_path)
    assert r.returncode != 0 and "not supported" in r.stderr and flag[0].split("=")[0] in r.stderr
    assert not (tmp_path / "out").exists()


def test_vcf_isec_needs_a_prefix_and_two_files(tmp_path):
    (tmp_path / "a.vcf").write_text(HA)
    assert "-p DIR is required" in tool("vcf_isec.py", ["a.vcf", "a.vcf"], tmp_path).stderr
    assert "exactly two" in tool("vcf_isec.py", ["-p", "o", "a.vcf"], tmp_path).stderr
