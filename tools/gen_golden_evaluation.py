#!/usr/bin/env python
"""Writes tests/golden/evaluation_*.json.gz from the REFERENCE's own tools/threshold.py and tools/called_variant_metrics.py.

Run only where a checkout of the reference exists (``--reference DIR``); never in a test or on the GPU machine.  Nothing of
the reference is copied: its two scripts are executed here, at generation time, and their printed output recorded.

* threshold.py runs as a script (runpy, sys.argv set, in a scratch directory so that the paths it prints are the bare names
  ``scored.vcf`` / ``truth.vcf``) with a ``sklearn.metrics`` stand-in written to scikit-learn 0.22's algorithm (the curve
  stops at the first threshold of full recall), and a second time with the installed scikit-learn when there is one.
* called_variant_metrics.py runs on a ``pysam`` stand-in: ``VariantFile`` iterates parsed records (contig, pos, ref, alts)
  and ``bcftools.isec`` is routed to this project's isec (dl4vc_amd/truthset.py).  So the counting, the arithmetic and the
  printing are the reference's; the isec pairing rule is NOT pinned by these fixtures (there is no bcftools here): its cases
  are hand-written in tests/test_truthset.py.
"""
import argparse
import contextlib
import gzip
import io
import json
import os
import random
import runpy
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dl4vc_amd import truthset as T   # noqa: E402


# --- scikit-learn 0.22 stand-in ------------------------------------------------------------------------------------------

def _clf_curve_022(y_true, y_score):
    y_true = np.ravel(np.asarray(y_true))
    y_score = np.ravel(np.asarray(y_score))
    classes = np.unique(y_true)
    if not (np.array_equal(classes, [0, 1]) or np.array_equal(classes, [-1, 1]) or np.array_equal(classes, [0])
            or np.array_equal(classes, [-1]) or np.array_equal(classes, [1])):
        raise ValueError("Data is not binary and pos_label is not specified")
    pos_label = 1.
    y_true = (y_true == pos_label)
    desc_score_indices = np.argsort(y_score, kind="mergesort")[::-1]
    y_score = y_score[desc_score_indices]
    y_true = y_true[desc_score_indices]
    weight = 1.
    distinct_value_indices = np.where(np.diff(y_score))[0]
    threshold_idxs = np.r_[distinct_value_indices, y_true.size - 1]
    tps = np.cumsum(y_true * weight, dtype=np.float64)[threshold_idxs]
    fps = 1 + threshold_idxs - tps
    return fps, tps, y_score[threshold_idxs]


def precision_recall_curve_022(y_true, probas_pred, pos_label=None, sample_weight=None):
    fps, tps, thresholds = _clf_curve_022(y_true, probas_pred)
    precision = tps / (tps + fps)
    precision[np.isnan(precision)] = 0
    recall = tps / tps[-1]
    last_ind = tps.searchsorted(tps[-1])
    sl = slice(last_ind, None, -1)
    return np.r_[precision[sl], 1], np.r_[recall[sl], 0], thresholds[sl]


def sklearn_stub():
    sk = types.ModuleType("sklearn")
    m = types.ModuleType("sklearn.metrics")
    m.precision_recall_curve = precision_recall_curve_022
    sk.metrics = m
    return {"sklearn": sk, "sklearn.metrics": m}


# --- pysam stand-in -------------------------------------------------------------------------------------------------------

class Rec:
    def __init__(self, chrom, pos, ref, alts):
        self.contig, self.pos, self.ref, self.alts = chrom, pos, ref, alts


class VariantFile:
    def __init__(self, path, mode="r"):
        self.recs = [Rec(r[1], r[2], r[3], r[4] or None) for r in T.VcfReader(path)]

    def __iter__(self):
        return iter(self.recs)


def pysam_stub():
    ps = types.ModuleType("pysam")
    bc = types.ModuleType("pysam.bcftools")

    def isec(*args):
        assert len(args) == 4 and args[0] == "-p", args
        T.isec_to_dir(args[2], args[3], args[1])

    bc.isec = isec
    ps.VariantFile = VariantFile
    ps.bcftools = bc
    return {"pysam": ps, "pysam.bcftools": bc}


@contextlib.contextmanager
def modules(mods):
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def run_script(path, argv, cwd, mods):
    """(stdout, name of the exception it ended with or None)."""
    out = io.StringIO()
    old_argv, old_cwd = sys.argv, os.getcwd()
    err = None
    sys.argv = [os.path.basename(path)] + argv
    os.chdir(cwd)
    try:
        with modules(mods), contextlib.redirect_stdout(out), np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                runpy.run_path(path, run_name="__main__")
    except Exception as e:                          # the reference's own failures are recorded, not hidden
        err = type(e).__name__
    finally:
        sys.argv = old_argv
        os.chdir(old_cwd)
    return out.getvalue(), err


# --- random inputs --------------------------------------------------------------------------------------------------------

HEADER = ("##fileformat=VCFv4.2\n##contig=<ID=chr1,length=100000>\n##contig=<ID=chr2,length=100000>\n"
          "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")


def _bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def make_case(seed, n_sites=160, bad_canonical=False, no_positives=False):
    """no_positives: short insertions never in the truth and deletions never homozygous, so two curves have no positive
    label (the case where the two scikit-learn curves differ)."""
    rng = random.Random(seed)
    truth, calls, scored = [], [], []
    for chrom in ("chr1", "chr2"):
        pos = 100
        for _ in range(n_sites // 2):
            pos += rng.randint(0, 40)               # 0: two sites at one position
            b = _bases(rng, 1)
            kind = rng.choice(["snp"] * 5 + ["ins"] * 2 + ["del"] * 2 + ["longdel", "longins", "mnp", "multi", "canon"])
            if kind == "snp":
                ref, alt = b, rng.choice([c for c in "ACGT" if c != b])
            elif kind == "ins":
                ref, alt = b, b + _bases(rng, 1)
            elif kind == "longins":
                ref, alt = b, b + _bases(rng, rng.randint(2, 5))
            elif kind == "del":
                ref, alt = b + _bases(rng, 1), b
            elif kind == "longdel":
                ref, alt = b + _bases(rng, rng.randint(2, 6)), b
            elif kind == "mnp":                     # the last base shared: threshold.py asserts that of a truth MNP
                x, y = rng.sample("ACGT", 2)
                ref, alt = x + b, y + b
            elif kind == "multi":
                x, y = rng.sample([c for c in "ACGT" if c != b], 2)
                ref, alt = b, "%s,%s" % (x, y)
            else:                                   # canonicalisable truth indel: TTA > TTATA  ->  T > TAT
                suf = _bases(rng, rng.randint(1, 3))
                ref, alt = b + suf, b + _bases(rng, rng.randint(1, 3)) + suf
            in_truth = rng.random() < 0.7 and not (no_positives and kind == "ins")
            gt = rng.choice(["0/1", "1/1", "1|1", "0|1"]) if kind != "multi" else "1/2"
            if no_positives and kind in ("del", "longdel"):
                gt = "0/1"
            if in_truth:
                filt = rng.choice(["PASS", "PASS", "LowQual", "."])
                truth.append((chrom, pos, ref, alt, "%s\t50\t%s\t.\tGT\t%s" % (".", filt, gt)))
                if rng.random() < 0.05:             # a duplicate key in the truth
                    truth.append((chrom, pos, ref, alt, ".\t50\tPASS\t.\tGT\t%s" % gt))
            called = rng.random() < (0.75 if in_truth else 0.6)
            if called:
                calt = alt
                if kind == "multi" and rng.random() < 0.5:
                    calt = ",".join(reversed(alt.split(",")))          # same ALT set, other order
                elif kind == "multi" and rng.random() < 0.5:
                    calt = alt.split(",")[0]                             # a split allele: pairs with nothing
                reps = 2 if rng.random() < 0.05 else 1                   # duplicate calls
                for _ in range(reps):
                    calls.append((chrom, pos, ref, calt, ".\t%d\t%s\t.\tGT\t%s" % (rng.randint(1, 60),
                                                                                rng.choice(["PASS", "RefCall"]), gt)))
            # the scored VCF: one ALT per record, the canonical form of a canonicalisable indel
            sref, salts = ref, alt.split(",")
            if kind == "canon":
                t = min(len(ref), len(alt)) - 1
                sref, salts = ref[:-t], [alt[:-t]]
            if called or rng.random() < 0.3:
                for sa in salts:
                    nv = round(rng.random(), rng.choice([1, 2, 2, 3]))
                    ov = round(rng.random(), 2)
                    ids = "BP=%.8f;NV=%.8f;HV=%.8f;OV=%.8f" % (rng.random(), nv, rng.random(), ov)
                    last = "GT:%s" % gt if in_truth and rng.random() < 0.9 else "1:50"
                    scored.append((chrom, pos, sref, sa, "%s\t50\t.\tDP=10;AF=0.5\tGT:GQ\t1:50\t%s" % (ids, last)))
            if rng.random() < 0.1:                  # false positives with long / odd alleles
                fref, falt = b + _bases(rng, 3), b
                calls.append((chrom, pos, fref, falt, ".\t9\tPASS\t.\tGT\t0/1"))
    if bad_canonical:
        truth.append(("chr2", 999999, "ACG", "TTC", ".\t50\tPASS\t.\tGT\t0/1"))
    return _text(truth), _text(calls), _scored_text(scored)


def _text(recs):
    # rest = "ID\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE": REF and ALT go between ID and QUAL
    recs = sorted(recs, key=lambda r: (r[0], r[1]))
    return HEADER + "".join("%s\t%d\t%s\t%s\t%s\n" % (c, p, rest.split("\t", 1)[0], r, a + "\t" + rest.split("\t", 1)[1])
                            for c, p, r, a, rest in recs)


def _scored_text(recs):
    recs = sorted(recs, key=lambda r: (r[0], r[1]))
    return HEADER + "".join("%s\t%d\t%s\t%s\t%s\t%s\n" % (c, p, rest.split("\t", 1)[0], r, a, rest.split("\t", 1)[1])
                            for c, p, r, a, rest in recs)


def bed_text(seed):
    rng = random.Random(seed + 1000)
    lines = []
    for chrom in ("chr1", "chr2"):
        s = 0
        for _ in range(4):
            s += rng.randint(50, 800)
            e = s + rng.randint(100, 900)
            lines.append("%s\t%d\t%d\n" % (chrom, s, e))
            s = e
    return "".join(lines)


def filter_bed(text, bed_path):
    bed = T.BedRegions(bed_path)
    out = []
    for line in text.splitlines(True):
        if line.startswith("#"):
            out.append(line)
        else:
            f = line.split("\t")
            if bed.contains(f[0], int(f[1])):
                out.append(line)
    return "".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    thr = os.path.join(a.reference, "tools", "threshold.py")
    cvm = os.path.join(a.reference, "tools", "called_variant_metrics.py")
    try:
        import sklearn.metrics                                   # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    cases = [("random1", 1, {}), ("random2", 2, {}), ("nopos", 3, {"no_positives": True}),
             ("badcanon", 4, {"bad_canonical": True})]
    for name, seed, kw in cases:
        truth, calls, scored = make_case(seed, **kw)
        fx = {"truth": truth, "calls": calls, "scored": scored, "bed": bed_text(seed), "threshold": {}, "metrics": [],
              "counts": []}
        with tempfile.TemporaryDirectory() as d:
            for fn, txt in (("truth.vcf", truth), ("calls.vcf", calls), ("scored.vcf", scored), ("r.bed", fx["bed"])):
                open(os.path.join(d, fn), "w").write(txt)
            argv = ["--input_file", "scored.vcf", "--truth_file", "truth.vcf"]
            out, err = run_script(thr, argv, d, sklearn_stub())
            fx["threshold"]["truncate"] = {"stdout": out, "error": err}
            if have_sklearn:
                out, err = run_script(thr, argv, d, {})
                fx["threshold"]["full"] = {"stdout": out, "error": err}
            regions = [None, "chr1:1:2000", "chr2:500:100000", "chr1:1:1"]
            for region in regions:
                argv = ["--truth_variants", "truth.vcf", "--called_variants", "calls.vcf"]
                if region:
                    argv += ["--region", region]
                out, err = run_script(cvm, argv, d, pysam_stub())
                fx["metrics"].append({"region": region, "bed": False, "stdout": out, "error": err})
            # the --regions_bed extension: the reference on inputs filtered to the BED beforehand
            for fn in ("truth", "calls"):
                open(os.path.join(d, fn + "_bed.vcf"), "w").write(filter_bed(locals()[fn], os.path.join(d, "r.bed")))
            out, err = run_script(cvm, ["--truth_variants", "truth_bed.vcf", "--called_variants", "calls_bed.vcf"], d,
                                  pysam_stub())
            fx["metrics"].append({"region": None, "bed": True, "stdout": out, "error": err})
            # count_variant_types itself on the three isec outputs
            with modules(pysam_stub()):
                mod = runpy.run_path(cvm, run_name="reference_cvm")
            isec_dir = os.path.join(d, "isec")
            T.isec_to_dir(os.path.join(d, "truth.vcf"), os.path.join(d, "calls.vcf"), isec_dir)
            for i in range(3):
                for region in regions:
                    chrom, start, end = (None, None, None)
                    if region:
                        chrom, start, end = region.split(":")
                        start, end = int(start), int(end)
                    buf = io.StringIO()
                    with contextlib.redirect_stdout(buf):
                        tup = mod["count_variant_types"](VariantFile(os.path.join(isec_dir, "%04d.vcf" % i)), chrom, start,
                                                         end)
                    fx["counts"].append({"file": i, "region": region, "tuple": list(tup), "stdout": buf.getvalue()})
        path = os.path.join(a.out, "evaluation_%s.json.gz" % name)
        with gzip.GzipFile(path, "wb", mtime=0) as f:
            f.write(json.dumps(fx, sort_keys=True).encode())
        print("%s: %d bytes; threshold %s; metrics errors %s" % (path, os.path.getsize(path),
              {k: v["error"] for k, v in fx["threshold"].items()}, [m["error"] for m in fx["metrics"]]))


if __name__ == "__main__":
    main()
