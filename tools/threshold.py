#!/usr/bin/env python
"""Best-F1 variant-call and zygosity thresholds from the scored VCF of a labelled test set: the reference's
tools/threshold.py with its flags and its printed text, without scikit-learn.

    threshold.py --input_file epoch1_model_test.vcf --truth_file truth.vcf[.gz] [--no_truncate_at_full_recall]

The score of a site is 1 - NV and its zygosity score OV (ID column BP=;NV=;HV=;OV=); a site is homozygous when its last
column is GT:1/1 or GT:1|1.  Truth records whose REF and ALT are both longer than 1 are canonicalised (common suffix
dropped; a suffix that differs stops the run with AssertionError, as in the reference).  Sites match on the exact text
chrom, pos, ref, alt, so a multi-allelic truth ALT matches nothing.  Truth variants that are missing from the input are the
"base FN" and enter the second curves with score -1.

The precision-recall curve is restated in numpy (dl4vc_amd/truthset.py).  By default it is scikit-learn 0.22-0.24's, the
version the reference ran with: the curve stops at the first threshold that reaches full recall.
--no_truncate_at_full_recall gives scikit-learn >= 1.1's full curve instead.

Differences from the reference: the input may only be a text VCF (as in the reference), the truth may be plain, gzip or BGZF
text; a truth file with exactly one record is read as one record (numpy's genfromtxt would return a flat row there).
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_truth(path):
    """(chrom, pos, ref, alt) text of every truth record, split as np.genfromtxt(comments='#', delimiter='\\t',
    usecols=(0, 1, 3, 4)) splits it: text after a '#' dropped, spaces / CR / LF stripped from the line's ends, blank lines
    skipped."""
    from dl4vc_amd.truthset import open_text_lines
    rows = []
    for n, line in enumerate(open_text_lines(path), 1):
        line = line.split("#")[0].strip(" \r\n")
        if not line:
            continue
        f = line.split("\t")
        if len(f) < 5:
            raise ValueError("Some errors were detected !\n    Line #%d (got %d columns instead of 4)" % (n, len(f)))
        rows.append([f[0], f[1], f[3], f[4]])
    return rows


def _base_recall(called, total):
    if total == 0:
        raise ZeroDivisionError("division by zero")
    return np.int64(called) / total


def main(argv=None):
    from dl4vc_amd.truthset import canonicalize_bases, optimal_threshold
    parser = argparse.ArgumentParser(description="Calculate thresholds for Conv1D model output")
    parser.add_argument("--input_file", type=str, default="", help="input vcf file")
    parser.add_argument("--truth_file", type=str, default="", help="truth set")
    parser.add_argument("--no_truncate_at_full_recall", action="store_true",
                        help="precision-recall curve of scikit-learn >= 1.1 (all thresholds) instead of 0.22-0.24's")
    args = parser.parse_args(argv)
    print(argparse.Namespace(input_file=args.input_file, truth_file=args.truth_file))
    truncate = not args.no_truncate_at_full_recall

    def best(labels, scores):
        return optimal_threshold(labels, scores, truncate)

    print("reading input")
    with open(args.input_file, "r") as f:
        inputs = [x.split("\t") for x in f if x[0] != "#"]

    print("extracting information from input")
    input_variants = np.array(["\t".join(x[:2] + x[3:5]) for x in inputs])
    lref = np.array([len(x[3]) for x in inputs], dtype=np.int64)
    lalt = np.array([len(x[4]) for x in inputs], dtype=np.int64)
    is_snp = (lref == 1) & (lalt == 1)
    is_insert = (lref == 1) & (lalt > 1)
    is_delete = (lref > 1) & (lalt == 1)
    is_long_indel = (lref >= 3) | (lalt >= 3)
    thresh = np.array([1 - float(x[2].split(";")[1].split("=")[1]) for x in inputs])
    ov = np.array([float(x[2].split(";")[3].split("=")[1]) for x in inputs])
    gt = np.array([x[-1].strip("\n") in ("GT:1|1", "GT:1/1") for x in inputs], dtype=bool)
    del inputs

    print("splitting snps and indel inputs")
    groups = {"snps": is_snp, "indels": ~is_snp, "long_indels": is_long_indel, "long_dels": is_long_indel & ~is_insert,
              "inserts": is_insert & ~is_long_indel, "deletes": is_delete & ~is_long_indel}
    inp = {g: (input_variants[m], thresh[m], ov[m], gt[m]) for g, m in groups.items()}

    print("reading truth set")
    truths = read_truth(args.truth_file)
    print(np.array(truths[:10]) if truths else np.array([]))
    for x in truths:
        if len(x[2]) > 1 and len(x[3]) > 1:
            x[2], x[3] = canonicalize_bases(x[2], x[3])

    print("extracting information from truth set")
    tref = np.array([len(x[2]) for x in truths], dtype=np.int64)
    talt = np.array([len(x[3]) for x in truths], dtype=np.int64)
    t_snp = (tref == 1) & (talt == 1)
    t_long = (tref >= 3) | (talt >= 3)
    t_del = (tref > 1) & (talt == 1)
    t_ins = (tref == 1) & (talt > 1)
    truth_variants = np.array(["\t".join(x) for x in truths], dtype=object)

    print("splitting snps and indel truth")
    tgroups = {"snps": t_snp, "indels": ~t_snp, "long_indels": t_long, "long_dels": t_long & ~t_ins,
               "inserts": t_ins & ~t_long, "deletes": t_del & ~t_long}
    truth = {g: set(truth_variants[m]) if len(truth_variants) else set() for g, m in tgroups.items()}
    truth_list = {g: truth_variants[m] if len(truth_variants) else [] for g, m in tgroups.items()}

    def base_fn(g):
        called = set(inp[g][0])
        hit = sum(1 for v in truth_list[g] if v in called)
        return len(truth_list[g]) - hit, _base_recall(hit, len(truth_list[g]))

    base_fn_snps, max_recall_snps = base_fn("snps")
    print("base FN number for SNPs: " + str(base_fn_snps) + ". Max recall = " + str(max_recall_snps))
    base_fn_indels, max_recall_indels = base_fn("indels")
    print("base FN number for indels: " + str(base_fn_indels) + ". Max recall = " + str(max_recall_indels))

    def is_true(g):
        t = truth[g]
        return np.array([v in t for v in inp[g][0]], dtype=bool)

    _, thresh_snps, ov_snps, gt_snps = inp["snps"]
    is_snp_true = is_true("snps")
    print("-------------------")
    print("variant call threshold for SNPs")
    opt_thresh_snp_1 = best(is_snp_true, thresh_snps)
    print("variant call threshold for SNPs with all FNs included - assigning them a score of -1")
    best(np.concatenate([is_snp_true, np.repeat(1, base_fn_snps)]), np.concatenate([thresh_snps, np.repeat(-1, base_fn_snps)]))

    print("-------------------")
    print("homozygosity threshold for SNPs")
    best(gt_snps, ov_snps)
    print("homozygosity threshold for SNPs using only variants called with variant-call threshold")
    best(gt_snps[thresh_snps >= opt_thresh_snp_1], ov_snps[thresh_snps >= opt_thresh_snp_1])

    _, thresh_indels, ov_indels, gt_indels = inp["indels"]
    is_indel_true = is_true("indels")
    print("-------------------")
    print("variant call threshold for indels")
    opt_thresh_indel_1 = best(is_indel_true, thresh_indels)
    print("variant call threshold for indels with base FNs included")
    best(np.concatenate([is_indel_true, np.repeat(1, base_fn_indels)]),
         np.concatenate([thresh_indels, np.repeat(-1, base_fn_indels)]))

    print("-------------------")
    print("homozygosity threshold for indels")
    best(gt_indels, ov_indels)
    print("homozygosity threshold for indels using only variants called with variant-call threshold")
    best(gt_indels[thresh_indels >= opt_thresh_indel_1], ov_indels[thresh_indels >= opt_thresh_indel_1])

    for g, title in (("long_dels", "*long* DELS"), ("long_indels", "*long* indels"), ("deletes", "*deletes*"),
                     ("inserts", "*inserts*")):
        print("-------------------")
        print("variant call threshold for %s" % title)
        best(is_true(g), inp[g][1])
        print("-------------------")
        print("homozygosity threshold for %s" % title)
        best(inp[g][3], inp[g][2])
    return 0


if __name__ == "__main__":
    sys.exit(main())
