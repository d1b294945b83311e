#!/usr/bin/env python
"""SNP and indel precision and recall of called variants against a truth VCF: the reference's
tools/called_variant_metrics.py with its flags and its output, without pysam or bcftools.

    called_variant_metrics.py --truth_variants truth.vcf.gz --called_variants called_variants.vcf.gz [--region 20:1:5000000]
                              [--regions_bed confident.bed]

The truth and the calls are paired in process as `bcftools isec -p DIR truth calls` pairs them (dl4vc_amd/truthset.py: same
CHROM, POS, REF and ALT set; no normalisation): 0000 = false negatives, 0001 = false positives, 0002 = true positives.
Records are classified by REF and the FIRST ALT only; MNPs and complex alleles are printed as `Unknown alelle: ...` and not
counted.  `--region chrom:start:end` keeps 1-based POS in [start, end].

Differences from the reference:
* where a count is zero and the reference stops with ZeroDivisionError, the ratio is printed as `nan` and all four lines are
  printed;
* `--regions_bed BED` (an extension) keeps, in every set, only records whose 0-based `POS - 1` lies inside a BED interval;
* inputs need no index, and may be plain text as well as bgzip / gzip;
* `--left-align REF.fa` (an extension) moves the simple indels of both the truth and the calls to their left-most placement on
  the FASTA before they are paired (dl4vc_amd/truthset.py::left_align_record); MNPs, complex alleles and multi-allelic records
  are compared as they are.
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    from dl4vc_amd import truthset as T
    parser = argparse.ArgumentParser(description="Analyse VCF files")
    parser.add_argument("--truth_variants", help="truth set")
    parser.add_argument("--called_variants", help="called set")
    parser.add_argument("--region", type=str, default=None,
                        help="region in form chrom:start:end. If not set defaults to whole genome")
    parser.add_argument("--regions_bed", type=str, default=None,
                        help="BED file: count only records whose POS-1 lies in one of its intervals (not in the reference)")
    parser.add_argument("--left-align", dest="left_align", type=str, default=None, metavar="REF.fa",
                        help="left-align the simple indels of both inputs on this FASTA before pairing (not in the reference)")
    args = parser.parse_args(argv)
    if args.left_align is not None and not os.path.isfile(args.left_align):
        parser.error("--left-align %s is not a readable file" % args.left_align)

    if args.region is not None:
        chrom, start, end = args.region.split(":")
        start = int(start)
        end = int(end)
    else:
        chrom = start = end = None

    bed = T.BedRegions(args.regions_bed) if args.regions_bed else None
    sets = ([], [], [])                           # 0000 false negatives, 0001 false positives, 0002 true positives

    def keep(o, rec):
        if o <= T.SHARED_A and (bed is None or bed.contains(rec[1], rec[2])):
            sets[o].append(rec[1:])

    try:
        T.isec_stream(args.truth_variants, args.called_variants, keep,
                      normalise=T.record_left_aligner(args.left_align) if args.left_align else None)
        fn_snps, fn_insertions, fn_deletions = T.count_variant_types(sets[0], chrom, start, end)
        fp_snps, fp_insertions, fp_deletions = T.count_variant_types(sets[1], chrom, start, end)
        tp_snps, tp_insertions, tp_deletions = T.count_variant_types(sets[2], chrom, start, end)
    except T.VcfError as e:
        print("called_variant_metrics.py: %s" % e, file=sys.stderr)
        return 1

    fn_indels = fn_insertions + fn_deletions
    tp_indels = tp_insertions + tp_deletions
    fp_indels = fp_insertions + fp_deletions

    print("SNP Recall = {}".format(T.ratio(tp_snps, tp_snps + fn_snps)))
    print("SNP Precision = {}".format(T.ratio(tp_snps, tp_snps + fp_snps)))
    print("Indel Recall = {}".format(T.ratio(tp_indels, tp_indels + fn_indels)))
    print("Indel Precision = {}".format(T.ratio(tp_indels, tp_indels + fp_indels)))
    print("Cleaning up")
    return 0


if __name__ == "__main__":
    sys.exit(main())
