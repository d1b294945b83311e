#!/usr/bin/env python
"""BAM -> the BAM of the reads a name-hash subsampling keeps (the rule of `samtools view --subsample F --subsample-seed S`,
dl4vc_amd/bamio.py::SampleRule, csrc/bam_frame.h).  Every kept record is written as its bytes lie in the input, not re-packed, in
the input's order and under the input's header; OUT.bam.bai is written beside it.  What every BAM consumer of this project
computes on IN.bam with --subsample F --subsample-seed S, it computes on OUT.bam without.

    subsample_bam.py IN.bam OUT.bam --subsample 0.6 --subsample-seed 7
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def subsample_bam(src: str, dst: str, subsample, level: int = 6):
    """Writes ``dst`` and ``dst + ".bai"`` (no index for an input that is not coordinate-sorted: the records keep the input's
    order either way); returns (records seen, records kept, whether the index was written)."""
    from dl4vc_amd.bamio import BamFile, BamWriter, SampleRule, build_bai
    rule = SampleRule.of(subsample)
    seen = kept = 0
    with BamFile(src, index="") as bam:
        with BamWriter(dst, list(zip(bam.references, bam.lengths)), header_text=bam.header_text, level=level) as out:
            for body in bam.raw_records():
                seen += 1
                if rule.keeps_record(body):
                    out.write_raw(body)
                    kept += 1
    try:
        build_bai(dst, dst + ".bai")
    except ValueError:                                        # (not coordinate-sorted)
        return seen, kept, False
    return seen, kept, True


def main(argv=None) -> int:
    from dl4vc_amd import subsample
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    p.add_argument("input", metavar="IN.bam", help="coordinate-sorted input BAM")
    p.add_argument("output", metavar="OUT.bam", help="output BAM (OUT.bam.bai is written as well)")
    subsample.add_flags(p)
    args = p.parse_args(argv)
    if args.subsample is None and args.subsample_seed is None:
        p.error("--subsample F is required")
    rule = subsample.parse(p, args)
    if not os.path.isfile(args.input):
        p.error("%s is not a file" % args.input)
    if os.path.abspath(args.input) == os.path.abspath(args.output):
        p.error("OUT.bam must not be IN.bam")
    seen, kept, indexed = subsample_bam(args.input, args.output, rule)
    print(subsample.report_line(seen, kept, rule))
    if not indexed:
        print("%s is not coordinate-sorted: no %s.bai written" % (args.input, args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
