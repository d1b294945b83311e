#!/usr/bin/env python
"""BAM -> the BAM of the reads a name-hash subsampling keeps (the rule of `samtools view --subsample F --subsample-seed S`,
dl4vc_amd/bamio.py::SampleRule, csrc/bam_frame.h).  Every kept record is written as its bytes lie in the input, not re-packed, in
the input's order and under the input's header; OUT.bam.bai is written beside it.  What every BAM consumer of this project
computes on IN.bam with --subsample F --subsample-seed S, it computes on OUT.bam without.  The read filter flags (--min-mapq Q
--exclude-flags F --require-flags F, dl4vc_amd/bamio.py::ReadFilter) act in front of that rule, alone or with it: a record is
written iff it passes the filter and the rule.  --read-stats prints the census of the input's records.

    subsample_bam.py IN.bam OUT.bam --subsample 0.6 --subsample-seed 7
    subsample_bam.py IN.bam OUT.bam --min-mapq 20 --exclude-flags 0x704
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _count(census: dict, flag: int, mapq: int, flt) -> None:
    """One record into the ``read_*`` entries (``read_filter.ReadStats.flat``), in front of the filter."""
    keys = ["read_seen", "read_mapq_%d" % mapq] + ["read_flag_%d" % k for k in range(16) if flag >> k & 1]
    if flt is not None and not flt.passes(flag, mapq):
        keys.append("read_dropped_flags" if (flag & flt.exclude) or (flag & flt.require) != flt.require else "read_dropped_mapq")
    for k in keys:
        census[k] = census.get(k, 0) + 1


def subsample_bam(src: str, dst: str, subsample, level: int = 6, read_filter=None, census=None):
    """Writes ``dst`` and ``dst + ".bai"`` (no index for an input that is not coordinate-sorted: the records keep the input's
    order either way); returns (records seen, records kept, whether the index was written).  ``read_filter``: (exclude, require,
    min_mapq), in front of the sample rule -- ``seen`` then counts what passed it, and ``subsample`` may be None.  ``census`` (a
    dict): receives the ``read_*`` entries of ``read_filter.ReadStats.flat`` over every record of the input."""
    from dl4vc_amd.bamio import BamFile, BamWriter, ReadFilter, SampleRule, build_bai
    rule = SampleRule.of(subsample)
    flt = ReadFilter.of(read_filter)
    seen = kept = 0
    with BamFile(src, index="") as bam:
        with BamWriter(dst, list(zip(bam.references, bam.lengths)), header_text=bam.header_text, level=level) as out:
            for body in bam.raw_records():
                if census is not None:
                    _count(census, body[14] | body[15] << 8, body[9], flt)
                if flt is not None and not flt.passes_record(body):
                    continue
                seen += 1
                if rule is None or rule.keeps_record(body):
                    out.write_raw(body)
                    kept += 1
    if census is not None:
        census["read_kept"] = kept
    try:
        build_bai(dst, dst + ".bai")
    except ValueError:                                        # (not coordinate-sorted)
        return seen, kept, False
    return seen, kept, True


def main(argv=None) -> int:
    from dl4vc_amd import read_filter, subsample
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    p.add_argument("input", metavar="IN.bam", help="coordinate-sorted input BAM")
    p.add_argument("output", metavar="OUT.bam", help="output BAM (OUT.bam.bai is written as well)")
    subsample.add_flags(p)
    read_filter.add_flags(p)
    args = p.parse_args(argv)
    if args.subsample is None and args.subsample_seed is None and not read_filter.given(args):
        p.error("--subsample F is required")
    rule = subsample.parse(p, args)
    flt = read_filter.parse(p, args)
    if not os.path.isfile(args.input):
        p.error("%s is not a file" % args.input)
    if os.path.abspath(args.input) == os.path.abspath(args.output):
        p.error("OUT.bam must not be IN.bam")
    census = {} if read_filter.given(args) else None
    seen, kept, indexed = subsample_bam(args.input, args.output, rule, read_filter=flt, census=census)
    if flt is not None:
        print(read_filter.report_line(census, flt))
    if args.read_stats:
        print(read_filter.census_text(census))
    if rule is not None:
        print(subsample.report_line(seen, kept, rule))
    if not indexed:
        print("%s is not coordinate-sorted: no %s.bai written" % (args.input, args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
