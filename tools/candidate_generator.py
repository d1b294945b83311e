#!/usr/bin/env python
"""BAM -> candidates.vcf: the first stage of call_variants.sh, with the reference tool's flags, types and defaults
(reference tools/candidate_generator.py).  The per-read work and the per-locus counts run on the GPU
(libdl4vc_cand.so); see dl4vc_amd/candidates.py for the host logic and DESIGN.md section 9 for the divergences.

    candidate_generator.py --input in.bam --output out.vcf --contigs 20:1000:2000,17:0:50000,8
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
from argparse import RawTextHelpFormatter

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser() -> argparse.ArgumentParser:
    from dl4vc_amd.candgen import default_threads
    p = argparse.ArgumentParser(description="Generate a VCF from a BAM file with candidate variants.\n\n"
                                "Example usage:\n    candidate_generator.py --input in.bam --output out.vcf --contigs "
                                "20:1000:2000,17:0:50000", formatter_class=RawTextHelpFormatter)
    p.add_argument("--input", help="input BAM file (indexed by INPUT.bai when that file exists)")
    p.add_argument("--output", default="out.vcf", help="output VCF file")
    p.add_argument("--contigs", default=None, help="Comma delimited list of contigs to use in format contig:start:end")
    p.add_argument("--keep_contig_chr", action="store_true", default=False,
                   help='Set true if BAM file lists contigs as "chrC" instead of "X"')
    p.add_argument("--chunk_size", default=1000, type=int,
                   help="Size of region for each process to calculate variants on, in kb (kilobases)")
    p.add_argument("--threads", default=None, type=int,
                   help="Host threads that inflate and frame records. Defaults to min(16, usable cores) = %d here"
                   % default_threads())
    p.add_argument("--snp_min_freq", default=0.01, type=float,
                   help="The minimum fraction of SNP alleles at a locus to be included as a candidate")
    p.add_argument("--indel_min_freq", default=0.01, type=float,
                   help="The minimum fraction of indel alleles at a locus to be included as a candidate")
    p.add_argument("--keep_multialleles", action="store_true", default=False,
                   help="Do not remove multiple alleles for same genomic location")
    p.add_argument("--max_len_indel_allele", default=60, type=int, help="In case of bad mapping, ignore long alleles.")
    p.add_argument("--bedfile", default=None, help="BED file with intervals to use for candidate generation")
    p.add_argument("--debug", action="store_true", help="Print debug information")
    return p


def warn_no_md(stats, reference) -> None:
    """One line in the log (never in the VCF) when most reads gave no alleles for want of an MD tag."""
    if reference is None and 2 * stats.get("reads_no_md", 0) > stats.get("reads", 0):
        logging.warning("%d of %d reads have no MD tag and gave no alleles: give --reference REF.fa to walk them against the "
                        "reference bases", stats["reads_no_md"], stats["reads"])


def report_left_align(args, stats) -> None:
    if args.left_align:
        print("left-align: %d indel observations, %d shifted by %d bases in all, %d clamped by their read's start, %d not eligible"
              % tuple(stats.get("left_align_" + k, 0) for k in ("observations", "shifted", "bases_shifted", "clamped", "not_eligible")))


def report_reads(args, stats) -> None:
    """The read filter's line and, with --read-stats, the census."""
    from dl4vc_amd import read_filter
    flt = read_filter.check(args, sys.exit)
    if flt is not None:
        print(read_filter.report_line(stats, flt))
    if args.read_stats:
        print(read_filter.census_text(stats))


def run_children(args, argv) -> int:
    """--gpus N: a fresh process per GPU (``--shard g/N``, its own HIP_VISIBLE_DEVICES), then the merge of their parts."""
    import subprocess
    from dl4vc_amd.candidates import merge_parts, remove_parts
    from dl4vc_amd.procs import child_devices, child_env, wait_children
    devices = child_devices(args.gpus)
    remove_parts(args.output, args.gpus)                      # (nothing of an earlier run is merged)
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv + ["--shard", "%d/%d" % (g, args.gpus)],
                              env=child_env(devices[g])) for g in range(args.gpus)]
    rcs = wait_children(procs)
    if any(rcs):
        remove_parts(args.output, args.gpus)
        raise SystemExit("shard process failed: %s" % rcs)
    stats = merge_parts(args.output, args.gpus)
    warn_no_md(stats, args.reference)
    if args.subsample is not None:
        from dl4vc_amd import subsample
        print(subsample.report_line(stats["subsample_records_seen"], stats["subsample_records_kept"],
                                    (args.subsample, args.subsample_seed or 0)))
    report_reads(args, stats)                                 # (the census of the parts, summed)
    report_left_align(args, stats)
    logging.info("Generated final VCF file at %s from %d parts.", args.output, args.gpus)
    print("summary " + json.dumps(stats, sort_keys=True))
    return 0


def main(argv=None) -> int:
    p = build_parser()
    # (added here, after build_parser(): its table of flags stays the reference tool's)
    p.add_argument("--inflate-device", dest="inflate_device", choices=["gpu"], default=None,
                   help="Inflate the BAM's BGZF blocks and frame its records on the GPU instead of in host threads (needs INPUT.bai)")
    p.add_argument("--gpus", type=int, default=1,
                   help="One process per GPU: the groups of subregions are dealt to them in contiguous ranges, each writes its "
                   "unsorted records to OUTPUT.part<g>, and this process sorts them into OUTPUT (the same bytes as with 1)")
    p.add_argument("--shard", default="", help="g/N: count only the g-th of N ranges of groups into OUTPUT.part<g> (--gpus sets this)")
    p.add_argument("--reference", default=None, metavar="REF.fa",
                   help="Walk the reads that have no MD tag against this FASTA's bases (REF.fa.fai when that file exists) instead "
                   "of giving them no alleles; reads with an MD tag are walked by it as before. Each contig touched stays on the GPU "
                   "as 1 byte per base")
    p.add_argument("--left-align", dest="left_align", action="store_true", default=False,
                   help="Move every insertion and deletion to its left-most placement on the reference bases before it is counted, "
                   "so that the placements of one event inside a repeat give one candidate (needs --reference; with it, reads "
                   "without an MD tag are walked against the FASTA too)")
    from dl4vc_amd import subsample
    from dl4vc_amd import read_filter
    subsample.add_flags(p)
    read_filter.add_flags(p)
    args = p.parse_args(argv)
    rule = subsample.parse(p, args)                           # (before any device work, --gpus children included)
    flt = read_filter.parse(p, args)
    print(args)
    logging.basicConfig(format="%(levelname)s: %(message)s", level=logging.DEBUG if args.debug else logging.INFO)
    if args.left_align and args.reference is None:
        p.error("--left-align needs --reference REF.fa: left-alignment is defined by the reference bases")
    if args.reference is not None and not (os.path.isfile(args.reference) and os.access(args.reference, os.R_OK)):
        p.error("--reference %s is not a readable file" % args.reference)      # (before any device work, --gpus children included)
    from dl4vc_amd.candidates import generate
    from dl4vc_amd.shard import parse_shard
    if args.gpus < 1:
        p.error("--gpus must be at least 1")
    try:
        shard = parse_shard(args.shard) if args.shard else None
    except ValueError as e:
        p.error(str(e))
    if args.gpus > 1 and shard is None:
        return run_children(args, list(sys.argv[1:] if argv is None else argv))
    stats = generate(args.input, args.output, contigs=args.contigs, bedfile=args.bedfile, keep_contig_chr=args.keep_contig_chr,
                     chunk_size=args.chunk_size, threads=args.threads, snp_min_freq=args.snp_min_freq,
                     indel_min_freq=args.indel_min_freq, keep_multialleles=args.keep_multialleles,
                     max_len_indel_allele=args.max_len_indel_allele, inflate_device=args.inflate_device, shard=shard,
                     reference=args.reference, subsample=rule, read_filter=flt, read_stats=args.read_stats,
                     left_align=args.left_align)
    if shard is None:                      # (the parent of shards says it once, of the summed counts)
        warn_no_md(stats, args.reference)
        if rule is not None:
            print(subsample.report_line(stats["subsample_records_seen"], stats["subsample_records_kept"], rule))
        report_reads(args, stats)
        report_left_align(args, stats)
    if shard is not None:
        from dl4vc_amd.shard import part_path
        logging.info("Wrote the records of shard %d/%d to %s.", shard[0], shard[1], part_path(args.output, shard[0]))
    else:
        logging.info("Generated final VCF file at %s.", args.output)
    print("summary " + json.dumps(stats, sort_keys=True))
    return 0


if __name__ == "__main__":
    sys.exit(main())
