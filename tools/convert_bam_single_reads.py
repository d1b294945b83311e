#!/usr/bin/env python3
"""CLI twin of the reference's ``tools/convert_bam_single_reads.py``: BAM + FASTA + candidate
VCF(s) -> ``candidates.hdf`` in the record layout main.py reads.  Same flags as the reference for the path call_variants.sh
(:87-98) and the training-data recipe (docs/Data.md) take:

    python tools/convert_bam_single_reads.py --input X.bam --fasta-input ref.fa --fp_vcf OUT/candidates.vcf \
        --output OUT/candidates.hdf --max-reads 200 --num-processes 16 --locations-process-step 100000 \
        --max-insert-length 10 --max-insert-length-variant 50 --save-q-scores --save-strand

(``--tp_vcf`` / ``--tp_full_vcf`` / ``--fn_vcf`` label locations 0 / 1 as the reference does.)  Options of the reference that
this path never used are refused, not ignored.  BAM / BAI / FASTA are read by dl4vc_amd/bamio.py (no htslib needed); records
are written in input order; ``--num-processes`` worker processes each take contiguous runs of locations.
``--pileup-device gpu`` builds the records' planes on the GPU; ``--compress-device gpu`` (with it) also packs and compresses the
file's chunks there and writes them past the HDF5 filter: the same records, in chunks another encoder compressed;
``--compress-codes dynamic`` (with it) gives those chunks dynamic Huffman codes where they are smaller than the fixed ones.
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                             # noqa: E402

from dl4vc_amd import hdf5io                                   # noqa: E402
from dl4vc_amd.pileup_encoder import EncoderOptions, encode_locations, locations_from_vcf      # noqa: E402


def _work(task):
    bam, fasta, locs, opt = task
    return encode_locations(bam, fasta, locs, opt)


def _convert_compressed(args, locations, opt, start, step, procs, append):
    """The loop of ``main`` with ``--compress-device gpu``: every batch's whole chunks arrive compressed and go to the file with
    ``H5Dwrite_chunk``; ``hdf5io.ChunkWriter`` carries the records between them, across batches and process steps."""
    import json
    from dl4vc_amd.hdf5_schema import record_dtype
    n_loc = len(locations)
    dtype = record_dtype(opt.max_reads, 2 * opt.window_size + 1)
    total_errors = written = 0
    census = {}
    stages = {k: 0.0 for k in ("pack_ms", "deflate_ms", "gather_ms", "compress_copy_back_ms", "raw_bytes", "chunk_bytes_out", "stored_chunks",
                                "fixed_segments", "dynamic_segments", "stored_segments")}
    t0 = time.time()
    try:
        writer = hdf5io.ChunkWriter(args.output, dtype, chunk=8, append=append, codes=args.compress_codes)
    except ValueError as e:
        raise SystemExit("--compress-device gpu: %s" % e)
    with writer:
        while start < n_loc:
            for b in encode_locations(args.input, args.fasta_input, locations[start:start + step], opt, threads=procs, device="gpu",
                                      inflate_device=args.inflate_device, compress_device="gpu", pending=len(writer.pending),
                                      compress_codes=args.compress_codes):
                writer.append_records(b.head)
                if b.chunks is not None:
                    writer.write_chunks(b.chunks)
                    for k in stages:
                        stages[k] += b.stats[k]
                for k, v in b.stats.items():
                    if k.startswith("read_"):
                        census[k] = census.get(k, 0) + v
                writer.append_records(b.tail)
                total_errors += b.errors
                written += b.records
            start += step
            print("Total errors %d through %d steps (%d records, %.1f s)" % (total_errors, min(start, n_loc), written, time.time() - t0), flush=True)
    stages.update(chunk_write_ms=round(writer.write_s * 1e3, 3), chunks_from_device=writer.direct_chunks, chunks_from_host=writer.host_chunks,
                  chunks_unfiltered=writer.stored_chunks, records=written)
    print("compress-device gpu stages: %s" % json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in stages.items()}))
    report_reads(opt, census)
    print("Parsing errors in %d / %d locations -- saved to: %s" % (total_errors, n_loc, args.output))
    return 0


def report_reads(opt, census) -> None:
    """The read filter's line and, with --read-stats, the census: the counts of the encoder that framed the reads (the GPU
    encoder's with --pileup-device gpu, else pe_encode's; the Python builder keeps none)."""
    from dl4vc_amd import read_filter
    if not census:
        return
    if opt.read_filter is not None:
        print(read_filter.report_line(census, opt.read_filter))
    if opt.read_stats:
        print(read_filter.census_text(census))


def main(argv=None):
    ap = argparse.ArgumentParser(description="BAM file to candidate records for single reads")
    ap.add_argument("--input", type=str, required=True, help="input BAM (coordinate-sorted; a .bai beside it is used when present)")
    ap.add_argument("--chrom", type=str, default="22")
    ap.add_argument("--locations", type=str, default=None)
    ap.add_argument("--tp_vcf", type=str, default=None)
    ap.add_argument("--tp_full_vcf", type=str, default=None)
    ap.add_argument("--fp_vcf", type=str, default=None)
    ap.add_argument("--fn_vcf", type=str, default=None)
    ap.add_argument("--restrict_locations_file", type=str, default="")
    ap.add_argument("--restrict_locations", action="store_true", default=False)
    ap.add_argument("--non_restrict_match_random", action="store_true", default=False)
    ap.add_argument("--output", type=str, default="result")
    ap.add_argument("--locations-process-step", type=int, default=100000)
    ap.add_argument("--locations-restart-pos", type=int, default=0)
    ap.add_argument("--locations-append-data", action="store_true", default=False)
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("--min-base-quality", type=int, default=0)
    ap.add_argument("--fasta-input", type=str, default="hs37d5.fa")
    ap.add_argument("--num-processes", type=int, default=10)
    ap.add_argument("--max-loc", type=int, default=0)
    ap.add_argument("--max-reads", type=int, default=1000)
    ap.add_argument("--window-size", type=int, default=100)
    ap.add_argument("--max-insert-length", type=int, default=10)
    ap.add_argument("--max-insert-length-variant", type=int, default=50)
    ap.add_argument("--save-q-scores", action="store_true")
    ap.add_argument("--save-strand", action="store_true")
    ap.add_argument("--pileup-device", type=str, default=None, choices=["gpu"],
                    help="gpu: build the image planes with the GPU pileup encoder (libdl4vc_pileup.so); what it declines goes to the "
                         "host encoders, so the file is the same bytes (default: the host encoders)")
    ap.add_argument("--inflate-device", type=str, default=None, choices=["gpu"],
                    help="gpu: with --pileup-device gpu, the GPU encoder inflates the BAM's BGZF blocks and frames its records on the "
                         "device as well (needs the .bai); the file is the same bytes")
    ap.add_argument("--compress-device", type=str, default=None, choices=["gpu"],
                    help="gpu: with --pileup-device gpu, the records are packed and compressed into the file's chunks on the device "
                         "and written past the HDF5 filter; the same records in a file any HDF5 reader inflates (other bytes: "
                         "another encoder)")
    ap.add_argument("--compress-codes", type=str, default="fixed", choices=["fixed", "dynamic"],
                    help="with --compress-device gpu: dynamic gives a chunk's segments dynamic Huffman codes where that is smaller "
                         "(a smaller file, the same records; the compressor parses every segment twice); default fixed")
    from dl4vc_amd import subsample
    from dl4vc_amd import read_filter
    subsample.add_flags(ap)
    read_filter.add_flags(ap)
    args = ap.parse_args(argv)
    rule = subsample.parse(ap, args)
    flt = read_filter.parse(ap, args)
    if args.inflate_device and args.pileup_device != "gpu":
        raise SystemExit("--inflate-device gpu is an option of the GPU pileup encoder: give --pileup-device gpu as well")
    if args.compress_device and args.pileup_device != "gpu":
        raise SystemExit("--compress-device gpu compresses the GPU pileup encoder's planes where they lie, in device memory: "
                         "give --pileup-device gpu as well")
    if args.compress_codes != "fixed" and args.compress_device != "gpu":
        raise SystemExit("--compress-codes %s chooses the codes of the device compressor: give --compress-device gpu as well "
                         "(without it the file's chunks are libhdf5's gzip)" % args.compress_codes)
    for flag, why in (("locations", "numpy location tables"), ("restrict_locations", "location restriction files"),
                      ("non_restrict_match_random", "location restriction files")):
        if getattr(args, flag):
            raise SystemExit("--%s (%s) is not supported by this converter" % (flag, why))
    # convert_bam_single_reads.py:700-701: the record layout always holds both planes
    assert args.save_q_scores, "Too many options, need to run with Q scores"
    assert args.save_strand, "Too many options, need to run with strand save"
    opt = EncoderOptions(window_size=args.window_size, max_reads=args.max_reads, max_insert_length=args.max_insert_length,
                         max_insert_length_variant=args.max_insert_length_variant, min_base_quality=args.min_base_quality,
                         subsample=rule, read_filter=flt, read_stats=args.read_stats)
    if rule is not None:
        # (the host encoders keep no count of the records they drop: tools/subsample_bam.py and the candidate generator print them)
        print("subsample: every encoder keeps the reads of fraction %g, seed %d" % rule)
    locations = []
    if args.tp_vcf:
        locations.extend(locations_from_vcf(args.tp_vcf, label=0, full_vcf=args.tp_full_vcf))
    if args.fn_vcf:
        locations.extend(locations_from_vcf(args.fn_vcf, label=1))
    if args.fp_vcf:
        locations.extend(locations_from_vcf(args.fp_vcf, label=2))
    print("After adding from VCF, %d total locations considered" % len(locations))
    if args.max_loc > 0:
        locations = locations[:args.max_loc]
    n_loc = len(locations)
    start = args.locations_restart_pos
    append = start > 0 or args.locations_append_data
    if append:
        assert os.path.isfile(args.output), "Output file must exist for append mode."
    step = args.locations_process_step
    procs = max(1, args.num_processes)
    print("Processing %d locations with %d process" % (n_loc, procs))
    print("Splitting locations into ~%d chunks [%d each] to save memory..." % (math.ceil(max(n_loc - start, 0) / step), step))
    pool = None
    from dl4vc_amd import loader
    native = loader.available() and not os.environ.get("DL4VC_PILEUP_PYTHON")
    if args.pileup_device == "gpu":
        print("GPU pileup encoder; %d thread(s) for what it declines" % procs)
    elif native:
        # the native encoder (libdl4vc_loader.so, pe_*): --num-processes becomes worker THREADS over contiguous runs of locations
        print("native pileup encoder: %d thread(s)" % procs)
    if not native and args.pileup_device is None and procs > 1 and n_loc - start > 4 * procs:
        import multiprocessing as mp
        pool = mp.get_context("spawn").Pool(procs)
    total_errors, written, created = 0, 0, append
    census = {}                                               # the read census of the encode calls (with a filter or --read-stats)
    t0 = time.time()
    if args.compress_device == "gpu":
        return _convert_compressed(args, locations, opt, start, step, procs, append)
    try:
        while start < n_loc or not created:
            chunk = locations[start:start + step]
            if pool is not None and len(chunk) > 4 * procs:
                per = max(8, math.ceil(len(chunk) / (4 * procs)))
                tasks = [(args.input, args.fasta_input, chunk[i:i + per], opt) for i in range(0, len(chunk), per)]
                parts = pool.map(_work, tasks)
                recs = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0)
                errors = sum(p[1] for p in parts)
            else:
                recs, errors = encode_locations(args.input, args.fasta_input, chunk, opt, native=native, threads=procs,
                                                device=args.pileup_device, inflate_device=args.inflate_device, read_stats=census)
            total_errors += errors
            if not created:
                hdf5io.write_candidates(args.output, recs, chunk=8)
                created = True
            elif len(recs):
                hdf5io.append_candidates(args.output, recs)
            written += len(recs)
            start += step
            print("Total errors %d through %d steps (%d records, %.1f s)" % (total_errors, min(start, n_loc), written, time.time() - t0), flush=True)
    finally:
        if pool is not None:
            pool.terminate()
            pool.join()
    report_reads(opt, census)
    print("Parsing errors in %d / %d locations -- saved to: %s" % (total_errors, n_loc, args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
