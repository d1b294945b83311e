#!/usr/bin/env python
"""Candidate generation rate on a seeded synthetic BAM (about 30x over 10 Mb: 2 M reads of 150 bases with MD tags, SNPs at
seeded sites plus 0.2 % sequencing errors, an indel in 5 % of reads).  Prints one JSON line: reads/s end to end, and the
host's inflate-and-frame time against the device time (per-stage device times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this tool).

    python tools/candgen_rate.py --bam /tmp/cg_rate.bam [--reads 2000000 --length 10000000] [--out profiles/x.json]
        [--inflate-device gpu] [--chunk_size 1000] [--no-md] [--fasta REF.fa] [--reference REF.fa]
        [--left-align] [--subsample F [--subsample-seed S]] [--min-mapq Q] [--exclude-flags F] [--require-flags F] [--read-stats]

``--inflate-device gpu`` measures the device inflate path (the line then carries its read / inflate / walk-and-frame times);
``--chunk_size`` other than 1000 changes the subregions, and with them the candidates at their boundaries: a timing line only.

The reference arm: ``--no-md`` writes the same reads without aux tags (when ``--bam`` has to be made), ``--fasta`` writes the
genome they were drawn from beside it (60 bases a line, with its ``.fai``), and ``--reference REF.fa`` walks the reads that have
no MD tag against it; the line then carries the ``reference_*`` figures.  Every repeat opens its own handle, so the contig's
one-time load (read, upload and convert) is inside every repeat's wall time.

``--left-align`` (with ``--reference``) left-aligns the indels before they are counted; the line then carries the
``left_align_*`` counters.

``--subsample F [--subsample-seed S]`` is passed through (reads subsampled by name hash in front of every count); the line then
carries the records seen and kept, and ``reads_per_s`` counts the records SEEN, the work the framing did.  The read filter
flags are passed through likewise; the line then carries the census totals, and ``reads_per_s`` counts the records the census saw.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dl4vc_amd.bamio import BamWriter, build_bai, CMATCH, CINS, CDEL   # noqa: E402


def make_bam(path, n_reads, length, seed=1, md_tags=True, fasta=None):
    rng = np.random.default_rng(seed)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), length)
    sites = np.zeros(length, bool)
    sites[rng.choice(length, length // 1000, replace=False)] = True
    starts = np.sort(rng.integers(0, length - 200, n_reads))
    if fasta:
        with open(fasta, "wb") as f:
            f.write(b">chr1\n")
            at = f.tell()
            f.write(b"\n".join(ref[i:i + 60].tobytes() for i in range(0, length, 60)) + b"\n")
        open(fasta + ".fai", "w").write("chr1\t%d\t%d\t60\t61\n" % (length, at))
    L = 150
    with BamWriter(path, [("chr1", length)], level=1) as w:
        for i, s in enumerate(starts.tolist()):
            seq = ref[s:s + L].copy()
            mut = (sites[s:s + L] & (rng.random(L) < 0.5)) | (rng.random(L) < 0.002)
            idx = np.nonzero(mut)[0]
            for k in idx:
                seq[k] = b"ACGT"[(b"ACGT".index(bytes([seq[k]])) + 1) % 4]
            cigar = [(CMATCH, L)]
            md_parts, run = [], 0
            r = ref[s:s + L]
            for k in range(L):
                if seq[k] != r[k]:
                    md_parts.append("%d%s" % (run, chr(r[k])))
                    run = 0
                else:
                    run += 1
            md = "".join(md_parts) + str(run)
            sq = seq.tobytes().decode()
            if i % 20 == 0:                     # a 2-base deletion or insertion at base 70
                if i % 40 == 0:
                    cigar = [(CMATCH, 70), (CDEL, 2), (CMATCH, 80)]
                    sq = ref[s:s + 70].tobytes().decode() + ref[s + 72:s + 152].tobytes().decode()
                    md = "70^%s80" % ref[s + 70:s + 72].tobytes().decode()
                else:
                    cigar = [(CMATCH, 70), (CINS, 2), (CMATCH, 78)]
                    sq = ref[s:s + 70].tobytes().decode() + "GT" + ref[s + 70:s + 148].tobytes().decode()
                    md = "148"
            w.write(0, s, "r%d" % i, 16 if i & 1 else 0, 60, cigar, sq, aux=b"MDZ" + md.encode() + b"\x00" if md_tags else b"")
    build_bai(path, path + ".bai")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bam", required=True)
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--length", type=int, default=10000000)
    ap.add_argument("--threads", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--inflate-device", dest="inflate_device", choices=["gpu"], default=None)
    ap.add_argument("--chunk_size", type=int, default=1000)
    ap.add_argument("--no-md", dest="no_md", action="store_true", help="write the BAM without aux tags (when it has to be made)")
    ap.add_argument("--fasta", default=None, help="write the BAM's genome here, with its .fai (when the BAM has to be made)")
    ap.add_argument("--reference", default=None, help="walk the reads that have no MD tag against this FASTA")
    ap.add_argument("--left-align", dest="left_align", action="store_true", help="left-align the indels on --reference before counting")
    from dl4vc_amd import subsample
    from dl4vc_amd import read_filter
    subsample.add_flags(ap)
    read_filter.add_flags(ap)
    a = ap.parse_args()
    rule = subsample.parse(ap, a)
    flt = read_filter.parse(ap, a)
    if a.left_align and not a.reference:
        ap.error("--left-align needs --reference REF.fa")
    if not os.path.isfile(a.bam + ".bai"):
        t = time.time()
        make_bam(a.bam, a.reads, a.length, md_tags=not a.no_md, fasta=a.fasta)
        print("wrote %s in %.1f s" % (a.bam, time.time() - t), file=sys.stderr)
    from dl4vc_amd.candidates import generate
    extra = {"subsample": rule} if rule is not None else {}
    if flt is not None or a.read_stats:
        extra.update(read_filter=flt, read_stats=a.read_stats)
    if a.left_align:
        extra.update(left_align=True)
    runs = []
    for k in range(a.repeats):
        t = time.perf_counter()
        st = generate(a.bam, a.bam + ".vcf", threads=a.threads, snp_min_freq=0.075, indel_min_freq=0.02, keep_multialleles=True,
                      chunk_size=a.chunk_size, inflate_device=a.inflate_device, reference=a.reference, **extra)
        st["wall_s"] = time.perf_counter() - t
        runs.append(st)
    best = min(runs, key=lambda r: r["wall_s"])
    res = {"tool": "candgen_rate", "reads_fetched": best["reads"], "wall_s": [round(r["wall_s"], 3) for r in runs],
           "reads_per_s": round(best["reads"] / best["wall_s"]), "host_frame_ms": round(best["host_frame_ms"], 1),
           "upload_ms": round(best["upload_ms"], 1), "device_ms": round(best["device_ms"], 1),
           "native_total_ms": round(best["total_ms"], 1), "candidates": best["candidates"], "alleles": best["alleles"],
           "allele_events": best["allele_events"], "batches": best["batches"], "threads": a.threads or min(16, len(os.sched_getaffinity(0))),
           "chunk_size": a.chunk_size, "inflate_device": a.inflate_device, "reference": bool(a.reference),
           "reads_no_md": best["reads_no_md"], "left_align": bool(a.left_align)}
    for k in ("inflate_blocks", "inflate_compressed_bytes", "inflate_inflated_bytes", "inflate_records", "inflate_read_ms", "inflate_ms",
              "inflate_walk_frame_ms", "reference_reads", "reference_contigs", "reference_bases", "reference_other_bytes",
              "reference_read_ms", "reference_upload_convert_ms", "left_align_observations", "left_align_shifted",
              "left_align_bases_shifted", "left_align_clamped", "left_align_not_eligible"):
        if k in best:
            res[k] = round(best[k], 1) if isinstance(best[k], float) else best[k]
    if rule is not None:
        res.update(subsample=list(rule), subsample_records_seen=best["subsample_records_seen"],
                   subsample_records_kept=best["subsample_records_kept"],
                   reads_per_s=round(best["subsample_records_seen"] / best["wall_s"]))
    if flt is not None or a.read_stats:
        res.update(read_filter=list(flt) if flt is not None else None, reads_per_s=round(best["read_seen"] / best["wall_s"]),
                   **{k: best[k] for k in ("read_seen", "read_dropped_flags", "read_dropped_mapq", "read_kept")})
        if flt is not None:
            print(read_filter.report_line(best, flt), file=sys.stderr)
        if a.read_stats:
            print(read_filter.census_text(best), file=sys.stderr)
    if best.get("inflate_ms"):
        res["inflate_MB_per_s"] = round(best["inflate_inflated_bytes"] / 1e6 / (best["inflate_ms"] / 1e3))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
