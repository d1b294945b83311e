#!/usr/bin/env python
"""Rate of the GPU pileup encoder (``pg_encode_device``) with the BAM inflated and framed on the host (the default) against the
device (``inflate_device="gpu"``), on two seeded synthetic BAMs:
  dense         the 200-kbp, ~30x BAM of tools/score_bam_rate.py with a location every 10 bases (19 940 locations);
  whole_genome  the 2 M-read, 10-Mb BAM of tools/candgen_rate.py with a location every 500 bases: short runs, more inflated
                bytes per location.
Calls of 4 096 locations, window 100, 200 stored rows.  Every measurement is a fresh child process (option off, then on, three
rounds), each under its own time limit; a child that fails ends the tool, nothing is started after it.  A child warms up on
1 000 locations and reports the best of three passes over all locations: locations/s and every ``pg_stats`` field summed over
the pass.  One JSON record; no number in it is a pass mark.

    python tools/pileup_inflate_rate.py --dir /tmp/pir [--rounds 3] [--wg-reads 2000000 --wg-length 10000000] [--out profiles/x.json]
        [--kernel-trace] [--score-bam] [--subsample F [--subsample-seed S]] [--min-mapq Q] [--exclude-flags F] [--require-flags F]
        [--read-stats]

``--kernel-trace``: afterwards, for both shapes and both settings, one more child (one pass) under ``rocprofv3 --kernel-trace
--stats``; the record gains the total time per kernel, warm-up included.  ``--score-bam``: afterwards, one round each of
``tools/score_bam_rate.py`` on the dense BAM at fp32 and bf16x3, without and with ``--inflate-device gpu``; the record gains the
scoring-loop rates.  Every one of these is again one process at a time under its own time limit, and a failure ends the tool.
``--subsample F [--subsample-seed S]`` is passed through to every child's encoder (reads subsampled by name hash where the
framing runs); the summed stats then carry ``subsample_records_seen`` / ``subsample_records_kept``.  The read filter flags are
passed through likewise; the stats then carry the census totals (``read_seen`` ...).
"""
import argparse
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CALL = 4096


def child(a):
    import torch
    from dl4vc_amd import pileup_gpu
    pos = [a.first + a.step * i for i in range(a.count)]
    contigs = [a.contig] * len(pos)
    dev = torch.device("cuda", 0)
    out = [torch.empty((CALL, 200, 201), dtype=torch.uint8, device=dev) for _ in range(3)]
    extra = {"subsample": (a.subsample, a.subsample_seed or 0)} if a.subsample is not None else {}
    if a.read_filter is not None or a.read_stats:
        extra.update(read_filter=a.read_filter, read_stats=a.read_stats)
    with pileup_gpu.GpuPileupEncoder(a.bam, a.fasta, 100, 200, 10, 50, inflate_device=a.inflate_device, **extra) as g:
        g.encode_device(contigs[:1000], pos[:1000], out=out)
        torch.cuda.synchronize()
        best = None
        for _ in range(a.repeats):
            total, status = {}, np.zeros(3, np.int64)
            t0 = time.perf_counter()
            for i in range(0, len(pos), CALL):
                r = g.encode_device(contigs[i:i + CALL], pos[i:i + CALL], out=out)
                for k, v in g.stats().items():
                    total[k] = total.get(k, 0) + v
                status += np.bincount(r[5], minlength=3)[:3]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if best is None or dt < best["seconds"]:
                best = {"seconds": round(dt, 4), "locations_per_s": round(len(pos) / dt), "status_0_1_2": status.tolist(),
                        "stats": {k: (round(v, 2) if isinstance(v, float) else int(v)) for k, v in total.items()}}
    if a.read_filter is not None:
        from dl4vc_amd import read_filter
        print(read_filter.report_line(best["stats"], a.read_filter), file=sys.stderr)
    print("RESULT " + json.dumps(best))
    return 0


def make_whole_genome(d, n_reads, length):
    from candgen_rate import make_bam
    bam, fa = os.path.join(d, "wg.bam"), os.path.join(d, "wg.fa")
    if not all(os.path.isfile(p) for p in (bam, bam + ".bai", fa)):
        make_bam(bam, n_reads, length, seed=1)
        ref = np.random.default_rng(1).choice(np.frombuffer(b"ACGT", np.uint8), length).tobytes().decode()   # (make_bam's first draw)
        with open(fa, "w") as f:
            f.write(">chr1\n" + "\n".join(ref[i:i + 60] for i in range(0, length, 60)) + "\n")
    return bam, fa


def kernel_trace(d, tag, child_cmd, timeout):
    """One child under rocprofv3 -> {kernel: {calls, total_ms}}, from the top_kernels view of its results database."""
    out = os.path.join(d, "trace_" + tag)
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "p", "--"] + child_cmd, capture_output=True, text=True,
                       timeout=timeout)
    db = glob.glob(os.path.join(out, "**", "*results.db"), recursive=True)
    if p.returncode != 0 or not db:
        sys.exit("kernel trace %s failed with %d: nothing more is started\n%s" % (tag, p.returncode, p.stderr[-1500:]))
    ks = {}
    for name, calls, total_us in sqlite3.connect(db[0]).execute("select name, total_calls, total_duration from top_kernels"):
        m = re.search(r"(pileup_\w+_kernel|bgzf_\w+_kernel|bam_\w+_kernel|resolve_records|encode_locations|__amd_rocclr_\w+)", name)
        e = ks.setdefault(m.group(1) if m else "rocprim scans and radix sort", {"calls": 0, "total_ms": 0.0})
        e["calls"] += calls
        e["total_ms"] = round(e["total_ms"] + total_us / 1e3, 3)      # (the view's durations are microseconds)
    return dict(sorted(ks.items(), key=lambda kv: -kv[1]["total_ms"]))


def score_bam(d, precision, inflate, timeout):
    out = os.path.join(d, "sbr_%s_%s.json" % (precision, "on" if inflate else "off"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "score_bam_rate.py"), "--dir", d, "--rounds", "1", "--precision", precision,
                        "--no-bench", "--out", out] + (["--inflate-device", "gpu"] if inflate else []), capture_output=True, text=True, timeout=timeout)
    if p.returncode not in (0, 1) or not os.path.isfile(out):      # (1: its own verdict on the two-step comparison, not a failure)
        sys.exit("score_bam_rate %s failed with %d: nothing more is started\n%s" % (precision, p.returncode, p.stderr[-1500:]))
    r = json.load(open(out))
    return {k: r[k] for k in ("i_test_bam_sites_per_s_scoring_loop", "i_test_bam_wall_s", "iii_forward_sites_per_s_test_file_loop", "ratio_i_to_iii",
                              "same_scored_vcf")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", help="working directory (inputs are made there once and reused)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dense-length", type=int, default=200000)
    ap.add_argument("--wg-reads", type=int, default=2000000)
    ap.add_argument("--wg-length", type=int, default=10000000)
    ap.add_argument("--timeout", type=int, default=300, help="seconds, per child")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", action="store_true")
    ap.add_argument("--score-bam", action="store_true")
    ap.add_argument("--child", action="store_true")
    for name in ("--bam", "--fasta", "--contig"):
        ap.add_argument(name)
    for name, default in (("--first", 300), ("--step", 10), ("--count", 0), ("--repeats", 3)):
        ap.add_argument(name, type=int, default=default)
    ap.add_argument("--inflate-device", default=None, choices=["gpu"])
    from dl4vc_amd import subsample
    from dl4vc_amd import read_filter
    subsample.add_flags(ap)
    read_filter.add_flags(ap)
    a = ap.parse_args()
    rule = subsample.parse(ap, a)
    a.read_filter = read_filter.parse(ap, a)
    sub_flags = ["--subsample", repr(rule[0]), "--subsample-seed", str(rule[1])] if rule is not None else []
    sub_flags += read_filter.cli_flags(a.read_filter, a.read_stats)
    if a.child:
        return child(a)
    if not a.dir:
        ap.error("--dir is required")
    os.makedirs(a.dir, exist_ok=True)
    from score_bam_rate import make_inputs
    dense_bam, dense_fa, _vcf, n_dense = make_inputs(a.dir, a.dense_length)
    wg_bam, wg_fa = make_whole_genome(a.dir, a.wg_reads, a.wg_length)
    shapes = [("dense", dense_bam, dense_fa, "chr20", 300, 10, n_dense),
              ("whole_genome", wg_bam, wg_fa, "chr1", 500, 500, (a.wg_length - 1000) // 500)]
    res = {"tool": "pileup_inflate_rate", "call_locations": CALL, "window_size": 100, "max_reads": 200, "dense_length": a.dense_length,
           "wg_reads": a.wg_reads, "wg_length": a.wg_length, "subsample": list(rule) if rule is not None else None,
           "read_filter": list(a.read_filter) if a.read_filter is not None else None, "shapes": {}}
    for name, bam, fa, contig, first, step, count in shapes:
        rounds = []
        for k in range(a.rounds):
            r = {}
            for tag, extra in (("off", []), ("on", ["--inflate-device", "gpu"])):      # one child at a time holds the GPU
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--bam", bam, "--fasta", fa, "--contig", contig, "--first", str(first),
                       "--step", str(step), "--count", str(count)] + extra + sub_flags
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
                if p.returncode != 0 or not line:
                    sys.exit("%s round %d (%s) failed with %d: nothing more is started\n%s\n%s" % (name, k, tag, p.returncode, p.stdout[-1500:], p.stderr[-1500:]))
                r[tag] = json.loads(line[0][7:])
            r["on_over_off"] = round(r["on"]["locations_per_s"] / max(1, r["off"]["locations_per_s"]), 3)
            rounds.append(r)
            print("%s round %d: off %d, on %d locations/s" % (name, k, r["off"]["locations_per_s"], r["on"]["locations_per_s"]), file=sys.stderr, flush=True)
        res["shapes"][name] = {"locations": count, "bam_mb": round(os.path.getsize(bam) / 1e6, 1), "rounds": rounds,
                               "on_faster_in_every_round": all(r["on_over_off"] > 1 for r in rounds)}
    if a.kernel_trace:
        res["kernel_trace"] = {"what": "one child per shape and setting under rocprofv3 --kernel-trace --stats: the 1 000-location warm-up plus "
                                       "one pass; total ms per kernel"}
        for name, bam, fa, contig, first, step, count in shapes:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--bam", bam, "--fasta", fa, "--contig", contig, "--first", str(first),
                   "--step", str(step), "--count", str(count), "--repeats", "1"]
            res["kernel_trace"][name] = {"off": kernel_trace(a.dir, name + "_off", cmd, a.timeout),
                                         "on": kernel_trace(a.dir, name + "_on", cmd + ["--inflate-device", "gpu"], a.timeout)}
    if a.score_bam:
        res["score_bam_rate_one_round_each"] = {"%s_%s" % (prec, "on" if on else "off"): score_bam(a.dir, prec, on, 2 * a.timeout)
                                                for prec in ("fp32", "bf16x3") for on in (False, True)}
    text = json.dumps(res)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
