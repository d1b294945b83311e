#!/usr/bin/env python
"""The converter with ``--compress-device gpu``, in fixed and in dynamic codes (``--compress-codes``), against the converter
without it (``--pileup-device gpu`` all three), on the seeded synthetic BAM of tools/score_bam_rate.py (by default 200 kbp at
~30x, 19 940 locations).

Alternating rounds (off fixed dynamic off fixed dynamic ...), each converter a fresh process as a user would start it, under its own ``timeout`` and
chained: the first step that fails or runs out of time ends the run.  Per round the wall clock of the whole process and the
locations per second; for the device arms the stages they print (pack, deflate, gather, copy back on the device clock; the chunk
writes on the host clock), the deflate kernel's input rate and the segments by kind; the size of each file against libhdf5's
gzip-4 file of the same records.  After the last round the three files are read back and compared record by record.  One JSON
record.

    python tools/convert_rate.py --dir /tmp/cr [--length 200000 --rounds 3 --threads 16 --step 100000] [--out profiles/convert_compress.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from score_bam_rate import make_inputs          # noqa: E402


def step(cmd, limit):
    """One link of the chain: the command under ``timeout``; -> (wall seconds, stdout), or ends the run."""
    t = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        sys.exit("%s ended with status %d after %.1f s; nothing more is started\n%s\n%s"
                 % (" ".join(cmd[1:3]), r.returncode, dt, r.stdout[-1500:], r.stderr[-1500:]))
    return dt, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="working directory (inputs are made there once and reused)")
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="--num-processes of the converter")
    ap.add_argument("--step", type=int, default=100000, help="--locations-process-step of the converter")
    ap.add_argument("--limit", type=int, default=240, help="seconds each converter process may take")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    bam, fa, vcf, n_loc = make_inputs(a.dir, a.length)
    files = {"off": os.path.join(a.dir, "gzip4.hdf"), "on": os.path.join(a.dir, "device.hdf"), "dyn": os.path.join(a.dir, "device_dynamic.hdf")}
    flags = {"off": [], "on": ["--compress-device", "gpu"], "dyn": ["--compress-device", "gpu", "--compress-codes", "dynamic"]}
    base = [sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa,
            "--max-reads", "200", "--num-processes", str(a.threads), "--locations-process-step", str(a.step), "--max-insert-length", "10",
            "--max-insert-length-variant", "50", "--save-q-scores", "--save-strand", "--pileup-device", "gpu"]
    rounds = []
    for k in range(a.rounds):
        r = {}
        for mode in ("off", "on", "dyn"):
            if os.path.isfile(files[mode]):
                os.remove(files[mode])
            wall, out = step(base + ["--output", files[mode]] + flags[mode], a.limit)
            r[mode + "_wall_s"] = round(wall, 3)
            r[mode + "_locations_per_s"] = round(n_loc / wall)
            r[mode + "_file_bytes"] = os.path.getsize(files[mode])
            loop = re.findall(r"\((\d+) records, ([0-9.]+) s\)", out)
            r[mode + "_convert_loop_s"] = float(loop[-1][1]) if loop else None
            if mode != "off":
                st = json.loads(re.search(r"compress-device gpu stages: (\{.*\})", out).group(1))
                st["deflate_input_gb_per_s"] = round(st["raw_bytes"] / 1e9 / (st["deflate_ms"] / 1e3), 2) if st["deflate_ms"] else None
                r[mode + "_stages"] = st
        rounds.append(r)
        print("round %d: %s" % (k, json.dumps(r)), file=sys.stderr, flush=True)
    # the same records in all three files
    from dl4vc_amd import hdf5io
    with hdf5io.CandidateFile(files["off"]) as f0, hdf5io.CandidateFile(files["on"]) as f1, hdf5io.CandidateFile(files["dyn"]) as f2:
        same = len(f0) == len(f1) == len(f2)
        for lo in range(0, len(f0), 1024):
            want = f0.read(lo, lo + 1024).tobytes()
            same = same and want == f1.read(lo, lo + 1024).tobytes() and want == f2.read(lo, lo + 1024).tobytes()
        records = len(f0)
    if not same:
        sys.exit("the three files hold different records")
    res = {"tool": "convert_rate", "locations": n_loc, "records": records, "threads": a.threads, "step": a.step, "rounds": rounds,
           "off_wall_s": [r["off_wall_s"] for r in rounds], "on_wall_s": [r["on_wall_s"] for r in rounds],
           "dyn_wall_s": [r["dyn_wall_s"] for r in rounds],
           "on_faster_in_every_round": all(r["on_wall_s"] < r["off_wall_s"] for r in rounds),
           "dyn_faster_than_off_in_every_round": all(r["dyn_wall_s"] < r["off_wall_s"] for r in rounds),
           "dyn_faster_than_on_in_every_round": all(r["dyn_wall_s"] < r["on_wall_s"] for r in rounds),
           "on_faster_than_dyn_in_every_round": all(r["on_wall_s"] < r["dyn_wall_s"] for r in rounds),
           "speedup_best_of_rounds": round(min(r["off_wall_s"] for r in rounds) / min(r["on_wall_s"] for r in rounds), 2),
           "file_bytes_gzip4": rounds[-1]["off_file_bytes"], "file_bytes_device": rounds[-1]["on_file_bytes"],
           "file_bytes_device_dynamic": rounds[-1]["dyn_file_bytes"],
           "file_size_ratio_device_to_gzip4": round(rounds[-1]["on_file_bytes"] / rounds[-1]["off_file_bytes"], 3),
           "file_size_ratio_device_dynamic_to_gzip4": round(rounds[-1]["dyn_file_bytes"] / rounds[-1]["off_file_bytes"], 3),
           "dynamic_file_smaller_than_fixed": rounds[-1]["dyn_file_bytes"] < rounds[-1]["on_file_bytes"], "same_records": True}
    if a.out and os.path.isfile(a.out):
        # (the split of the converter before this option existed, measured once on that commit: kept)
        try:
            old = json.loads(open(a.out).read())
            if "parent_split" in old:
                res["parent_split"] = old["parent_split"]
        except ValueError:
            pass
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
