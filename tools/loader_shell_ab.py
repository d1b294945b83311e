#!/usr/bin/env python
"""Two builds of ``libdl4vc_loader.so`` against each other on the CPU: ``NativeLoader`` sites/s over a generated candidate file
(the host arm of tools/loader_rate.py) and ``NativePileupEncoder.encode`` locations/s over the synthetic 30x BAM of
tools/score_bam_rate.py.  Alternating rounds (A B A B ...), every measurement a fresh process that picks its library through
``DL4VC_LOADER_LIB``, after one pass per library that is kept apart (``warmup``: it reads the inputs into the page cache).
The criterion of each line: B's median is not below A's median by more than A's own max - min.  One JSON record; no GPU is
needed.

    python tools/loader_shell_ab.py --a /path/to/parent/libdl4vc_loader.so [--b dl4vc_amd/csrc/libdl4vc_loader.so]
                                    [--label-a parent --label-b tree] --dir /tmp/lsab
                                    [--records 4096 --length 200000 --rounds 3 --threads 8] [--out profiles/x.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(kind, d, threads):
    """One pass over the whole input; prints one JSON line."""
    if kind == "loader":
        from dl4vc_amd.loader import NativeLoader
        t0 = time.perf_counter()
        with NativeLoader(os.path.join(d, "candidates.hdf"), 100, batch_sites=4096, seed=0, threads=threads) as nl:
            n = sum(len(b) for b in nl)
    else:
        from dl4vc_amd.loader import NativePileupEncoder
        from dl4vc_amd.location_round import default_encoder_options
        from dl4vc_amd.pileup_encoder import locations_from_vcf
        locs = locations_from_vcf(os.path.join(d, "candidates.vcf"), 2)
        contigs, positions = [l.contig for l in locs], [l.pos for l in locs]
        with NativePileupEncoder.from_options(os.path.join(d, "reads.bam"), os.path.join(d, "ref.fa"), default_encoder_options()) as enc:
            t0 = time.perf_counter()
            status = enc.encode(contigs, positions, threads)[5]
        n = int((status == 1).sum())
        assert n > 0.9 * len(locs), "the native path took %d of %d locations" % (n, len(locs))
        n = len(locs)
    print(json.dumps({"n": n, "seconds": time.perf_counter() - t0}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a"), ap.add_argument("--b", default=os.path.join(ROOT, "dl4vc_amd", "csrc", "libdl4vc_loader.so"))
    ap.add_argument("--dir"), ap.add_argument("--out")
    ap.add_argument("--records", type=int, default=4096), ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3), ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--label-a", default="a"), ap.add_argument("--label-b", default="b")
    ap.add_argument("--child")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dir, a.threads)
    import numpy as np
    from dl4vc_amd import hdf5io, synth
    from score_bam_rate import make_inputs
    os.makedirs(a.dir, exist_ok=True)
    hdf = os.path.join(a.dir, "candidates.hdf")
    if not os.path.isfile(hdf):
        base = hdf5io.records_from_sites(synth.make_sites(256, reads=100, seed=31))
        with hdf5io.ChunkWriter(hdf, base.dtype, chunk=8) as w:
            for b0 in range(0, a.records, 1024):
                w.append_records(base[np.arange(b0, min(a.records, b0 + 1024)) % len(base)])
    make_inputs(a.dir, a.length)
    libs = {"a": os.path.abspath(a.a), "b": os.path.abspath(a.b)}
    res = {"libraries": {"a": a.label_a, "b": a.label_b}, "records": a.records, "bam_length": a.length, "threads": a.threads,
           "rounds": a.rounds, "lines": {}}
    for kind, unit in (("loader", "sites_per_s"), ("pileup", "locations_per_s")):
        runs = {"a": [], "b": []}
        warmup = []
        for rnd in range(a.rounds + 1):
            for arm in ("a", "b"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--dir", a.dir, "--threads", str(a.threads)],
                                   capture_output=True, text=True, env=dict(os.environ, DL4VC_LOADER_LIB=libs[arm]))
                if r.returncode != 0:
                    sys.exit("%s on %s failed:\n%s" % (kind, arm, r.stderr[-2000:]))
                got = json.loads(r.stdout.strip().splitlines()[-1])
                (runs[arm] if rnd else warmup).append(got["n"] / got["seconds"])
        med = {k: statistics.median(v) for k, v in runs.items()}
        spread = max(runs["a"]) - min(runs["a"])
        res["lines"][kind] = {"unit": unit, "warmup": warmup, "a": runs["a"], "b": runs["b"], "median_a": med["a"], "median_b": med["b"],
                              "spread_a": spread, "b_not_below_a_by_more_than_its_spread": med["b"] >= med["a"] - spread}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
