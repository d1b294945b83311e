#!/usr/bin/env python
"""``--loader-device gpu`` against the host loader, on a generated candidate file (by default 32 768 records of the production
layout: 200 stored rows of 201 columns, a model of 100 reads).

(a) The loader alone: ``NativeLoader`` on ``--threads`` host threads against ``DeviceChunkLoader`` (the planes of every batch
ready in device memory), sites per second over the whole file.  (b) The scoring loop of ``main.py --test_file`` with the option
off and on at fp32, bf16x3 and bf16: the loop's own rate as main.py prints it, and with the option on the loader's stage times
(``cl_get_stats`` summed over the run, ``read_ms`` and ``plan_ms`` on the host clock beside them).  Alternating rounds, every
measurement a fresh process under its own ``timeout`` and chained: the first step that fails or runs out of time ends the run.
(c) One more child of the device loader under ``rocprofv3 --kernel-trace --stats``, in a run of its own: the kernels' times.
One JSON record.

    python tools/loader_rate.py --dir /tmp/lr [--records 32768 --rounds 3 --threads 16] [--out profiles/loader_device.json]
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL_FLAGS = ["--model-conv-layers", "7", "--model-residual-layer-start", "5", "--model-batchnorm", "--model-use-q-scores",
               "--model-use-strands", "--model-use-reads-ref-var-mask", "--model-highway-single-reads", "--model_concat_hw_reads",
               "--model_pool_combine_dimension", "0", "--model_middle_layer_dilation", "2", "--model_final_layer_dilation", "2",
               "--model-hidden-dropout", "0.1"]


def make_inputs(d, records):
    """-> (candidates.hdf, checkpoint, sample VCF): seeded synthetic sites, tiled, written 1 024 records at a time."""
    import numpy as np
    import torch
    from dl4vc_amd import hdf5io, synth
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    hdf, ck, sample = (os.path.join(d, n) for n in ("candidates.hdf", "ckpt.pth.tar", "candidates.vcf"))
    if not os.path.isfile(sample):
        base = hdf5io.records_from_sites(synth.make_sites(256, reads=100, seed=31))
        with hdf5io.ChunkWriter(hdf, base.dtype, chunk=8) as w:
            for b0 in range(0, records, 1024):
                part = base[np.arange(b0, min(records, b0 + 1024)) % len(base)]
                w.append_records(part)
        sd = random_state_dict(DanConfig(), seed=12)
        torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {}, "state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
        open(sample, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n")   # (written last)
    return hdf, ck, sample


def child(kind, hdf, threads, batch):
    """One loader over the whole file; prints one JSON line."""
    t0 = time.perf_counter()
    if kind == "native":
        from dl4vc_amd.loader import NativeLoader
        with NativeLoader(hdf, 100, batch_sites=batch, seed=0, threads=threads) as nl:
            n = sum(len(b) for b in nl)
        res = {"sites": n}
    else:
        import torch
        from dl4vc_amd.chunk_loader import DeviceChunkLoader
        with DeviceChunkLoader(hdf, 100, batch_sites=batch, seed=0) as dl:
            dev = torch.device("cuda", 0)
            outs = [torch.empty((batch, 100, 201), dtype=torch.uint8, device=dev) for _ in range(3)] + \
                   [torch.empty((batch, 201), dtype=torch.uint8, device=dev) for _ in range(3)]
            s = torch.cuda.current_stream(dev)
            n = 0
            t0 = time.perf_counter()                                  # (allocation is not the loader's rate)
            for b0 in range(0, len(dl), batch):
                n += len(dl.load(b0, b0 + batch, [t.data_ptr() for t in outs], s.cuda_stream))
                s.synchronize()
            res = {"sites": n, "stages": {k: round(v, 2) if isinstance(v, float) else v for k, v in dl.stage.items()}}
    res["wall_s"] = round(time.perf_counter() - t0, 3)
    res["sites_per_s"] = round(res["sites"] / res["wall_s"])
    print(json.dumps(res))


def step(cmd, limit):
    """One link of the chain: the command under ``timeout``; -> (wall seconds, stdout), or ends the run."""
    t = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        sys.exit("%s ended with status %d after %.1f s; nothing more is started\n%s\n%s"
                 % (" ".join(cmd[:4]), r.returncode, dt, r.stdout[-1500:], r.stderr[-1500:]))
    return dt, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="working directory (inputs are made there once and reused)")
    ap.add_argument("--records", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="host threads of NativeLoader")
    ap.add_argument("--batch", type=int, default=4096, help="sites per launch")
    ap.add_argument("--limit", type=int, default=240, help="seconds each measured process may take")
    ap.add_argument("--no-rocprof", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--hdf", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.hdf, a.threads, a.batch)
        return 0
    os.makedirs(a.dir, exist_ok=True)
    hdf, ck, sample = make_inputs(a.dir, a.records)
    me = [sys.executable, os.path.abspath(__file__), "--dir", a.dir, "--hdf", hdf, "--threads", str(a.threads), "--batch", str(a.batch)]
    score = [sys.executable, os.path.join(ROOT, "main.py"), "--test_file", hdf, "--modelload", ck, "--sample_vcf", sample, "--save_vcf_records",
             "--sites-per-launch", str(a.batch)] + MODEL_FLAGS
    rounds, same = [], True
    for k in range(a.rounds):
        r = {}
        for kind in ("native", "device"):
            _wall, out = step(me + ["--child", kind], a.limit)
            r["loader_" + kind] = json.loads(out.strip().splitlines()[-1])
        for precision in ("fp32", "bf16x3", "bf16"):
            texts = {}
            for mode, flags in (("off", []), ("on", ["--loader-device", "gpu"])):
                out_vcf = os.path.join(a.dir, "%s_%s.vcf" % (precision, mode))
                wall, out = step(score + ["--precision", precision, "--save_vcf_records_file", out_vcf] + flags, a.limit)
                m = re.search(r"scoring loop \(.*?\): (\d+) sites in ([0-9.]+) s = (\d+) sites/s", out)
                e = {"process_s": round(wall, 2), "loop_s": float(m.group(2)), "loop_sites_per_s": int(m.group(3))}
                st = re.search(r"device loader: (.*)", out)
                if st:
                    e["stages"] = {kv.rsplit(" ", 1)[0]: float(kv.rsplit(" ", 1)[1]) for kv in st.group(1).split(", ")}
                r["score_%s_%s" % (precision, mode)] = e
                texts[mode] = open(os.path.join(a.dir, "epoch1_%s_%s.vcf" % (precision, mode))).read()
            same = same and texts["off"] == texts["on"]
        rounds.append(r)
        print("round %d: %s" % (k, json.dumps(r)), file=sys.stderr, flush=True)
    if not same:
        sys.exit("the scored VCF with the option differs from the one without")
    res = {"tool": "loader_rate", "records": a.records, "threads": a.threads, "sites_per_launch": a.batch, "rounds": rounds,
           "same_scored_vcf": True,
           "loader_device_faster_in_every_round": all(r["loader_device"]["sites_per_s"] > r["loader_native"]["sites_per_s"] for r in rounds)}
    for precision in ("fp32", "bf16x3", "bf16"):
        res["loop_on_over_off_" + precision] = [round(r["score_%s_on" % precision]["loop_sites_per_s"] /
                                                       max(1, r["score_%s_off" % precision]["loop_sites_per_s"]), 3) for r in rounds]
    if not a.no_rocprof:
        # counters and traces are separate runs: this one traces kernels only
        prof = os.path.join(a.dir, "rocprof")
        step(["rocprofv3", "--kernel-trace", "--stats", "-d", prof, "--"] + me + ["--child", "device"], 2 * a.limit)
        kernels = {}
        for path in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
            for line in open(path).read().splitlines()[1:]:
                cols = [c.strip('"') for c in line.split(",")]
                if any(n in cols[0] for n in ("zi_inflate_kernel", "assemble_planes")):
                    kernels[cols[0].split("(")[0]] = {"calls": int(cols[1]), "total_ns": int(cols[2]), "average_ns": float(cols[3])}
        res["kernel_stats"] = kernels
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
