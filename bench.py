#!/usr/bin/env python3
"""Throughput of the DAN inference forward on MI355X  (metric of BASELINE.json).

    python bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path (dan_forward_device: token planes -> conv stack (fp32: layer 1 summed from
tables) -> read pooling -> highway -> FC -> heads -> softmax) over one synthetic batch of 65 536 candidate sites x 64 reads x 201
columns per GPU, production network (7 x 128-channel dilated conv, FC 65 792 -> 1024 -> 256), fp32,
seeded random weights (no checkpoint or HG002 data offline).  Inputs are resident in HBM before the
timed region.  For N > 1 the driver launches one rank per GPU with torch.distributed.run; sites shard
with no data-path collective -- RCCL is used only for the barrier and the
max-over-ranks of the elapsed time.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (with the per-kernel HIP-event times and the roofline
figures taken inside the timed steps).  --full adds everything else the benchmark measures or checks, each in a pass of its own
after the timed steps: the oracle comparison and tiling check of the timed outputs, the CPU baseline, the host-buffer pass and
the skip_empty_rows pass (their --no-* options still turn them off one by one).  --dump-outputs DIR writes what rank 0's last
timed step computed as DIR/<name>.npy (float32; inputs and weights are seeded, so two builds can be compared output for output).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3          # /opt/skills/guides/MI355X_MICROARCH.md, v_mfma_f32_16x16x4_f32
PEAK_BF16_MFMA_TFLOPS = 2500.0        # dense bf16 MFMA; the bf16x3 path issues 3 MFMAs per algorithmic product
PEAK_HBM_GBS = 8000.0


def pmc_traffic(section, key, source_hash, chunk_sites=None, profiles_dir=None):
    """(traffic, stale): HBM bytes measured by the newest round's rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE: separate runs of the
    same command, committed as profiles/rNN_traffic.json -- counters cannot be collected inside the timed process).

    The figure is reported only when it was measured on THIS code: the section must carry the ``source_hash`` of the library
    that was profiled (dan_source_hash(), stamped on the PMC run's bench line and copied by tools/summarize_profile.py) and,
    where the bytes depend on it, the same ``chunk_sites`` as the handle being timed chose (the automatic chunk depends on the
    device memory that is free at dan_create).  Otherwise (None, True): stale bytes are not evidence.  (None, False) when no
    capture exists for the section at all."""
    import glob
    tfiles = sorted(glob.glob(os.path.join(profiles_dir or os.path.join(ROOT, "profiles"), "r[0-9][0-9]_traffic.json")))
    if not tfiles:
        return None, False
    with open(tfiles[-1]) as f:
        rec = json.load(f).get(section)
    if not rec or key not in rec:
        return None, False
    if not source_hash or rec.get("source_hash") != source_hash:
        return None, True
    if chunk_sites is not None and rec.get("chunk_sites") != chunk_sites:
        return None, True
    return int(rec[key]), False


def resolve_ranks(args, argv):
    """--gpus N is a promise about how many ranks take part; it is kept here or the run fails.

    * WORLD_SIZE unset, N == 1: this process is the job.
    * WORLD_SIZE unset, N > 1: this process has not touched the GPU yet (nothing above imports torch.cuda state), so it
      starts the N ranks itself -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
      ...` as a CHILD process (never an exec) -- relays the child's stdout / stderr (inherited) and exits with its code.
    * WORLD_SIZE set (the driver's torch.distributed.run launch): it must equal N.
    Returns (rank, local_rank, world) for a process that is a rank."""
    import subprocess
    ws = os.environ.get("WORLD_SIZE")
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if ws is None:
        if args.gpus == 1:
            return 0, 0, 1
        import socket
        import torch
        if not os.environ.get("BENCH_FORCE_DEVICE0"):
            have = torch.cuda.device_count()                 # counts devices without initialising the GPU runtime
            if have < args.gpus:
                raise SystemExit("bench.py: --gpus %d but only %d GPU(s) are visible" % (args.gpus, have))
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
        sys.stderr.write("[bench launcher] --gpus %d without WORLD_SIZE: starting %d ranks: %s\n" % (args.gpus, args.gpus, " ".join(cmd)))
        sys.stderr.flush()
        raise SystemExit(subprocess.call(cmd, env=env))
    world = int(ws)
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d: refusing to report a rank count that is not the one running"
                         % (args.gpus, world))
    return int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), world


def bind_device(local_rank, world):
    """The rank's device; N ranks need N visible devices (BENCH_FORCE_DEVICE0: the one-GPU rehearsal of the tests)."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the DAN path has no CPU form")
    if os.environ.get("BENCH_FORCE_DEVICE0"):
        local_rank = 0
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank with LOCAL_RANK %d of %d, but only %d GPU(s) are visible"
                         % (local_rank, world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    return local_rank


def count_ranks(dist, world, device):
    """All-reduce of ones: the number of ranks that really took part (`ranks_seen` of the line)."""
    if dist is None:
        return 1
    import torch
    t = torch.ones(1, device=device, dtype=torch.int64)
    dist.all_reduce(t)
    seen = int(t.item())
    if seen != world:
        raise SystemExit("bench.py: %d ranks answered the all-reduce, WORLD_SIZE is %d" % (seen, world))
    return seen


def cpu_baseline(cfg, sd, batch, budget_s=20.0, timing=True):
    """The oracle (torch CPU fp32 restatement of the reference's op sequence) on the host cores:
    a bounded sample of the same workload."""
    import torch
    from oracle.dan_oracle import dan_forward_oracle
    # the GPU box grants one GPU's share of the host (16 hardware threads); oversubscribing torch's intra-op
    # pool across all 256 visible threads is slower than using the share
    cores = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(cores)
    n = 32                                                   # ~2 s per pass on 16 threads: 10-15 s of CPU work in all
    arrays = [a[:n] for a in batch.arrays()]
    t0 = time.perf_counter()
    want = dan_forward_oracle(sd, cfg, *arrays)               # warm-up (also sizes the sample); kept: the GPU outputs of
    warm = time.perf_counter() - t0                           # the timed region are checked against it (parity_check)
    if not timing:
        return None, want
    reps = int(max(1, min(5, (budget_s - warm) // max(warm, 1e-3))))
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        dan_forward_oracle(sd, cfg, *arrays)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return {"value": round(n / best, 3), "unit": "candidate-variants/s", "cores": int(cores), "kind": "port",
            "sample": "%d sites x %d reads x %d bp, best of %d passes of oracle/dan_oracle.py (torch CPU fp32); threads = "
                      "min(host threads, 16): the GPU box grants one GPU's share of the host, not all %d visible threads"
                      % (n, cfg.reads, cfg.length, reps, os.cpu_count() or 1)}, want


def parity_check(outs, want, period, precision):
    """Outputs of the LAST timed step against the oracle (first sites of the batch) and the tiling property over the
    whole batch: the synthetic batch repeats `period` distinct sites, and sites are independent (the reference scores
    a site the same wherever it sits in a batch: main.py:94 shuffle=False, trainer.py:569-572), so outs[i] must equal
    outs[i + period] bit for bit across every chunk / macro-batch / XCD-slice boundary."""
    import torch
    bin_l, vt_l, vt_p, bp = outs
    B = vt_p.shape[0]
    res = {"tiled_sites": int(B), "tile_period": int(period)}
    ok = True
    full = (B // period) * period
    tiled = True
    if full >= 2 * period:
        for t in outs:
            v = t[:full].reshape(full // period, period, -1)
            tiled = tiled and bool(torch.equal(v, v[0:1].expand_as(v)))
        if B > full:
            for t in outs:
                tiled = tiled and bool(torch.equal(t[full:], t[:B - full]))
    res["tiled_identical"] = tiled
    ok = ok and tiled
    if want is not None:
        n = want["vt_prob"].shape[0]
        g = lambda t: t[:n].detach().cpu().numpy().astype(np.float64)   # noqa: E731
        e_p = float(np.abs(g(vt_p) - want["vt_prob"]).max())
        e_b = float(np.abs(g(bp) - want["bp"]).max())
        sc = max(1.0, float(np.abs(want["vt_logits"]).max()), float(np.abs(want["bin_logits"]).max()))
        e_l = max(float(np.abs(g(vt_l) - want["vt_logits"]).max()), float(np.abs(g(bin_l) - want["bin_logits"]).max())) / sc
        # north_star: scores within 1e-4 of the reference fp32 forward (fp32 and bf16x3 paths); plain bf16 (config 5) is
        # not a parity path -- its looser bar is the one tests/test_hip_bf16.py holds
        tol = 1e-4 if precision < 2 else 5e-2
        res.update({"oracle_sites": int(n), "max_abs_vt_prob": e_p, "max_abs_bp": e_b, "max_rel_logits": e_l, "tol": tol,
                    "interior_prob_sites": int(((want["vt_prob"].max(axis=1) < 0.999)).sum())})
        ok = ok and e_p <= tol and e_b <= tol and e_l <= tol
    res["ok"] = bool(ok)
    return res


DUMP_BYTES_MAX = 60 << 20            # array bytes: with the .npy headers the files stay below 64 MB (10^6 or 2^20)


def dump_outputs(out_dir, arrays):
    """--dump-outputs: {name: array} of the last timed step -> out_dir/<name>.npy, float32 (float64 where the array is).  Above
    DUMP_BYTES_MAX in all, a fixed sample of rows (seed 0, sorted; every array has one row per site) is written instead, with
    its row numbers as row_index.npy."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.asarray(v, np.float64 if np.asarray(v).dtype == np.float64 else np.float32) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    if total > DUMP_BYTES_MAX:
        rows = max(v.shape[0] for v in arrays.values() if v.ndim)
        keep = min(rows, DUMP_BYTES_MAX // (total // rows + 8))          # + 8 bytes per row: its float64 row number
        idx = np.sort(np.random.default_rng(0).choice(rows, size=keep, replace=False))
        arrays = {k: (v[idx] if v.ndim and v.shape[0] == rows else v) for k, v in arrays.items()}
        arrays["row_index"] = idx.astype(np.float64)
    for k, v in arrays.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(v))


def bench_train(args):
    """--mode train: BASELINE config 4's unit of work -- one optimisation step of the DAN network (train-mode forward with
    BatchNorm batch statistics and dropout, loss mix, backward, gradient clipping, Adam; dl4vc/trainer.py:109-439) on a
    synthetic batch of --train-batch sites x 100 reads x 201 bp per GPU (100 reads: the reference's dataset always yields
    MAX_READS = 100, dl4vc/dataset.py:398), production network, fp32, seeded weights.  N > 1: one process per GPU, the flat
    gradient buffer averaged in two buckets (dl4vc_amd.train.GradientExchange: direct reduce-scatter + all-gather over RCCL,
    the FC-side bucket under the convolution layers' backward; replaces nn.DataParallel, main.py:117); weak scaling."""
    import torch
    from dl4vc_amd.config import DanConfig
    from dl4vc_amd.train import DanTrainer, TrainHyper, example_weights, GradientExchange, base_class_weight_sums
    from dl4vc_amd import synth
    from dl4vc_amd.synth import random_state_dict
    rank, local_rank, world = args.ranks
    local_rank = bind_device(local_rank, world)
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    props = torch.cuda.get_device_properties(local_rank)
    sys.stderr.write("[bench rank %d/%d] pid %d device cuda:%d %s, %d CUs, backend %s (train)\n" %
                     (rank, world, os.getpid(), local_rank, props.name, props.multi_processor_count, backend if world > 1 else "none"))
    sys.stderr.flush()
    ranks_seen = count_ranks(dist, world, torch.device("cuda", local_rank) if backend == "nccl" else "cpu")
    cfg = DanConfig(reads=100, length=args.window, conv_algo=args.conv_algo)
    hp = TrainHyper()
    B = args.train_batch
    sd = random_state_dict(cfg, seed=0)
    tr = DanTrainer(cfg, hp, max_batch=B, device_id=local_rank).load_state_dict(sd)
    batch = synth.tile_sites(synth.make_sites(min(B, 64), reads=cfg.reads, length=cfg.length, seed=rank), B)
    rng = np.random.default_rng(rank)
    tg = {"label": rng.integers(0, 3, B), "var_type": rng.integers(0, 3, B), "allele_freq": rng.random(B).astype(np.float32),
          "coverage": rng.integers(5, 90, B).astype(np.float32), "var_base_enum": rng.integers(1, 6, B),
          "var_ref_enum": rng.integers(1, 5, B), "is_snp": rng.integers(0, 2, B)}
    tg["weight"] = example_weights(tg["is_snp"], hp)
    planes = batch.arrays()
    grad = tr.grad_tensor() if world > 1 else None
    exchange = GradientExchange(dist, world) if world > 1 else None
    (o0, n0), (o1, n1) = tr.grad_buckets()

    sums_dev = "cuda" if backend == "nccl" else "cpu"
    # what the exchange costs a step beyond the device step itself (host clock, this rank): the three-number all-reduce of the loss
    # normalisers in front of it, and the wait from the end of the backward pass (dan_train_backward_end has synchronised) to the
    # end of the last bucket's exchange -- bucket 0 travels under the conv layers' backward, so this is bucket 1 + what of bucket 0
    # did not hide.  tools/scale_run.sh prints it per N.
    ex_ms = {"normalisers": 0.0, "exposed": 0.0, "steps": 0}

    def step(i):
        if world > 1:
            t_a = time.perf_counter()
            g = torch.tensor(base_class_weight_sums(tg), dtype=torch.float64, device=sums_dev)     # full-batch loss normalisers
            dist.all_reduce(g)
            g = g.cpu().numpy() / world
            t_b = time.perf_counter()
            tr.set_global_batch(g[0], g[1], g[2])
            tr.backward_begin(planes, tg, seed=i)
            tr.wait_bucket(0)
            exchange.start(grad[o0:o0 + n0])                  # FC stack + heads: exchanged under the conv layers' backward
            out = tr.backward_end()
            t_c = time.perf_counter()
            exchange.start(grad[o1:o1 + n1])
            exchange.finish()
            t_d = time.perf_counter()
            ex_ms["normalisers"] += (t_b - t_a) * 1e3; ex_ms["exposed"] += (t_d - t_c) * 1e3; ex_ms["steps"] += 1
        else:
            out = tr.backward(planes, tg, seed=i)
        out["grad_norm"] = tr.apply()
        return out

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.warmup):
        step(i)
    fence()
    ex_ms.update(normalisers=0.0, exposed=0.0, steps=0)
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = step(args.warmup + i)
    fence()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=torch.device("cuda", local_rank) if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        from dl4vc_amd.train import LOSS_NAMES
        dump_outputs(args.dump_outputs, {"losses": np.array([last[k] for k in LOSS_NAMES], np.float32), "grad_norm": np.array([last["grad_norm"]], np.float32),
                                         "bin_close": last["bin_close"], "vt_close": last["vt_close"]})
    if rank == 0:
        # algorithmic FLOPs of one step: every GEMM of the forward once more for its data gradient and once for its weight
        # gradient (the layer-1 data gradient IS needed: the embeddings train)
        flops_site = 3.0 * cfg.flops_per_site()
        from dl4vc_amd import capi
        build = {"source_hash": capi.source_hash()}
        traffic, stale = pmc_traffic("train_step_b%d" % B, "hbm_bytes_per_step", build["source_hash"]) if cfg.length == 201 else (None, False)
        value = B * world * args.steps / elapsed
        achieved = value / world * flops_site / 1e12
        line = {"metric": "training sites/sec (DAN train step, 100 reads x %d bp)" % cfg.length, "value": round(value, 2),
                "unit": "sites/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": "f32", "data": "synthetic", "build": build,
                "config": {"workload": "one optimisation step (train-mode forward, focal + aux losses, backward, clip, Adam) on %d sites "
                                       "x 100 reads x %d bp per GPU, DAN production network, seeded random weights" % (B, cfg.length),
                           "sites_per_gpu_per_step": B, "reads": 100, "window": cfg.length,
                           "parallelism": "data-parallel x%d, %d gradient floats averaged per step in two buckets (%s)" % (
                               world, tr.query("num_param_floats"),
                               "no exchange at N=1" if world == 1 else ("direct reduce-scatter + all-gather" if exchange.direct else "all-reduce")),
                           "gflop_per_site": round(flops_site / 1e9, 3)},
                "roofline": {"bound": "mfma", "achieved": round(achieved, 3), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(achieved / PEAK_F32_MFMA_TFLOPS, 4),
                             "traffic": traffic, "traffic_stale": stale,
                             "kernel": "whole step (train_row_kernel + train_wgrad_kernel + train_point_kernel dominate; per-kernel "
                                       "durations and HBM bytes: profiles/rNN_train_kernel_stats.csv, rNN_train_pmc_summary.csv)"},
                "exchange": None if world == 1 else {
                    "form": "direct reduce-scatter + all-gather (all-to-all of 1/N chunks, rank-ordered shard sum)" if exchange.direct else "all-reduce",
                    "backend": backend, "bucket_floats": [int(n0), int(n1)],
                    "exposed_ms_per_step": round(ex_ms["exposed"] / max(ex_ms["steps"], 1), 3),
                    "normalisers_ms_per_step": round(ex_ms["normalisers"] / max(ex_ms["steps"], 1), 3),
                    "note": "rank 0's host clock: exposed = end of the backward pass to the end of the last bucket's exchange"},
                "last_step": {k: round(float(last[k]), 6) for k in ("loss", "bin", "vt", "af", "cov", "vb", "vr")}}
        if args.full and world == 1 and not args.no_cpu_baseline:
            from oracle.dan_train_oracle import train_step_oracle, TrainHyper as OH
            cores = min(os.cpu_count() or 1, 16)
            torch.set_num_threads(cores)
            n = 2
            masks = [np.ones((n, w), np.uint8) for w in (cfg.feature_width,) + tuple(cfg.fc_sizes)]
            ohp = OH(**{k: getattr(hp, k) for k in OH.__dataclass_fields__})
            sub = [a[:n] for a in planes]
            stg = {k: v[:n] for k, v in tg.items()}
            t1 = time.perf_counter()
            train_step_oracle(sd, cfg, sub, stg, ohp, dropout_masks=masks)
            dt = time.perf_counter() - t1
            line["cpu_baseline"] = {"value": round(n / dt, 3), "unit": "sites/s", "cores": int(cores), "kind": "port",
                                    "sample": "one step of oracle/dan_train_oracle.py (torch CPU fp32 autograd) on %d sites x 100 reads x %d "
                                              "bp; threads = min(host threads, 16)" % (n, cfg.length)}
        if not all(np.isfinite(float(last[k])) for k in ("loss", "bin", "vt")):
            print(json.dumps(line), flush=True)
            raise SystemExit("bench.py --mode train: non-finite loss")
        print(json.dumps(line), flush=True)
    tr.close()
    if dist is not None:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="infer", choices=("infer", "train"),
                    help="infer (default, BASELINE.json's headline metric) or train (BASELINE config 4: one optimisation step)")
    ap.add_argument("--train-batch", type=int, default=64, help="--mode train: sites per GPU per step")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sites", type=int, default=65536, help="candidate sites per GPU per step")
    ap.add_argument("--reads", type=int, default=64)
    ap.add_argument("--chunk-sites", type=int, default=0)
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="--full: skip the oracle's timing passes (its one pass used as the parity check of the timed outputs still runs "
                         "unless --no-oracle-check)")
    ap.add_argument("--no-oracle-check", action="store_true", help="--full: skip the oracle comparison of the timed outputs")
    ap.add_argument("--no-host-path", action="store_true",
                    help="--full: omit the informational host-buffer pass (first H2D to last D2H through dan_forward_async/dan_wait)")
    ap.add_argument("--precision", type=int, default=0, help="0 fp32 MFMA (headline), 1 bf16x3 split, 2 bf16")
    ap.add_argument("--window", type=int, default=201)
    ap.add_argument("--conv-algo", type=int, default=0, help="fp32 conv form: 0 auto (Winograd F(2,3) on the dilation-2 "
                                                              "layers), 1 direct, 2 winograd")
    ap.add_argument("--no-skip-pass", action="store_true", help="--full: omit the informational second pass with skip_empty_rows")
    ap.add_argument("--skip-empty-rows", action="store_true",
                    help="compute the all-padding rows of each pileup once per site (bit-identical outputs; off for the headline, "
                         "which computes every row like the reference)")
    ap.add_argument("--full", action="store_true",
                    help="also run the passes beyond the headline: oracle comparison and tiling check of the timed outputs, CPU "
                         "baseline, host-buffer pass, skip_empty_rows pass (off by default: a plain run only times the steps)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what rank 0's last timed step computed as DIR/<name>.npy (float32, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: --steps must be >= 1 and --warmup >= 0")
    args.ranks = resolve_ranks(args, sys.argv[1:])           # may start the ranks as a child job and exit with its code
    if args.mode == "train":
        return bench_train(args)

    import torch
    from dl4vc_amd.config import DanConfig
    from dl4vc_amd.model import DanNet
    from dl4vc_amd import synth
    from dl4vc_amd.synth import random_state_dict          # seeded weights of the reference's shapes

    rank, local_rank, world = args.ranks
    # rehearsal knobs (tests only): several ranks on ONE GPU cannot use RCCL ("duplicate GPU"), so the launch path can
    # be exercised on a one-GPU box with BENCH_FORCE_DEVICE0=1 BENCH_DIST_BACKEND=gloo; the driver's runs use neither
    local_rank = bind_device(local_rank, world)
    backend = os.environ.get("BENCH_DIST_BACKEND", "nccl")
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)

    props = torch.cuda.get_device_properties(local_rank)
    sys.stderr.write("[bench rank %d/%d] pid %d device cuda:%d %s, %d CUs, %.0f GiB, backend %s\n" %
                     (rank, world, os.getpid(), local_rank, props.name, props.multi_processor_count, props.total_memory / 2**30,
                      backend if world > 1 else "none"))
    sys.stderr.flush()

    ranks_seen = count_ranks(dist, world, torch.device("cuda", local_rank) if backend == "nccl" else "cpu")
    cfg = DanConfig(reads=args.reads, length=args.window, precision=args.precision, conv_algo=args.conv_algo,
                    skip_empty_rows=args.skip_empty_rows)
    sd = random_state_dict(cfg, seed=0)
    net = DanNet(cfg, device_id=local_rank, chunk_sites=args.chunk_sites).load_state_dict(sd)

    # synthetic inputs (seed 0 + rank), 256 distinct sites tiled to the batch on the device
    base = synth.make_sites(256, reads=cfg.reads, length=cfg.length, seed=rank)
    reps = -(-args.sites // 256)
    dev = torch.device("cuda", local_rank)
    planes = []
    for a in base.arrays():
        t = torch.from_numpy(a).to(dev)
        t = t.repeat((reps,) + (1,) * (t.dim() - 1))[:args.sites].contiguous()
        planes.append(t)
    B = args.sites
    outs = [torch.empty((B, 2), device=dev), torch.empty((B, 3), device=dev), torch.empty((B, 3), device=dev),
            torch.empty((B,), device=dev)]
    stream = torch.cuda.current_stream().cuda_stream
    in_ptrs = [t.data_ptr() for t in planes]
    out_ptrs = [t.data_ptr() for t in outs] + [0]

    def step():
        net.handle.forward_device(in_ptrs, B, out_ptrs, stream)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    net.handle.profile(True)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    elapsed = time.perf_counter() - t0
    n_launch, seg_ms = net.handle.kernel_stats("conv_segment")
    # the kernel groups behind the dominant one (HIP events, same stream): milliseconds per step
    other_ms = {k: round(net.handle.kernel_stats(k)[1] / args.steps, 3) for k in ("pool", "highway", "fc", "row_map")}
    net.handle.profile(False)
    if dist is not None:
        t = torch.tensor([elapsed], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {k: t.cpu().numpy() for k, t in zip(("bin_logits", "vt_logits", "vt_prob", "bp"), outs)})

    # --full: the outputs of the last timed step, checked: against the oracle on rank 0 (the pass that also sizes the cpu_baseline
    # sample) and through the tiling property on every rank.
    cpu_line, want, parity = None, None, None
    if args.full:
        if rank == 0 and not args.no_oracle_check:
            cpu_line, want = cpu_baseline(cfg, sd, base, timing=(world == 1 and not args.no_cpu_baseline))
        parity = parity_check(outs, want, 256, cfg.precision)

    # Informational (never `value`): SURVEY.md section 8d defines the metric from the first H2D to the last D2H.  One pass
    # of the same batch from PAGEABLE host buffers through the double-buffered asynchronous ABI (pinned staging, H2D /
    # forward / D2H on three streams), outputs checked bit-identical against the device-resident pass.
    host_path = None
    if args.full and world == 1 and not args.no_host_path:
        host = [t.cpu().numpy() for t in planes]
        mb = net.handle.query("max_batch")
        got = {k: [] for k in ("bin_logits", "vt_logits", "vt_prob", "bp")}
        # warm-up of the asynchronous path, untimed like the device-resident pass's: its pinned staging buffers, device mirrors,
        # streams and events are created on first use (2 x 474 MB of pinned memory at 128 x 301: ~170 ms once per handle -- with
        # only four batches in the pass that was the whole of the 0.885 ratio VERDICT r4 read as a staging-copy cost;
        # tools/host_path_trace.sh shows the GPU side of the pass gap-free)
        net.wait(net.forward_u8_async(*[a[:min(64, B)] for a in host]))
        torch.cuda.synchronize()
        th = time.perf_counter()
        prev = None
        for b0 in range(0, B, mb):
            tok = net.forward_u8_async(*[a[b0:b0 + mb] for a in host])
            if prev is not None:
                o = net.wait(prev)
                for k in got:
                    got[k].append(o[k])
            prev = tok
        o = net.wait(prev)
        for k in got:
            got[k].append(o[k])
        eh = time.perf_counter() - th
        same = all(np.array_equal(np.concatenate(got[k]), t.cpu().numpy())
                   for k, t in zip(("bin_logits", "vt_logits", "vt_prob", "bp"), outs))
        host_path = {"value": round(B / eh, 2), "unit": "candidate-variants/s", "sites": B,
                     "definition": "first H2D to last D2H, pageable host inputs and outputs, %d-site batches through "
                                   "dan_forward_async/dan_wait (pinned double-buffered staging)" % mb,
                     "outputs_bit_identical_to_device_resident_pass": bool(same)}
        del host, got

    # Informational second pass (never `value`): the same K steps with the all-padding pileup rows computed once per site
    # (dan_config.skip_empty_rows; outputs bit-identical).  The headline above computes every row, as the reference does.
    skip_value = None
    if args.full and not cfg.skip_empty_rows and not args.no_skip_pass:
        import dataclasses
        net2 = DanNet(dataclasses.replace(cfg, skip_empty_rows=True), device_id=local_rank,
                      chunk_sites=args.chunk_sites).load_state_dict(sd)
        ref_out = [t.clone() for t in outs]
        net2.handle.forward_device(in_ptrs, B, out_ptrs, stream)          # warm-up; also checked against the first pass
        fence()
        identical = all(bool(torch.equal(a, b)) for a, b in zip(ref_out, outs))
        t1 = time.perf_counter()
        for _ in range(args.steps):
            net2.handle.forward_device(in_ptrs, B, out_ptrs, stream)
        fence()
        e2 = time.perf_counter() - t1
        if dist is not None:
            t = torch.tensor([e2], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            e2 = float(t.item())
        skip_value = (B * world * args.steps / e2, identical)
        net2.close()

    if rank == 0:
        # HBM traffic of the dominant kernel: measured by separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE)
        # of this same command and committed under profiles/ (PMC collection cannot run inside the timed process)
        from dl4vc_amd import capi
        build = {"source_hash": capi.source_hash(), "chunk_sites": int(net.handle.query("chunk_sites")),
                 "chunk_sites_auto": bool(net.handle.query("chunk_sites_auto"))}
        section = {(0, 64, 201): "segment_kernel_bytes_per_launch", (2, 128, 301): "segmentp_kernel_bytes_per_launch",
                   (1, 64, 201): "segmentx_kernel_bytes_per_launch"}.get((cfg.precision, cfg.reads, cfg.length))
        traffic, stale = pmc_traffic(section, "total", build["source_hash"], build["chunk_sites"]) if section else (None, False)
        sites_total = B * world * args.steps
        value = sites_total / elapsed
        # roofline of the dominant kernel (conv-stack segment kernel): algorithmic FLOPs = 2 x MAC of every
        # conv / residual / bottleneck GEMM it executes (the 32x32x201 highway compression runs in its own kernel)
        macs_pos = cfg.macs_per_position() - cfg.layers * cfg.bottleneck * cfg.bottleneck
        seg_flops_site = 2.0 * cfg.reads * cfg.length * macs_pos
        seg_flops_total = seg_flops_site * B * args.steps
        achieved = seg_flops_total / (seg_ms * 1e-3) / 1e12 if seg_ms > 0 else None
        # MFMA FLOPs the kernel actually issues: fewer than the algorithmic count when the dilation-2 layers run in
        # Winograd F(2,3) form (4 channel GEMMs per 2 outputs instead of 6); tile padding not counted
        exec_macs = cfg.executed_macs_per_position() - cfg.layers * cfg.bottleneck * cfg.bottleneck
        executed = achieved * exec_macs / macs_pos if achieved else None
        peak = PEAK_F32_MFMA_TFLOPS if cfg.precision == 0 else PEAK_BF16_MFMA_TFLOPS
        line = {
            "metric": "candidate-variants/sec (DAN fwd, %d reads x %d bp)" % (cfg.reads, cfg.length),
            "value": round(value, 2), "unit": "candidate-variants/s", "n_gpus": world, "ranks_seen": ranks_seen, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": ("f32", "bf16x3", "bf16")[cfg.precision], "data": "synthetic", "build": build,
            "config": {"workload": "synthetic %d sites x %d reads x %d bp per GPU per step, DAN production network "
                                   "(7x conv128 dil2, residual 5-7, read-mean after L2, highway 32, FC %d->1024->256), "
                                   "seeded random weights; `value` = device-resident rate (inputs in HBM before the timed region, "
                                   "the bench contract); `value_h2d_to_d2h` = SURVEY section 8d's definition (first H2D to last D2H "
                                   "from pageable host buffers)" % (B, cfg.reads, cfg.length, cfg.feature_width),
                       "sites_per_gpu": B, "reads": cfg.reads, "window": cfg.length, "parallelism": "site-shard x%d" % world,
                       "gflop_per_site": round(cfg.flops_per_site() / 1e9, 3),
                       "skip_empty_rows": bool(cfg.skip_empty_rows),
                       "empty_row_fraction": round(float((base.reads.reshape(-1, cfg.length).max(axis=1) == 0).mean()), 4)},
            "roofline": {"bound": "mfma", "achieved": round(achieved, 3) if achieved else None,
                         "peak": peak, "unit": "TFLOP/s",
                         "frac": round(achieved / peak, 4) if achieved else None, "traffic": traffic, "traffic_stale": stale,
                         "frac_definition": "algorithmic direct-convolution FLOPs / kernel time / peak (the contract's definition; an "
                                            "EFFECTIVE rate where the Winograd form runs and, fp32, layer 1 is summed from tables on the "
                                            "vector ALUs); matrix-pipe utilisation = executed_frac (MFMA FLOPs actually issued)",
                         "conv_algo": "winograd_f23" if cfg.winograd_applies() else "direct",
                         "executed": round(executed, 3) if executed else None,
                         "executed_frac": round(executed / peak, 4) if executed else None,
                         "kernel": "dan::segment_kernel", "launches": n_launch,
                         "avg_launch_ms": round(seg_ms / max(n_launch, 1), 4),
                         "gflop_per_launch": round(seg_flops_total / max(n_launch, 1) / 1e9, 3),
                         "hbm_frac_input_bytes": round(value / world * cfg.input_bytes_per_site() / (PEAK_HBM_GBS * 1e9), 6)},
        }
        if skip_value is not None:
            line["with_skip_empty_rows"] = {"value": round(skip_value[0], 2), "unit": "candidate-variants/s",
                                            "outputs_bit_identical_to_headline_pass": skip_value[1],
                                            "note": "informational: empty pileup rows computed once per site; not the headline"}
        if cpu_line is not None:
            line["cpu_baseline"] = cpu_line
        if parity is not None:
            line["parity"] = parity
        # whole-forward rate against the direct-convolution MFMA ceiling of the precision, for both definitions of the metric
        ceil_sites = peak * 1e12 / cfg.flops_per_site()
        line["roofline"]["whole_forward_frac"] = round(value / world / ceil_sites, 4)
        line["roofline"]["other_kernels_ms_per_step"] = other_ms
        line["roofline"]["kernel_ms_per_step"] = round(seg_ms / args.steps, 3)
        if host_path is not None:
            host_path["ratio_to_value"] = round(host_path["value"] / value, 4)
            line["host_path"] = host_path
            line["value_h2d_to_d2h"] = host_path["value"]
            line["roofline"]["whole_forward_frac_h2d_to_d2h"] = round(host_path["value"] / ceil_sites, 4)
        print(json.dumps(line), flush=True)
    net.close()
    if dist is not None:
        dist.destroy_process_group()
    if parity is not None and not parity["ok"]:
        raise SystemExit("bench.py: outputs of the timed region failed the parity check: %s" % parity)
    if host_path is not None and not host_path["outputs_bit_identical_to_device_resident_pass"]:
        raise SystemExit("bench.py: the host-buffer pass disagrees with the device-resident pass")


if __name__ == "__main__":
    main()
