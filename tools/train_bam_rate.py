#!/usr/bin/env python
"""From a BAM and its location VCF to the first training step, three ways, on one GPU and the seeded synthetic BAM of
tools/score_bam_rate.py (by default 200 kbp at ~30x, 19 940 locations, all with label 2):

* ``file``: the converter with ``--pileup-device gpu`` writes train.hdf (libhdf5's gzip), then the resident fill
  (``--train-loader-device gpu --train-cache-device gpu``) inflates it into the record store;
* ``file_compressed``: the same with ``--compress-device gpu`` (the chunks compressed on the device);
* ``bam``: ``--train_bam`` -- the encoder's planes go into the record store where they lie, no file;
* ``bam_compact``: the same with ``--train-cache-format compact`` (``record_spans`` and ``store_pack_compact`` instead of
  ``record_extent`` and ``store_pack``; fewer stored bytes, which the record reports per format).

``--arms`` runs a subset, in the order given.

Alternating rounds (file file_compressed bam file ...), every process fresh and under its own ``timeout``; the first that fails or
runs out of time ends the run.  Per arm and round: the converter's wall clock (0 for ``bam``), the fill (the construction of the
resident loader, host clock), the time from the start of the arm to the end of the first training step (the production network,
batch ``--batch``), the peak of the device memory in use while the loader was filled and the step ran (sampled every 10 ms from
``hipMemGetInfo``, over what was in use when the process started), and the store's records and bytes, which must agree between the
arms.  Medians over the rounds.  One JSON record.

    python tools/train_bam_rate.py --dir /tmp/tbr [--length 200000 --rounds 3 --threads 16] [--out profiles/train_bam.json]
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

ARMS = ("file", "file_compressed", "bam", "bam_compact")
FROM_BAM = ("bam", "bam_compact")


class Count:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def child(arm, bam, fa, vcf, hdf, batch, threads):
    """The resident loader of one arm and the first training step from it, in this process; prints one JSON line."""
    t_start = time.perf_counter()
    import threading
    import numpy as np
    import torch                                                      # before the HIP libraries: one HIP runtime per process
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing is measured without one")
    from dl4vc_amd import synth
    from dl4vc_amd.chunk_loader import BamSource
    from dl4vc_amd.config import production_config
    from dl4vc_amd.pileup_encoder import locations_from_vcf
    from dl4vc_amd.train import DanTrainer, TrainHyper
    from dl4vc_amd.train_data import DeviceBatchPrefetcher, EasyExampleSampler
    from dl4vc_amd.trainer import train_epoch
    free0, total = torch.cuda.mem_get_info(0)
    peak, stop = [total - free0], threading.Event()

    def watch():
        while not stop.is_set():
            peak[0] = max(peak[0], total - torch.cuda.mem_get_info(0)[0])
            time.sleep(0.01)

    watcher = threading.Thread(target=watch, daemon=True)
    watcher.start()
    cfg, hyper = production_config(), TrainHyper()
    trainer = DanTrainer(cfg, hyper, max_batch=batch).load_state_dict(synth.torch_default_init(cfg, seed=0, dropout_keys=True))
    budget = lambda: torch.cuda.mem_get_info(0)[0] * 3 // 8   # noqa: E731
    t0 = time.perf_counter()
    if arm in FROM_BAM:
        source, cache = BamSource(bam, fa, locations_from_vcf(vcf, label=2), threads=threads), budget
    else:
        source, cache = hdf, budget()
    stamps = []
    with DeviceBatchPrefetcher(source, cfg.reads, batch, use_q=cfg.use_q, use_strand=cfg.use_strand, resident=True, cache_bytes=cache,
                               record_format="compact" if arm == "bam_compact" else "rows") as pf:
        t1 = time.perf_counter()
        sampler = EasyExampleSampler(len(pf), rng=np.random.RandomState(0), plain=True)
        train_epoch(trainer, Count(len(pf)), sampler, hyper, batch, 1, prefetcher=pf, max_batches=1,
                    log=lambda _m: stamps.append(time.perf_counter()))
        stage = {k: round(v, 2) if isinstance(v, float) else int(v) for k, v in pf.stage.items()}
    stop.set()
    watcher.join()
    trainer.close()
    print(json.dumps({"arm": arm, "fill_s": round(t1 - t0, 3), "start_to_first_step_s": round(stamps[0] - t_start, 3),
                      "peak_device_bytes": int(peak[0] - (total - free0)), "store_records": stage["store_records"],
                      "store_bytes": stage["store_bytes"], "stage": stage}))


def step(cmd, limit):
    """One link of the chain: the command under ``timeout``; -> (wall seconds, stdout), or ends the run."""
    t = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        sys.exit("%s ended with status %d after %.1f s; nothing more is started\n%s\n%s"
                 % (" ".join(cmd[1:3] + cmd[-2:]), r.returncode, dt, r.stdout[-1500:], r.stderr[-2500:]))
    return dt, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="working directory (inputs are made there once and reused)")
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="--num-processes of the converter; host threads of the encoders' fallback")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--limit", type=int, default=240, help="seconds each process may take")
    ap.add_argument("--arms", default=",".join(ARMS), help="the arms to run, in this order")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    from score_bam_rate import make_inputs
    bam, fa, vcf, n_loc = make_inputs(a.dir, a.length)
    hdf = os.path.join(a.dir, "train.hdf")
    if a.child:
        child(a.child, bam, fa, vcf, hdf, a.batch, a.threads)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--dir", a.dir, "--length", str(a.length), "--batch", str(a.batch), "--threads", str(a.threads)]
    convert = [sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa,
               "--output", hdf, "--max-reads", "200", "--num-processes", str(a.threads), "--locations-process-step", "100000",
               "--max-insert-length", "10", "--max-insert-length-variant", "50", "--save-q-scores", "--save-strand", "--pileup-device", "gpu"]
    arms = [n for n in a.arms.split(",") if n]
    if not arms or any(n not in ARMS for n in arms):
        sys.exit("--arms: a list of %s" % ", ".join(ARMS))
    rounds = []
    for k in range(a.rounds):
        r = {}
        for arm in arms:
            wall = 0.0
            if arm not in FROM_BAM:
                if os.path.isfile(hdf):
                    os.remove(hdf)
                wall, _ = step(convert + (["--compress-device", "gpu"] if arm == "file_compressed" else []), a.limit)
            dt, out = step(me + ["--child", arm], a.limit)
            r[arm] = json.loads(out.strip().splitlines()[-1])
            r[arm].update(convert_wall_s=round(wall, 3), file_bytes=os.path.getsize(hdf) if arm not in FROM_BAM else 0,
                          bam_to_first_step_s=round(wall + r[arm]["start_to_first_step_s"], 3), child_wall_s=round(dt, 3))
        rounds.append(r)
        print("round %d: %s" % (k, json.dumps(r)), file=sys.stderr, flush=True)
    if os.path.isfile(hdf):
        os.remove(hdf)
    # (the arms of one record format hold the same records in the same bytes)
    held = {compact: {(r[arm]["store_records"], r[arm]["store_bytes"]) for r in rounds for arm in arms if (arm == "bam_compact") == compact}
            for compact in (False, True)}
    if any(len(v) > 1 for v in held.values()) or len({n for v in held.values() for n, _b in v}) != 1:
        sys.exit("the arms hold different records: %s" % [(arm, r[arm]["store_records"], r[arm]["store_bytes"]) for r in rounds for arm in arms])
    res = {"tool": "train_bam_rate", "locations": n_loc, "records": rounds[0][arms[0]]["store_records"],
           "store_bytes": {"compact" if compact else "rows": b for compact, v in held.items() for _n, b in v},
           "batch": a.batch, "threads": a.threads, "same_store_in_every_arm": True, "rounds": rounds,
           "shape": "production network, fp32, batch %d; synthetic BAM of %d bp at ~30x; one GPU" % (a.batch, a.length),
           "not_measured": "more than one GPU; a real 30x genome"}
    for arm in arms:
        res[arm] = {k: round(statistics.median(r[arm][k] for r in rounds), 3)
                    for k in ("convert_wall_s", "fill_s", "bam_to_first_step_s", "peak_device_bytes", "file_bytes")}
        res[arm]["bam_to_first_step_s_rounds"] = [r[arm]["bam_to_first_step_s"] for r in rounds]
        stage = [r[arm]["stage"] for r in rounds]
        res[arm]["bytes_per_record"] = round(stage[0]["store_bytes"] / max(1, stage[0]["store_records"]), 1)
        res[arm]["measure_ms"] = [s["spans_ms"] if arm == "bam_compact" else s["extent_ms"] for s in stage]      # record_spans / record_extent
        res[arm]["pack_ms"] = [s["pack_ms"] for s in stage]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
