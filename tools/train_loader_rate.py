#!/usr/bin/env python
"""``--train-loader-device gpu`` against the loader workers, on one generated file of production-layout records (200 stored rows of
201 columns, a model of 100 reads) read in shuffled order.

Arms: ``--num-data-workers 5``, ``--num-data-workers 16``, the device loader (``device``) and the device loader with the files resident
(``resident``: ``--train-cache-device gpu``; its fill lies in front of the timed window and is reported on its own as ``fill_ms``, with
the stored bytes per record and their ratio to the inflated bytes) and the same with ``--train-cache-format compact``
(``resident_compact``), or with dynamic read down-sampling of the training epoch at rate 0.3 and prob 0.5 (``resident_downsample``:
``--reads-dynamic-downsample-rate 0.3 --reads-dynamic-downsample-prob 0.5``; its evaluation is the ``resident`` arm's);
``--arms`` runs a subset, in the order given.  Every measurement is a fresh process that runs
the epoch loop of ``main.py --train_file`` -- ``trainer.train_epoch`` over the whole file (a plain shuffled epoch, batches of
``--batch``), then ``trainer.evaluate`` over the test file -- under its own ``timeout``; three alternating rounds; the first
process that fails or runs out of time ends the run.  Per arm and round:

* training steps/s: steps over the time from the end of step ``--skip`` to the end of the last step (the host clock at the loop's
  progress callback; the steps before it load code objects and start the workers), and its ratio to ``bench.py --mode train`` at
  the same batch (the device-resident step rate, one run at the end);
* evaluation sites/s, the same way over the evaluation batches;
* the device loader's stage times summed over the run (``read_ms``, ``plan_ms`` and ``counts_ms`` on the host clock, the others
  between device events);
* host CPU seconds per 1 000 sites: user + system time of the process and of its reaped children (the loader workers) from the
  start of the training loop to the closing of the loaders, over the sites trained and evaluated.  It includes the workers'
  start-up (importing the package, opening the file), which is host time the arm spends.

One JSON record.

    python tools/train_loader_rate.py --dir /tmp/tlr [--records 4096 --test-records 2048 --rounds 3] [--out profiles/train_cache_device.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = (("workers5", 5), ("workers16", 16), ("device", None), ("resident", "resident"), ("resident_compact", "resident_compact"),
        ("resident_downsample", "resident_downsample"))
RESIDENT = ("resident", "resident_compact", "resident_downsample")
DOWNSAMPLE = dict(downsample_rate=0.3, downsample_prob=0.5)          # the ``resident_downsample`` arm's training epoch


def make_inputs(d, records, test_records):
    """-> (train.hdf, test.hdf): seeded labelled records, tiled, gzip-chunked as the converter writes them."""
    import numpy as np
    from dl4vc_amd import hdf5io, synth
    train, test, done = (os.path.join(d, n) for n in ("train.hdf", "test.hdf", "inputs.done"))
    if not os.path.isfile(done):
        base = synth.make_labelled_records(256, 100, 900)
        for path, n in ((train, records), (test, test_records)):
            with hdf5io.ChunkWriter(path, base.dtype, chunk=8) as w:
                for b0 in range(0, n, 1024):
                    w.append_records(base[np.arange(b0, min(n, b0 + 1024)) % len(base)])
        open(done, "w").write("%d %d\n" % (records, test_records))
    return train, test


def cpu_seconds():
    import resource
    a, b = resource.getrusage(resource.RUSAGE_SELF), resource.getrusage(resource.RUSAGE_CHILDREN)
    return a.ru_utime + a.ru_stime + b.ru_utime + b.ru_stime


def child(workers, train, test, batch, skip):
    """One arm in this process; prints one JSON line."""
    import numpy as np
    import torch                                                      # before the HIP libraries: one HIP runtime per process
    if not torch.cuda.is_available():
        sys.exit("no HIP device: nothing is measured without one")
    from dl4vc_amd import synth
    from dl4vc_amd.config import production_config
    from dl4vc_amd.hdf5io import CandidateFile
    from dl4vc_amd.model import DanNet
    from dl4vc_amd.train import DanTrainer, TrainHyper
    from dl4vc_amd.train_data import BatchPrefetcher, DeviceBatchPrefetcher, EasyExampleSampler
    from dl4vc_amd.trainer import evaluate, train_epoch
    cfg, hyper = production_config(), TrainHyper()
    trainer = DanTrainer(cfg, hyper, max_batch=batch).load_state_dict(synth.torch_default_init(cfg, seed=0, dropout_keys=True))

    def loader(path):
        if workers is None:
            return DeviceBatchPrefetcher(path, cfg.reads, batch, use_q=cfg.use_q, use_strand=cfg.use_strand)
        if workers in RESIDENT:
            return DeviceBatchPrefetcher(path, cfg.reads, batch, use_q=cfg.use_q, use_strand=cfg.use_strand, resident=True,
                                         cache_bytes=torch.cuda.mem_get_info(0)[0] * 3 // 8,
                                         record_format="compact" if workers == "resident_compact" else "rows")
        return BatchPrefetcher(path, workers)

    stamps = {"train": [], "eval": []}
    with CandidateFile(train) as src, CandidateFile(test) as tsrc:
        cpu0 = cpu_seconds()
        with loader(train) as tl, loader(test) as el:
            sampler = EasyExampleSampler(len(src), rng=np.random.RandomState(0), plain=True)
            train_epoch(trainer, src, sampler, hyper, batch, 1, prefetcher=tl, log=lambda _m: stamps["train"].append(time.perf_counter()),
                        **(DOWNSAMPLE if workers == "resident_downsample" else {}))
            net = DanNet(cfg, device_id=0, max_batch=batch).load_state_dict(trainer.state_dict())
            evaluate(net, tsrc, hyper, batch, write=lambda _t: stamps["eval"].append(time.perf_counter()), prefetcher=el)
            net.close()
            stages = {}
            if workers is None or workers in RESIDENT:
                for name, l in (("train", tl), ("eval", el)):
                    stages[name] = {k: round(v, 2) if isinstance(v, float) else int(v) for k, v in l.stage.items()}
        cpu1 = cpu_seconds()                                          # (the workers are reaped: their time is in RUSAGE_CHILDREN)
        n_train, n_eval = len(src), len(tsrc)
    trainer.close()
    # (train_epoch's last calls are its closing summary lines: one, and a second with down-sampling)
    tr, ev = stamps["train"][:-2 if workers == "resident_downsample" else -1], stamps["eval"]
    k = min(skip, len(tr) - 2)
    ke = min(2, len(ev) - 2)
    res = {"arm": "device" if workers is None else workers if workers in RESIDENT else "workers%d" % workers, "train_sites": n_train, "eval_sites": n_eval, "steps": len(tr),
           "steps_per_s": round((len(tr) - 1 - k) / (tr[-1] - tr[k]), 3),
           "eval_sites_per_s": round((len(ev) - 1 - ke) * batch / (ev[-1] - ev[ke]), 1),
           "cpu_s": round(cpu1 - cpu0, 2), "cpu_s_per_1000_sites": round((cpu1 - cpu0) * 1000.0 / (n_train + n_eval), 3)}
    if stages:
        res["stages"] = stages
    if workers in RESIDENT:
        both = [stages["train"], stages["eval"]]
        res["fill_ms"] = round(sum(s["fill_ms"] for s in both), 1)
        res["assemble_ms_per_batch"] = round(sum(s["assemble_ms"] for s in both) / (len(tr) + len(ev)), 4)
        res["fallback_records"] = sum(s["store_rows_records"] for s in both) if workers == "resident_compact" else 0
        res["stored_bytes_per_record"] = round(sum(s["store_bytes"] for s in both) / sum(s["store_records"] for s in both), 1)
        res["stored_over_inflated"] = round(sum(s["store_bytes"] for s in both) / sum(s["inflated_bytes"] for s in both), 4)
    print(json.dumps(res))


def step(cmd, limit):
    """One link of the chain: the command under ``timeout``; -> stdout, or ends the run."""
    t = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s ended with status %d after %.1f s; nothing more is started\n%s\n%s"
                 % (" ".join(cmd[-6:]), r.returncode, time.perf_counter() - t, r.stdout[-1500:], r.stderr[-2500:]))
    return r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="working directory (inputs are made there once and reused)")
    ap.add_argument("--records", type=int, default=4096)
    ap.add_argument("--test-records", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--skip", type=int, default=8, help="training steps in front of the timed window")
    ap.add_argument("--limit", type=int, default=240, help="seconds each measured process may take")
    ap.add_argument("--arms", default=",".join(n for n, _w in ARMS), help="the arms to run, in this order")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    os.makedirs(a.dir, exist_ok=True)
    train, test = make_inputs(a.dir, a.records, a.test_records)
    if a.child:
        child(dict(ARMS)[a.child], train, test, a.batch, a.skip)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--dir", a.dir, "--records", str(a.records), "--test-records", str(a.test_records),
          "--batch", str(a.batch), "--skip", str(a.skip)]
    arms = [n for n in a.arms.split(",") if n]
    if not arms or any(n not in dict(ARMS) for n in arms):
        sys.exit("--arms: a list of %s" % ", ".join(n for n, _w in ARMS))
    rounds = []
    for k in range(a.rounds):
        r = {}
        for arm in arms:
            r[arm] = json.loads(step(me + ["--child", arm], a.limit).strip().splitlines()[-1])
        rounds.append(r)
        print("round %d: %s" % (k, json.dumps(r)), file=sys.stderr, flush=True)
    out = step([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "train", "--gpus", "1", "--train-batch", str(a.batch), "--steps", "20",
                "--warmup", "3", "--no-cpu-baseline"], a.limit)
    bench = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    resident = bench["value"] / a.batch
    res = {"tool": "train_loader_rate", "records": a.records, "test_records": a.test_records, "batch": a.batch,
           "shape": "batch %d, 100 reads x 201 bp, production network, fp32; synthetic labelled records, 200 stored rows, chunks of 8, "
                    "one plain shuffled epoch" % a.batch,
           "device_resident_steps_per_s": round(resident, 3), "rounds": rounds, "not_measured": "more than one GPU"}
    for arm in arms:
        res[arm] = {"steps_per_s": [r[arm]["steps_per_s"] for r in rounds],
                    "steps_over_device_resident": [round(r[arm]["steps_per_s"] / resident, 3) for r in rounds],
                    "eval_sites_per_s": [r[arm]["eval_sites_per_s"] for r in rounds],
                    "cpu_s_per_1000_sites": [r[arm]["cpu_s_per_1000_sites"] for r in rounds]}
        for k in ("fill_ms", "stored_bytes_per_record", "stored_over_inflated", "assemble_ms_per_batch", "fallback_records"):
            if k in rounds[0][arm]:
                res[arm][k] = [r[arm][k] for r in rounds]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
