#!/usr/bin/env python3
"""End-to-end rate of the TRAINING CLI on the GPU box: train.hdf -> main.py --train_file (loader workers, HIP training step)
against the device-resident step rate of `bench.py --mode train`, written as one JSON record (profiles/rNN_e2e_train.json).
Two epoch sizes per worker count separate the workers' start-up from the steady-state rate (a line through the two points).
In place of a worker count an arm may be named: ``resident`` (--train-loader-device gpu --train-cache-device gpu) or
``resident_downsample`` (the same with --reads-dynamic-downsample-rate 0.3 --reads-dynamic-downsample-prob 0.5).
Usage: python tools/e2e_train_rate.py [n_sites] [workers...]      (E2E_TRAIN_OUT=path for the JSON, default gpurun_out/e2e_train.json)"""
import json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDENT = ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]
NAMED_ARMS = {"resident": RESIDENT,
              "resident_downsample": RESIDENT + ["--reads-dynamic-downsample-rate", "0.3", "--reads-dynamic-downsample-prob", "0.5"]}
sys.path.insert(0, ROOT)
import numpy as np

if __name__ == "__main__":
    from dl4vc_amd import hdf5io
    from dl4vc_amd.synth import make_labelled_records as make_records      # (synthetic labelled records with GT columns; test infrastructure)
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    workers = [w if w in NAMED_ARMS else int(w) for w in sys.argv[2:]] or [0, 5]
    td = tempfile.mkdtemp(prefix="e2e_train_")
    base = make_records(256, 100, 900)
    recs = np.concatenate([base] * (n // 256))
    train = os.path.join(td, "train.hdf")
    test = os.path.join(td, "test.hdf")
    t0 = time.perf_counter()
    hdf5io.write_candidates(train, recs)
    hdf5io.write_candidates(test, base[:64])
    print("wrote %d training records (%.1f MB on disk) in %.1f s" % (len(recs), os.path.getsize(train) / 1e6, time.perf_counter() - t0))
    flags = ["--model-conv-layers", "7", "--model-residual-layer-start", "5", "--model-batchnorm", "--model-use-q-scores",
             "--model-use-strands", "--model-use-reads-ref-var-mask", "--model-highway-single-reads", "--model_concat_hw_reads",
             "--model_pool_combine_dimension", "0", "--model_middle_layer_dilation", "2", "--model_final_layer_dilation", "2",
             "--model-hidden-dropout", "0.1", "--lr", "0.0002", "--grad-clip", "1.0", "--epochs", "1", "--log-interval", "8",
             "--label-smoothing", "0.001", "--batch-size", "64", "--test-batch-size", "64", "--trust-snp-only", "--non-snp-train-weight", "2.0",
             "--fp-train-weight", "0.2", "--auxillary-loss-weight", "1.0", "--auxillary-loss-bases-weight", "0.01",
             "--auxillary-loss-allele-weight", "0.001", "--aux-keep-candidate-af", "--close_match_window", "2.0", "--focal_loss_alpha", "1.",
             "--focal_loss_gamma", "0.2", "--close_examples_sample_rate", "0.15", "--model-ave-pool-layers", "2",
             "--model-init-conv-channels", "128", "--model-final-conv-channels", "128", "--model-bottleneck-size", "32"]
    small = os.path.join(td, "train_small.hdf")
    hdf5io.write_candidates(small, recs[:len(recs) // 4])
    rec = {"shape": "batch 64, 100 reads x 201 bp, production network; synthetic labelled records", "epochs": {}, "sites": [len(recs) // 4, len(recs)]}
    for w in workers:
        pts = []
        for path, m_sites in ((small, len(recs) // 4), (train, len(recs))):
            cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--train_file", path, "--test_file", test, "--modelsave",
                   os.path.join(td, "m%s.pth.tar" % w)] + (NAMED_ARMS[w] if w in NAMED_ARMS else ["--num-data-workers", str(w)]) + flags
            t0 = time.perf_counter()
            r = subprocess.run(cmd, capture_output=True, text=True)
            dt = time.perf_counter() - t0
            if r.returncode:
                print(r.stderr[-2000:])
                sys.exit(1)
            m = re.search(r"Time elapsed for training ([0-9.]+)", r.stdout)
            tt = float(m.group(1))
            pts.append((m_sites, tt))
            print("%s: training epoch of %d sites in %.2f s = %.0f sites/s (whole process %.1f s)"
                  % (w if w in NAMED_ARMS else "--num-data-workers %d" % w, m_sites, tt, m_sites / tt, dt), flush=True)
        (n0, t0_), (n1, t1_) = pts
        per_site = (t1_ - t0_) / (n1 - n0)
        rec["epochs"][str(w)] = {"epoch_s": {str(n0): round(t0_, 3), str(n1): round(t1_, 3)}, "sites_per_s_large_epoch": round(n1 / t1_, 1),
                                 "start_up_s": round(t0_ - per_site * n0, 3), "steady_state_sites_per_s": round(1.0 / per_site, 1)}
    b = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--mode", "train", "--steps", "20", "--warmup", "3", "--no-cpu-baseline"],
                       capture_output=True, text=True)
    line = [l for l in b.stdout.splitlines() if l.startswith("{")]
    dev = json.loads(line[-1])["value"] if line else None
    rec["device_resident_sites_per_s"] = dev
    for w, e in rec["epochs"].items():
        e["ratio_steady_to_device_resident"] = round(e["steady_state_sites_per_s"] / dev, 4) if dev else None
    best = max(rec["epochs"].values(), key=lambda e: e["steady_state_sites_per_s"])
    rec["note"] = ("steady state = the slope between the two epoch sizes (worker start-up removed); with 0 workers the epoch loop assembles every "
                   "batch in-process (HDF5 chunk inflation + site assembly, ~60-70 ms per 64 shuffled sites) and the device waits for it")
    rec["best_ratio"] = best["ratio_steady_to_device_resident"]
    out = os.environ.get("E2E_TRAIN_OUT", os.path.join(ROOT, "gpurun_out", "e2e_train.json"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(rec, open(out, "w"), indent=1)
    print(json.dumps(rec))
