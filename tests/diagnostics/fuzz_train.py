#!/usr/bin/env python3
"""Wider sweep of tests/test_hip_train.py::test_random_structures_train_step_against_float64_oracle (GPU):
python tests/diagnostics/fuzz_train.py [first] [count] [--sites N] [--reads N].  --sites / --reads fix the batch of every structure, so
that the same check sweeps the row counts (sites x reads) at which the step's schedules change (tests/test_hip_train_rows.py): the
trainer is created for that many sites.  A case beyond the tolerance is then classified by tests/diagnostics/fuzz_train_masks.py:
"flip" when the HIP step took a discrete decision (a ReLU mask element, the read that wins the final max) differently from
the float64 oracle on a value at the fp32 rounding level (< 1e-5 of the tensor's scale), FAILED otherwise."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "diagnostics"))
import test_hip_train as T      # noqa: E402
from fuzz_train_masks import decision_differences   # noqa: E402

import argparse   # noqa: E402
ap = argparse.ArgumentParser()
ap.add_argument("first", nargs="?", type=int, default=6)
ap.add_argument("count", nargs="?", type=int, default=48)
ap.add_argument("--sites", type=int, default=None, help="sites of every case (default: the structure's own 1..5)")
ap.add_argument("--reads", type=int, default=None, help="reads per site of every case (default: the structure's own 1..13)")
args = ap.parse_args()
first, count = args.first, args.count
shape = {k: v for k, v in (("sites", args.sites), ("reads", args.reads)) if v is not None}
bad = flips = 0
for seed in range(first, first + count):
    try:
        worst, branch = T.run_random_train_case(seed, **shape)
        print("seed %d ok, %s branch (worst gradient %s at %.2g of its max)" % (seed, branch, worst[0], worst[1]), flush=True)
    except (AssertionError, RuntimeError, ValueError) as e:
        diffs = [d for d in decision_differences(seed, **shape) if d[1]] if isinstance(e, AssertionError) else []
        if diffs and all(rel < 1e-5 for _, _, rel in diffs) and "grad " in str(e):
            flips += 1
            print("seed %d flip (%s): %s" % (seed, "; ".join("%s x%d at %.0e" % d for d in diffs), str(e)[-110:]), flush=True)
        else:
            bad += 1
            print("seed", seed, "FAILED:", str(e)[:600], flush=True)
print("%d structures, %d rounding flips, %d failures" % (count, flips, bad))
sys.exit(1 if bad else 0)
