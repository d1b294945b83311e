#!/usr/bin/env python
"""Writes tests/golden/dataset_downsample.npz from the REFERENCE's own ``sample_single_reads`` (dl4vc/dataset.py:256-287).

Run only where a checkout of the reference exists (``--reference DIR``); never in a test or on the GPU machine.  Nothing of the
reference is copied: its function is called here, at generation time, under ``np.random.seed(s)`` with the coin of
``_get_generator`` (dataset.py:531) drawn first, and what it returns is recorded -- the permutation and the three gathered
planes (quality and strand gathered with the permutation from their untouched arrays, dataset.py:555, :571).

Every case uses one synthetic record of 200 stored rows x 9 columns whose three planes are non-zero everywhere, row 199
included, so that the reference's zeroing of the reads plane of the last row shows.  The rule does not depend on the width.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STORED, WINDOW, MAX_R = 200, 9, 100
NUM_READS = (0, 1, 3, 4, 5, 40, 99, 100, 101, 150, 199, 200, 201, 260, 400)
MODEL_READS = (8, 64, 100)
RATE_PROB = ((0.3, 1.0), (0.3, 0.5), (0.79, 1.0), (0.3, 0.0))
SEEDS = 8
KINDS = ("sampled_zero", "clip_high", "clip_low", "pad_shallow", "pad_deep_last_row_chosen", "first_rows")


def record_planes():
    """reads, qual, strand ``[200][9]`` uint8, no zero byte anywhere."""
    r, c = np.arange(STORED)[:, None], np.arange(WINDOW)[None, :]
    return ((1 + (r + c) % 9).astype(np.uint8), (1 + (3 * r + c) % 60).astype(np.uint8), (1 + (r + c // 4) % 2).astype(np.uint8))


def run_case(d, planes, num_reads, R, rate, prob, seed, drawn):
    """One call of the reference -> (perm, reads, qual, strand [R'][9], kinds)."""
    reads, qual, strand = (np.transpose(p).copy() for p in planes)          # (pos, read), dataset.py:521
    del drawn[:]
    np.random.seed(seed)
    coin = np.random.random()                                                # dataset.py:531
    sampled, perm = d.sample_single_reads(reads, max_reads=R, num_reads=num_reads, random=True,
                                          dynamic_downsample_rate=(rate if coin < prob else 0.))
    perm = np.asarray(perm, np.int64)
    out = [np.ascontiguousarray(np.transpose(a)) for a in (sampled, qual[:, perm], strand[:, perm])]
    rp = min(R, STORED)
    kinds = set()
    kept = num_reads
    if drawn:
        kept = int((1.0 - drawn[0]) * num_reads)
        if drawn[0] == 0.8:
            kinds.add("clip_high")
        if drawn[0] == 0.0:
            kinds.add("clip_low")
        if kept == 0 and num_reads > 0:
            kinds.add("sampled_zero")
    padded = kept < num_reads and min(rp, kept) < rp
    if padded and num_reads < R:
        kinds.add("pad_shallow")
    if padded and num_reads >= STORED and kept > 0 and (perm[:min(rp, kept)] == STORED - 1).any():
        kinds.add("pad_deep_last_row_chosen")
    if rp >= num_reads and kept == num_reads:
        kinds.add("first_rows")
    return perm, out, kept, kinds


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", required=True, help="checkout of the reference (its dl4vc/ package is imported, not copied)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dataset_downsample.npz"))
    args = ap.parse_args()
    from oracle import gen_golden
    gen_golden.REF = args.reference
    _m, d, _u = gen_golden.import_reference()
    drawn = []
    inner = d.double_sample_rate

    def recording(*a, **k):                                   # (the site's clipped rate, to name the kind of the case)
        r = inner(*a, **k)
        drawn.append(float(r))
        return r
    d.double_sample_rate = recording
    planes = record_planes()
    assert all(p.all() for p in planes)
    cases = [(n, R, rate, prob, 1000 * k + 37 * n + R + s)
             for k, (rate, prob) in enumerate(RATE_PROB) for n in NUM_READS for R in MODEL_READS for s in range(SEEDS)]
    seen = set()
    for c in cases:
        seen |= run_case(d, planes, *c, drawn)[3]
    # a kind the listed seeds do not produce: search seeds at the case most likely to give it, and take the place of its last seed
    where = {"sampled_zero": (1, 8, 0.3, 1.0), "clip_high": (150, 100, 0.79, 1.0), "clip_low": (150, 100, 0.3, 1.0),
             "pad_shallow": (40, 64, 0.3, 1.0), "pad_deep_last_row_chosen": (200, 100, 0.79, 1.0), "first_rows": (40, 64, 0.3, 0.0)}
    for kind in KINDS:
        if kind in seen:
            continue
        at = where[kind]
        seed = next(s for s in range(100000, 200000) if kind in run_case(d, planes, *at, s, drawn)[3])
        last = max(i for i, c in enumerate(cases) if c[:4] == at)
        cases[last] = at + (seed,)
        seen.add(kind)
    n = len(cases)
    perm = np.full((n, MAX_R), -1, np.int16)
    zero = np.zeros((n, MAX_R), np.uint8)
    out = [np.zeros((n, MAX_R, WINDOW), np.uint8) for _ in range(3)]
    kept = np.zeros(n, np.int32)
    kinds = np.zeros((n, len(KINDS)), np.uint8)
    for i, c in enumerate(cases):
        p, got, kept[i], ks = run_case(d, planes, *c, drawn)
        k = len(p)
        assert k == min(c[1], STORED) and all(a.shape == (k, WINDOW) for a in got)
        perm[i, :k] = p
        zero[i, :k] = ~got[0].any(axis=1)                    # (no stored byte is zero: a zero row is a row the reference zeroed)
        for dst, a in zip(out, got):
            dst[i, :k] = a
        for kd in ks:
            kinds[i, KINDS.index(kd)] = 1
    missing = [kd for j, kd in enumerate(KINDS) if not kinds[:, j].any()]
    assert not missing, "no case of kind %s" % missing
    cols = list(zip(*cases))
    np.savez_compressed(args.out, record_reads=planes[0], record_qual=planes[1], record_strand=planes[2],
                        num_reads=np.array(cols[0], np.int32), model_reads=np.array(cols[1], np.int32), rate=np.array(cols[2], np.float64),
                        prob=np.array(cols[3], np.float64), seed=np.array(cols[4], np.int64), perm=perm, zero_reads=zero, sampled=kept,
                        reads=out[0], qual=out[1], strand=out[2], kinds=kinds, kind_names=np.array(KINDS))
    print("%s: %d cases, %d bytes; kinds %s" % (args.out, n, os.path.getsize(args.out),
                                                 ", ".join("%s %d" % (kd, kinds[:, j].sum()) for j, kd in enumerate(KINDS))))


if __name__ == "__main__":
    main()
