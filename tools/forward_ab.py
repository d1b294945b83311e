#!/usr/bin/env python
"""Bit comparison of two builds of libdl4vc_dan.so over a fixed list of forward cases.

    DL4VC_DAN_LIB=<library> python tools/forward_ab.py --out A.json     (once per library, one process each)
    python tools/forward_ab.py --compare A.json B.json    (exit 1 on any difference)

Per case the JSON holds the sha256 of every output, of the buffers wl, feature, hidden0, hidden1, pool, h and tap (or the refusal's
text where the case has no such buffer) and the launch counts of dan_kernel_stats.  The cases: the small network of
tests/test_dan_handle_gpu.py (5 sites, chunk_sites 2, max_batch 4) and the golden case dan_small at the three precisions, with
bf16_form 0 / 1, conv_algo 0 / 1 / 2, skip_empty_rows, pool forms 1 / 2, the split window (216 columns, precisions 0 and 1) and the
asynchronous path.  How to build a library from another commit: the header of tools/lib_ab.sh."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

NET = dict(reads=3, length=16, layers=3, c_init=16, c_final=16, bottleneck=8, fc_sizes=(32, 16), pool_layers=(2,), residual_start=3)
KERNELS = ("row_map", "conv_segment", "pool", "highway", "fc")
BUFFERS = ("wl", "feature", "hidden0", "hidden1", "pool", "h", "tap")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cases():
    """(name, network, config overrides, pool form or None, asynchronous)"""
    out = []
    for net in ("small", "dan_small"):
        for p in (0, 1, 2):
            out.append(("%s_p%d" % (net, p), net, dict(precision=p), None, False))
            out.append(("%s_p%d_async" % (net, p), net, dict(precision=p), None, True))
            out.append(("%s_p%d_skip" % (net, p), net, dict(precision=p, skip_empty_rows=True), None, False))
        out.append((net + "_p2_form1", net, dict(precision=2, bf16_form=1), None, False))
        for algo in (1, 2):
            out.append(("%s_p0_algo%d" % (net, algo), net, dict(precision=0, conv_algo=algo), None, False))
        for form in (1, 2):
            out.append(("%s_p0_pool%d" % (net, form), net, dict(precision=0), form, False))
            out.append(("%s_p0_pool%d_async" % (net, form), net, dict(precision=0), form, True))
    for p in (0, 1):
        out.append(("split_p%d" % p, "split", dict(precision=p), None, False))
        out.append(("split_p%d_async" % p, "split", dict(precision=p), None, True))
    return out


def network(name):
    """(config keywords, state dict, six input planes, max_batch, chunk_sites)"""
    from dl4vc_amd import synth
    from dl4vc_amd.config import DanConfig
    if name == "dan_small":
        from golden_util import input_tuple, load_case
        spec, w, inp, _ = load_case("dan_small")
        keys = DanConfig.__dataclass_fields__.keys()
        kw = {k: (tuple(v) if isinstance(v, list) else v) for k, v in spec.items() if k in keys}
        return kw, w, input_tuple(inp), 8, 2                      # 12 sites: macro-batches of 8 and 4, chunks of 2
    kw = dict(NET, reads=2, length=216) if name == "split" else dict(NET)
    sd = synth.random_state_dict(DanConfig(**kw), seed=13 if name == "split" else 11)
    batch = synth.make_sites(5, reads=kw["reads"], length=kw["length"], seed=14 if name == "split" else 12)
    return kw, sd, batch.arrays(), 4, 2


def run_case(net_name, over, pool_form, use_async):
    from dl4vc_amd.config import DanConfig
    from dl4vc_amd.model import DanNet
    kw, sd, planes, max_batch, chunk = network(net_name)
    cfg = DanConfig(**dict(kw, **over))
    net = DanNet(cfg, max_batch=max_batch, chunk_sites=chunk).load_state_dict(sd)
    h = net.handle
    if pool_form is not None:
        h.set_pool_form(pool_form)
    h.set_tap(2)
    h.profile(True)
    n = planes[0].shape[0]
    if use_async:
        tokens = [net.forward_u8_async(*[a[lo:lo + max_batch] for a in planes], aux=True) for lo in range(0, n, max_batch)]
        outs = [net.wait(t) for t in tokens]
        out = {k: np.concatenate([o[k] for o in outs]) for k in outs[0]}
    else:
        out = net.forward_u8(*planes, aux=True)
    rec = {"out:" + k: sha(v) for k, v in sorted(out.items())}
    rec["launches"] = {k: h.kernel_stats(k)[0] for k in KERNELS}
    rec["pool_form"] = h.query("pool_form")
    cap = cfg.layers * max(h.query("layer_stride"), chunk * cfg.reads * cfg.length * 128) + max_batch * h.query("feature_stride")
    for b in BUFFERS:
        try:
            rec["buf:" + b] = sha(h.read_buffer(b, cap))
        except RuntimeError as e:
            rec["buf:" + b] = "refused: " + str(e)
    net.close()
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        a, b = (json.load(open(p)) for p in args.compare)
        diff = [(c, k) for c in sorted(set(a["cases"]) | set(b["cases"]))
                for k in sorted(set(a["cases"].get(c, {})) | set(b["cases"].get(c, {})))
                if a["cases"].get(c, {}).get(k) != b["cases"].get(c, {}).get(k)]
        for c, k in diff:
            print("DIFFERENT %s %s: %s | %s" % (c, k, a["cases"].get(c, {}).get(k), b["cases"].get(c, {}).get(k)))
        print("%d cases, %d values, %d differences (%s vs %s)" % (len(a["cases"]), sum(len(v) for v in a["cases"].values()), len(diff),
                                                                   a["source_hash"], b["source_hash"]))
        return 1 if diff or not a["cases"] else 0
    from dl4vc_amd import capi
    res = {"library": os.path.basename(os.environ.get("DL4VC_DAN_LIB", capi.LIB_PATH)), "source_hash": capi.source_hash(), "cases": {}}
    for name, net_name, over, pool_form, use_async in cases():
        res["cases"][name] = run_case(net_name, over, pool_form, use_async)
        print(name, res["cases"][name]["launches"], flush=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
