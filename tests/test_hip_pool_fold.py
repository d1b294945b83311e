"""Read-axis pooling inside the fp32 segment kernel (dan_set_pool_form 2) against the separate tail kernels (form 1).  GPU only.

The in-segment form gives a workgroup whole sites and forms the read-mean behind a pool layer and the final max / mean pool in
the segment kernel, from the same fp32 operations in the same order as read_mean_kernel / final_pool_kernel.  So every output
must come out BIT FOR BIT the same, the sign of a zero included: arrays are compared through their uint32 views.  Compared: the
four score arrays, the auxiliary heads, the `feature` buffer and (where the network has a pool layer) the `pool` buffer."""
import dataclasses

import numpy as np
import pytest
import torch

from dl4vc_amd import synth
from dl4vc_amd.config import DanConfig, PRECISION_BF16, PRECISION_BF16X3, production_config
from dl4vc_amd.model import DanNet
from dl4vc_amd.synth import random_state_dict

pytestmark = pytest.mark.gpu

SMALL = dict(c_init=32, c_final=32, bottleneck=8, fc_sizes=(32, 16))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d words differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def run(net, batch, form=None):
    """One forward; scores + heads, feature rows, the pool image of the last chunk and the form that chunk ran."""
    if form is not None:
        net.handle.set_pool_form(form)
    arrs = batch.arrays()
    out = dict(net.forward_u8(*arrs, aux=True))
    h = net.handle
    cfg = h.cfg
    B = arrs[0].shape[0]
    nb = B - (B - 1) // h.query("max_batch") * h.query("max_batch")          # sites of the last macro-batch
    out["feature"] = h.read_buffer("feature", nb * h.query("feature_stride")).copy()
    if cfg.pool_layers:
        out["pool"] = h.read_buffer("pool", h.query("tap_sites") * cfg.length * h.query("cpad")).copy()
    return out, h.query("pool_form")


def both_forms(cfg, n_sites, seed=0, **kw):
    sd = random_state_dict(cfg, seed=10 + seed)
    batch = synth.make_sites(n_sites, reads=cfg.reads, length=cfg.length, seed=20 + seed)
    net = DanNet(cfg, **kw).load_state_dict(sd)
    want, f1 = run(net, batch, 1)
    got, f2 = run(net, batch, 2)
    net.close()
    assert (f1, f2) == (1, 2)
    assert set(want) >= {"bin_logits", "vt_logits", "vt_prob", "bp", "feature"}
    for k in want:
        same_bits(got[k], want[k], "%s sites %d: %s" % (cfg, n_sites, k))
    return want


@pytest.mark.parametrize("conv_algo", [1, 2], ids=["direct", "winograd"])
@pytest.mark.parametrize("reads", [64, 100])
def test_production_network(reads, conv_algo):
    both_forms(dataclasses.replace(production_config(reads=reads), conv_algo=conv_algo), 5, seed=reads + conv_algo)


@pytest.mark.parametrize("length", [120, 208])
def test_window_lengths(length):
    both_forms(DanConfig(reads=6, length=length, **SMALL), 5, seed=length)


@pytest.mark.parametrize("reads", [1, 5, 128])
def test_read_counts(reads):
    both_forms(DanConfig(reads=reads, **SMALL), 4, seed=reads)


@pytest.mark.parametrize("n_sites", [3, 13, 300, 1024])
def test_site_counts(n_sites):
    """Fewer sites than workgroups; a count that is no multiple of 8; some workgroups own two sites and some one; every
    compute unit busy for several sites."""
    both_forms(DanConfig(reads=4, **SMALL), n_sites, seed=n_sites)


@pytest.mark.parametrize("which", ["no_pool_layer", "three_segments", "no_highway", "residual_opens_segment", "direct_three_segments"])
def test_structures(which):
    kw = {"no_pool_layer": dict(layers=4, pool_layers=(), residual_start=3, **SMALL),
          "three_segments": dict(layers=5, pool_layers=(2, 4), residual_start=0, **SMALL),
          "no_highway": dict(layers=5, pool_layers=(2,), residual_start=4, c_init=48, c_final=48, bottleneck=0, fc_sizes=(32, 16)),
          "residual_opens_segment": dict(layers=6, pool_layers=(3,), residual_start=4, length=203, **SMALL),
          "direct_three_segments": dict(layers=5, pool_layers=(1, 3), residual_start=2, conv_algo=1, c_init=16, c_final=128,
                                        bottleneck=8, fc_sizes=(32, 16))}[which]
    both_forms(DanConfig(reads=7, **kw), 11, seed=len(which))


def test_two_forwards_in_a_row_and_a_second_batch():
    """No state of the running planes survives a site or a call."""
    cfg = DanConfig(reads=5, **SMALL)
    sd = random_state_dict(cfg, seed=3)
    a, b = synth.make_sites(9, reads=5, seed=4), synth.make_sites(20, reads=5, seed=5)
    net = DanNet(cfg).load_state_dict(sd)
    first, _ = run(net, a, 2)
    other, _ = run(net, b, 2)
    again, _ = run(net, a, 2)
    want_b, _ = run(net, b, 1)
    net.close()
    for k in first:
        same_bits(again[k], first[k], "second forward: " + k)
        same_bits(other[k], want_b[k], "other batch: " + k)


def test_chunking_leaves_every_bit_unchanged():
    cfg = DanConfig(reads=8, **SMALL)
    sd = random_state_dict(cfg, seed=5)
    batch = synth.make_sites(37, reads=8, seed=6)
    outs = []
    for kw in (dict(chunk_sites=64, max_batch=64), dict(chunk_sites=5, max_batch=64)):
        net = DanNet(cfg, **kw).load_state_dict(sd)
        out, form = run(net, batch, 2)
        assert form == 2
        outs.append(out)
        net.close()
    for k in outs[0]:
        if k != "pool":                                   # (the pool image is the last chunk's: 37 sites against 2)
            same_bits(outs[1][k], outs[0][k], k)
    L, cpad = cfg.length, 128
    same_bits(outs[1]["pool"], outs[0]["pool"].reshape(37, L * cpad)[35:].ravel(), "pool of the last chunk")


def test_automatic_choice_follows_the_site_count():
    """Form 0: a chunk that deals evenly over the workgroups runs in-segment, small and uneven chunks keep the tail kernels."""
    W = torch.cuda.get_device_properties(0).multi_processor_count & ~7
    assert W >= 8
    cfg = DanConfig(reads=3, **SMALL)
    sd = random_state_dict(cfg, seed=7)
    net = DanNet(cfg, chunk_sites=W, max_batch=W).load_state_dict(sd)
    assert net.handle.query("pool_form") == 2            # what a full chunk would run
    for n, form in ((3, 1), (W + 5, 1), (W, 2)):
        batch = synth.make_sites(n, reads=3, seed=30 + form)
        auto, ran = run(net, batch, 0)
        assert ran == form, (n, ran)
        if n > W:                                         # two chunks: W sites in-segment, then five by the tail kernels
            assert net.handle.query("tap_sites") == n - W
        want, _ = run(net, batch, 1)
        for k in want:
            same_bits(auto[k], want[k], "automatic, %d sites: %s" % (n, k))
    net.close()
    # one chunk of 300 sites: some workgroups would own two sites and some one -> the row form
    net = DanNet(cfg, chunk_sites=512, max_batch=512).load_state_dict(sd)
    batch = synth.make_sites(300, reads=3, seed=33)
    auto, ran = run(net, batch, 0)
    want, _ = run(net, batch, 1)
    net.close()
    assert ran == 1
    for k in want:
        same_bits(auto[k], want[k], "automatic, 300 sites: " + k)


@pytest.mark.parametrize("which", ["bf16x3", "bf16", "window_301", "skip_empty_rows"])
def test_where_the_form_does_not_apply_it_is_refused_with_a_reason(which):
    kw, word = {"bf16x3": (dict(precision=PRECISION_BF16X3), "precision 0"), "bf16": (dict(precision=PRECISION_BF16), "precision 0"),
                "window_301": (dict(length=301), "208 columns"), "skip_empty_rows": (dict(skip_empty_rows=True), "skip_empty_rows")}[which]
    cfg = DanConfig(reads=4, **SMALL, **kw)
    sd = random_state_dict(cfg, seed=9)
    batch = synth.make_sites(3, reads=4, length=cfg.length, seed=9)
    net = DanNet(cfg).load_state_dict(sd)
    assert net.handle.query("pool_form") == 1
    with pytest.raises(RuntimeError, match=word):
        net.handle.set_pool_form(2)
    want, ran = run(net, batch)
    assert ran == 1
    got, ran = run(net, batch, 0)
    assert ran == 1
    for k in want:
        same_bits(got[k], want[k], k)
    with pytest.raises(RuntimeError, match="pool form"):
        net.handle.set_pool_form(3)
    net.close()
