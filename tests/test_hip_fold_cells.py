"""The site-owning fold form of the fp32 F(4,3) segment kernel (dan_set_pool_form 2) against the row form with the tail kernels
(form 1), bit for bit, at the shapes where a lane's own cells of the image matter.  GPU only.

The residual layers request the old value of a lane's own cells in front of the barrier that ends the reads of the layer input,
and the fold's running planes are owned element by element; both are exact re-orderings, so every output must come out BIT FOR
BIT the same as the row form's, the sign of a zero included (uint32 views).  Compared: the score arrays and auxiliary heads of
`forward_u8(aux=True)` (bin_logits, vt_logits, vt_prob, bp, ...), the `feature` buffer and the `pool` buffer.

The network is the production conv stack (7 layers of 128 channels, pool behind layer 2, residual layers 5-7, 32-channel highway,
FC 1024 / 256) with seeded weights.  Shapes, the smallest at which a cell mapping can go wrong:
  windows   24 (one strip of a lane), 97 (the two halves' overlap at columns 94-96), 190 / 191 (the remainder tile off / on),
            201 (production), 206 (the remainder tile full); at 191 and 201 the remainder tile lies partly outside the window;
  reads     1 (row 0 alone), 2 (the first update), 5 (several);
  sites     264 x 2 reads: eight workgroups walk two sites each and their planes restart (the handle takes its workgroup count
            from the device, so more sites than workgroups is the way to make one walk two);
            520 x 2 reads at 201 columns: every compute unit busy over more than one site;
  networks  a last segment that ends in a plain layer (c_final != c_init), a first segment that ends in a residual layer;
  values    the images behind layers 5 and 7 through the tap against the direct form of the same library, at the bar
            tests/test_hip_wino43.py uses for that comparison (1e-5 of the tap's largest magnitude)."""
import dataclasses

import numpy as np
import pytest

from dl4vc_amd import synth
from dl4vc_amd.config import production_config
from dl4vc_amd.model import DanNet
from dl4vc_amd.synth import random_state_dict

pytestmark = pytest.mark.gpu

TAP_F43 = 1e-5
SCORES = {"bin_logits", "vt_logits", "vt_prob", "bp", "feature"}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d words differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


def wino(cfg):
    cfg = dataclasses.replace(cfg, conv_algo=2)
    assert cfg.winograd_applies()
    return cfg


def run(net, arrs, form):
    """One forward under pool form `form`: scores + heads, the feature rows and the pool image of the last chunk."""
    h = net.handle
    h.set_pool_form(form)
    out = dict(net.forward_u8(*arrs, aux=True))
    assert h.query("pool_form") == form
    B = arrs[0].shape[0]
    nb = B - (B - 1) // h.query("max_batch") * h.query("max_batch")
    out["feature"] = h.read_buffer("feature", nb * h.query("feature_stride")).copy()
    if h.cfg.pool_layers:
        out["pool"] = h.read_buffer("pool", h.query("tap_sites") * h.cfg.length * h.query("cpad")).copy()
    return out


def fold_against_rows(cfg, n_sites, seed, **kw):
    cfg = wino(cfg)
    sd = random_state_dict(cfg, seed=500 + seed)
    arrs = synth.make_sites(n_sites, reads=cfg.reads, length=cfg.length, seed=600 + seed).arrays()
    net = DanNet(cfg, **kw).load_state_dict(sd)
    want = run(net, arrs, 1)
    got = run(net, arrs, 2)
    net.close()
    assert set(want) >= SCORES
    for k in want:
        same_bits(got[k], want[k], "L %d R %d sites %d: %s" % (cfg.length, cfg.reads, n_sites, k))


@pytest.mark.parametrize("reads", [1, 2, 5])
@pytest.mark.parametrize("length", [24, 97, 190, 191, 201, 206])
def test_windows_and_read_counts(length, reads):
    fold_against_rows(production_config(reads=reads, length=length), 3, seed=length + reads)


def test_a_workgroup_walks_two_sites():
    """264 sites on (at most) 256 workgroups: eight of them own a second site, whose planes start afresh at its row 0."""
    fold_against_rows(production_config(reads=2, length=97), 264, seed=1, max_batch=264, chunk_sites=264)


def test_every_compute_unit_busy_over_several_sites():
    fold_against_rows(production_config(reads=2, length=201), 520, seed=2, max_batch=520, chunk_sites=520)


@pytest.mark.parametrize("which", ["last_segment_ends_plain", "first_segment_ends_residual"])
def test_segment_ends(which):
    base = production_config(reads=3, length=201)
    cfg = {"last_segment_ends_plain": dataclasses.replace(base, c_final=64),
           "first_segment_ends_residual": dataclasses.replace(base, pool_layers=(5,), residual_start=5)}[which]
    last = {"last_segment_ends_plain": False, "first_segment_ends_residual": True}[which]
    first_end = min(cfg.pool_layers)
    assert cfg.is_residual(cfg.layers) == last and cfg.is_residual(first_end) == (which == "first_segment_ends_residual")
    fold_against_rows(cfg, 3, seed=len(which))


def test_residual_images_against_the_direct_form():
    """Layers 5 and 7 (residual) through the tap, fold form: against the direct form of the same library."""
    cfg = wino(production_config(reads=4, length=201))
    sd = random_state_dict(cfg, seed=77)
    arrs = synth.make_sites(3, reads=4, length=201, seed=78).arrays()
    B, R, L = arrs[0].shape

    def taps(c, form):
        net = DanNet(c).load_state_dict(sd)
        net.handle.set_pool_form(form)
        out = {}
        for layer in (5, 7):
            net.handle.set_tap(layer)
            net.forward_u8(*arrs)
            cpad = net.handle.query("cpad")
            out[layer] = net.handle.read_buffer("tap", B * R * L * cpad).reshape(B, R, L, cpad).astype(np.float64)
        net.close()
        return out

    direct = taps(dataclasses.replace(cfg, conv_algo=1), 1)
    got = taps(cfg, 2)
    for layer in (5, 7):
        peak = float(np.abs(direct[layer]).max())
        err = float(np.abs(got[layer] - direct[layer]).max())
        print("conv%d: max abs err %.3g = %.3g of the tap's max %.3g (bar %.3g)" % (layer, err, err / peak, peak, TAP_F43))
        assert peak > 0
        assert err <= TAP_F43 * peak, "conv%d: max abs err %.3g > %.3g x %.3g" % (layer, err, TAP_F43, peak)
