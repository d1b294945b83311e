"""The F(4,3) conv GEMM of the fp32 segment kernel with its k-group loop walked in pairs (dan_device.h conv_gemm_wino43: two
fragment sets that swap roles, fragment loads from a wave-uniform base plus the lane's byte offset).  GPU only.

What can go wrong in that loop: a k-group multiplied with the other set's fragments (the sets swap at every k-group, the last
k-group re-requests its own), a fragment fetched from another wave's or another component's tile (the base is per wave, the
offset per lane), and the remainder tile's plain 3-tap fragments, which go through the same loads.  Any of these changes VALUES,
in the row form and the fold form alike, so the images are held against the direct form of the same library (`conv_algo 1`),
which shares none of that code, and the two forms against each other bit for bit.

The network is the production conv stack (7 layers of 128 channels, pool behind layer 2, residual layers 5-7, 32-channel highway,
FC 1024 / 256) with seeded weights.  Shapes:
  windows   24 (one strip of a lane), 97 (the two halves' overlap), 190 / 191 (the remainder tile off / on), 201 (production),
            206 (the remainder tile full), each at reads 1, 2 and 5: fold form against row form, every output, bit for bit;
  values    at every window, reads 2: the images behind layers 2 (plain, first segment), 5 and 7 (residual) through the tap, row
            form and fold form, against the direct form at tests/test_hip_wino43.py's bar for that comparison: 1e-5 of the tap's
            largest magnitude (the F(4,3) transforms' error at fp32; the direct form is the reference the bar was set against);
  sites     264 x 2 reads (workgroups walk more than one site) and 1 024 x 2 reads (every compute unit over several sites)."""
import dataclasses

import numpy as np
import pytest

from dl4vc_amd import synth
from dl4vc_amd.config import production_config
from dl4vc_amd.model import DanNet
from dl4vc_amd.synth import random_state_dict

pytestmark = pytest.mark.gpu

TAP_F43 = 1e-5
TAP_LAYERS = (2, 5, 7)
WINDOWS = [24, 97, 190, 191, 201, 206]
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
    sd = random_state_dict(cfg, seed=900 + seed)
    arrs = synth.make_sites(n_sites, reads=cfg.reads, length=cfg.length, seed=950 + seed).arrays()
    net = DanNet(cfg, **kw).load_state_dict(sd)
    want = run(net, arrs, 1)
    got = run(net, arrs, 2)
    net.close()
    assert set(want) >= SCORES
    for k in want:
        same_bits(got[k], want[k], "L %d R %d sites %d: %s" % (cfg.length, cfg.reads, n_sites, k))


@pytest.mark.parametrize("reads", [1, 2, 5])
@pytest.mark.parametrize("length", WINDOWS)
def test_fold_form_against_row_form(length, reads):
    fold_against_rows(production_config(reads=reads, length=length), 3, seed=length + reads)


def test_workgroups_walk_more_than_one_site():
    fold_against_rows(production_config(reads=2, length=97), 264, seed=1, max_batch=264, chunk_sites=264)


def test_1024_sites():
    fold_against_rows(production_config(reads=2, length=201), 1024, seed=2, max_batch=1024, chunk_sites=1024)


def taps(cfg, sd, arrs, form):
    B, R, L = arrs[0].shape
    net = DanNet(cfg).load_state_dict(sd)
    net.handle.set_pool_form(form)
    out = {}
    for layer in TAP_LAYERS:
        net.handle.set_tap(layer)
        net.forward_u8(*arrs)
        cpad = net.handle.query("cpad")
        out[layer] = net.handle.read_buffer("tap", B * R * L * cpad).reshape(B, R, L, cpad).astype(np.float64)
    net.close()
    return out


@pytest.mark.parametrize("length", WINDOWS)
def test_images_against_the_direct_form(length):
    """Layers 2, 5 and 7 through the tap, row form and fold form, against the direct form of the same library."""
    cfg = wino(production_config(reads=2, length=length))
    sd = random_state_dict(cfg, seed=300 + length)
    arrs = synth.make_sites(3, reads=2, length=length, seed=400 + length).arrays()
    direct = taps(dataclasses.replace(cfg, conv_algo=1), sd, arrs, 1)
    for form in (1, 2):
        got = taps(cfg, sd, arrs, form)
        for layer in TAP_LAYERS:
            peak = float(np.abs(direct[layer]).max())
            err = float(np.abs(got[layer] - direct[layer]).max())
            print("L %d form %d conv%d: max abs err %.3g = %.3g of the tap's max %.3g (bar %.3g)" % (length, form, layer, err, err / peak, peak, TAP_F43))
            assert peak > 0
            assert err <= TAP_F43 * peak, "L %d form %d conv%d: max abs err %.3g > %.3g x %.3g" % (length, form, layer, err, TAP_F43, peak)
