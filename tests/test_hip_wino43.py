"""Winograd F(4,3) in the fp32 conv layers: one-unit reads of up to 206 columns walk their strip ([0, 96) + [94, 190)) as THREE
tiles of four outputs per lane (points 0, +-1, +-2), with the direct-form remainder tile for columns [190, 206).  GPU only.

Production network (128 channels), 3 sites x 4 reads, fp32.  The reference is oracle/dan_oracle.py in float64, computed once per
window length and shared by the score and the tap checks.  Bars:
  scores            SCORE_ATOL (1e-4), the project's parity bar;
  layer taps        1e-5 of the tap's largest magnitude, over ALL columns -- five times the 2.05e-6 an fp32 emulation of F(4,3)
                    showed against the float64 oracle on the CPU, ten times tighter than TAP_RTOL;
  wide-range case   TAP_RTOL (1e-4), the project's bar: the emulation did not cover such inputs.
Window lengths: the strip ends (8, 9: one tile; 23 .. 25: a lane's 24-column strip; 47, 48: the lower-half lanes' last strip),
the hand-over between the halves (95 .. 97), the remainder tile off / on (189 .. 191), production (201) and the tile full (206)."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from dl4vc_amd import synth
from dl4vc_amd.config import production_config
from dl4vc_amd.model import DanNet
from oracle.dan_oracle import dan_forward_oracle, random_state_dict

pytestmark = pytest.mark.gpu

SCORE_ATOL = 1e-4
TAP_RTOL = 1e-4
TAP_F43 = 1e-5
SCORES = ("vt_prob", "bp")
TAP_LAYERS = (2, 5, 7)
LENGTHS = [8, 9, 23, 24, 25, 47, 48, 95, 96, 97, 189, 190, 191, 201, 206]
SITES, READS = 3, 4


def wino(cfg):
    cfg = dataclasses.replace(cfg, conv_algo=2)
    assert cfg.winograd_applies()
    return cfg


def tap_of(net, arrs, layer):
    """[B][R][L][cpad] image after conv layer `layer` (1-based)."""
    net.handle.set_tap(layer)
    net.forward_u8(*arrs)
    B, R, L = arrs[0].shape
    cpad = net.handle.query("cpad")
    return net.handle.read_buffer("tap", B * R * L * cpad).reshape(B, R, L, cpad).copy()


def tap_close(tap, ref, tol, what):
    """tap [B][R][L][C] against ref (B, C, R, L), float64: max abs error <= tol x the reference tap's largest magnitude"""
    ref = np.asarray(ref, np.float64)
    got = np.transpose(tap[..., :ref.shape[1]], (0, 3, 1, 2)).astype(np.float64)
    peak = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("%s: max abs err %.3g = %.3g of the tap's max %.3g (bar %.3g)" % (what, err, err / peak, peak, tol))
    assert peak > 0
    assert err <= tol * peak, "%s: max abs err %.3g > %.3g x %.3g" % (what, err, tol, peak)


def score_close(got, ref, tol, what):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("%s: max abs err %.3g (bar %.3g)" % (what, err, tol))
    assert err <= tol, "%s: max abs err %.3g > %.3g" % (what, err, tol)


@functools.lru_cache(maxsize=None)
def case(length):
    """(cfg, state dict, planes, float64 oracle with taps) of one window length; read-only for its users"""
    cfg = wino(production_config(reads=READS, length=length))
    sd = random_state_dict(cfg, seed=4300 + length)
    arrs = synth.make_sites(SITES, reads=READS, length=length, seed=4400 + length).arrays()
    want = dan_forward_oracle(sd, cfg, *arrs, taps=True, dtype=torch.float64)
    return cfg, sd, arrs, want


@functools.lru_cache(maxsize=None)
def run(length):
    """the library's scores and layer taps of `case(length)`"""
    cfg, sd, arrs, _ = case(length)
    net = DanNet(cfg).load_state_dict(sd)
    got = dict(net.forward_u8(*arrs, aux=True))
    taps = {layer: tap_of(net, arrs, layer) for layer in TAP_LAYERS}
    net.close()
    return got, taps


@pytest.mark.parametrize("length", LENGTHS)
def test_scores_against_the_float64_oracle(length):
    want = case(length)[3]
    got, _ = run(length)
    for k in SCORES:
        score_close(got[k], want[k], SCORE_ATOL, "L=%d:%s" % (length, k))


@pytest.mark.parametrize("length", LENGTHS)
def test_taps_against_the_float64_oracle(length):
    want = case(length)[3]
    _, taps = run(length)
    for layer in TAP_LAYERS:
        ref = want["conv%d" % layer]
        tap_close(taps[layer], ref, TAP_F43, "L=%d:conv%d" % (length, layer))
        assert np.all(taps[layer][..., ref.shape[1]:] == 0)


@pytest.mark.parametrize("length", [201, 206])
def test_layer7_against_the_direct_form(length):
    cfg, sd, arrs, _ = case(length)
    net = DanNet(dataclasses.replace(cfg, conv_algo=1)).load_state_dict(sd)
    direct = tap_of(net, arrs, 7)
    net.close()
    _, taps = run(length)
    tap_close(taps[7], np.transpose(direct, (0, 3, 1, 2)), TAP_F43, "L=%d: F(4,3) against the direct form, conv7" % length)


def test_wide_dynamic_range():
    """Read 0 of every site has its qualities and strand at the top of their uint8 range (q 0.01 = 2.55, strand 0.5 = 127.5 beside
    embeddings of order one), read 1 at the bottom (quality 1, strand 0), read 2 is ordinary and read 3 empty: the input transform's
    sums of up to 10 |x| and the 1/24 .. 1/4 weights see activations two orders of magnitude apart in one image."""
    L = 201
    cfg = wino(production_config(reads=READS, length=L))
    sd = random_state_dict(cfg, seed=4501)
    arrs = [a.copy() for a in synth.make_sites(SITES, reads=READS, length=L, seed=4502).arrays()]
    rd, ql, st = arrs[0], arrs[1], arrs[2]
    rng = np.random.default_rng(4503)
    rd[:, :3] = rng.integers(1, 5, (SITES, 3, L))
    ql[:, 0] = 255; st[:, 0] = 255
    ql[:, 1] = 1; st[:, 1] = 0
    rd[:, 3] = 0; ql[:, 3] = 0; st[:, 3] = 0
    want = dan_forward_oracle(sd, cfg, *arrs, taps=True, dtype=torch.float64)
    net = DanNet(cfg).load_state_dict(sd)
    got = dict(net.forward_u8(*arrs, aux=True))
    for k in SCORES:
        score_close(got[k], want[k], SCORE_ATOL, "wide range:%s" % k)
    for layer in TAP_LAYERS:
        tap_close(tap_of(net, arrs, layer), want["conv%d" % layer], TAP_RTOL, "wide range:conv%d" % layer)
    net.close()


def unpack_frags(block, comps):
    """[k][kg 8][tile 8][lane 64][4] MFMA A-fragment order -> U[k][o 128][c 128]"""
    f = np.asarray(block).reshape(comps, 8, 8, 64, 4)
    U = np.empty((comps, 128, 128), f.dtype)
    lane = np.arange(64)
    for g in range(8):
        for n in range(8):
            for s in range(4):
                U[:, 16 * n + (lane & 15), 16 * g + 4 * (lane >> 4) + s] = f[:, g, n, :, s]
    return U


def test_weight_blocks():
    """Layers > 1 keep their F(2,3) block where and what it was -- U = [g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2] -- and carry
    U = G g of F(4,3) behind it, both formed in double and rounded once to fp32."""
    cfg, sd, arrs, _ = case(8)
    net = DanNet(cfg).load_state_dict(sd)
    net.forward_u8(*arrs)
    stride, o23, o43 = (net.handle.query(k) for k in ("layer_stride", "wino_f23_offset", "wino_f43_offset"))
    wl = net.handle.read_buffer("wl", cfg.layers * stride).reshape(cfg.layers, stride).copy()
    net.close()
    assert (o23, o43, stride) == (70208, 70208 + 4 * 64 * 256, 70208 + 10 * 64 * 256)
    G43 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)
    for l in range(1, cfg.layers):
        g = np.asarray(sd["conv1D_layers.%d.weight" % l], np.float64).reshape(128, 128, 3)
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]
        u23 = np.stack([g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2]).astype(np.float32)
        got23 = unpack_frags(wl[l, o23:o43], 4)
        assert np.array_equal(got23.view(np.uint32), u23.view(np.uint32)), "layer %d: the F(2,3) block changed" % (l + 1)
        u43 = np.einsum("kt,oct->koc", G43, g)
        got43 = unpack_frags(wl[l, o43:stride], 6).astype(np.float64)
        err = np.abs(got43 - u43)
        assert np.all(err <= 2.0 ** -23 * np.abs(u43) + 1e-45), "layer %d: F(4,3) block, worst %.3g" % (l + 1, float(err.max()))
        assert np.abs(got43).max() > 0
