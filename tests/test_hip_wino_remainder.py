"""The one-unit Winograd form of the fp32 segment kernel: six F(2,3) tiles per lane over [0, 96) + [94, 190) and ONE direct-form
position tile per wave for columns [190, 206); reads of 207 and 208 columns keep seven tiles per lane.  GPU only.

Every case runs the production network (128 channels: all eight waves' channel tiles carry data) in fp32 on a handful of sites,
against oracle/dan_oracle.py on the CPU at the parity bars of test_hip_parity.py (SCORE_ATOL / TAP_RTOL, 1e-4).  The layer taps
are compared over ALL columns; with 128 channels a tap has no pad channels, so the narrower network of `test_structures` is the
one that checks them.  The image rows past L are not visible in a tap: a non-zero row there shows in the next layer's columns
L - 2 and L - 1 (the p + 2 taps), which the all-column comparison of layer 7 holds."""
import dataclasses

import numpy as np
import pytest

from dl4vc_amd import synth
from dl4vc_amd.config import DanConfig, production_config
from dl4vc_amd.model import DanNet
from oracle.dan_oracle import dan_forward_oracle, random_state_dict

pytestmark = pytest.mark.gpu

SCORE_ATOL = 1e-4
TAP_RTOL = 1e-4
SCORES = ("vt_prob", "bp")
LOGITS = ("bin_logits", "vt_logits", "af", "cov", "vb", "vr")

# every seam of the mapping: lower/upper hand-over (remainder tile skipped), the last length without the remainder tile, the
# first with it (one live column), production, the remainder tile full, the seven-tile form
LENGTHS = [8, 95, 96, 97, 189, 190, 191, 201, 205, 206, 207, 208]


def close(got, ref, tol, what):
    scale = max(1.0, float(np.abs(ref).max())) if ref.size else 1.0
    err = float(np.abs(got.astype(np.float64) - ref).max()) if ref.size else 0.0
    print("%s: max abs err %.3g, bar %.3g" % (what, err, tol * scale))
    assert err <= tol * scale, "%s: max abs err %.3g > %.3g" % (what, err, tol * scale)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert np.array_equal(bits(a), bits(b)), "%s: %d of %d words differ" % (what, int((bits(a) != bits(b)).sum()), a.size)


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


def check_against_oracle(cfg, sd, arrs, what, tap_layers=(2, 7)):
    want = dan_forward_oracle(sd, cfg, *arrs, taps=True)
    net = DanNet(cfg).load_state_dict(sd)
    got = net.forward_u8(*arrs, aux=True)
    for k in SCORES:
        close(got[k], want[k], SCORE_ATOL, "%s:%s" % (what, k))
    for k in LOGITS:
        close(got[k], want[k], TAP_RTOL, "%s:%s" % (what, k))
    taps = {}
    for layer in tap_layers:
        ref = want["conv%d" % layer]                         # (B, C, R, L)
        taps[layer] = tap = tap_of(net, arrs, layer)
        close(np.transpose(tap[..., :ref.shape[1]], (0, 3, 1, 2)), ref, TAP_RTOL, "%s:conv%d" % (what, layer))
        assert np.all(tap[..., ref.shape[1]:] == 0), "%s: pad channels of conv%d must stay zero" % (what, layer)
    net.close()
    return got, taps


@pytest.mark.parametrize("length", LENGTHS)
def test_window_lengths(length):
    cfg = wino(production_config(reads=4, length=length))
    sd = random_state_dict(cfg, seed=100 + length)
    batch = synth.make_sites(3, reads=4, length=length, seed=200 + length)
    check_against_oracle(cfg, sd, batch.arrays(), "L=%d" % length)


@pytest.mark.parametrize("length", [191, 201, 206])
def test_winograd_against_direct_at_the_seam(length):
    """Layer-7 tap of the Winograd form against the direct form of the same library, columns [184, L): the last Winograd tiles of
    the upper-half lanes and the remainder tile."""
    cfg_w = wino(production_config(reads=3, length=length))
    cfg_d = dataclasses.replace(cfg_w, conv_algo=1)
    sd = random_state_dict(cfg_w, seed=300 + length)
    arrs = synth.make_sites(4, reads=3, length=length, seed=400 + length).arrays()
    taps = {}
    for tag, cfg in (("winograd", cfg_w), ("direct", cfg_d)):
        net = DanNet(cfg).load_state_dict(sd)
        taps[tag] = tap_of(net, arrs, 7)[:, :, 184:, :]
        net.close()
    assert np.abs(taps["direct"]).max() > 0
    close(taps["winograd"], taps["direct"].astype(np.float64), TAP_RTOL, "L=%d: winograd vs direct, columns [184, L)" % length)


@pytest.mark.parametrize("length", [201, 206])
def test_reads_at_the_window_edge(length):
    """Planes written by hand: row 0 ends with its last non-padding base in column L - 1 (the remainder tile's p + 2 taps see the
    zero rows past L), row 1 starts with its first base in column 190 (the remainder tile's first column; nothing but padding
    left of it), row 2 covers the whole window, row 3 is empty."""
    L = length
    rng = np.random.default_rng(length)
    B, R = 2, 4
    rd = np.zeros((B, R, L), np.uint8); ql = np.zeros_like(rd); st = np.zeros_like(rd)
    rf = rng.integers(1, 5, (B, L)).astype(np.uint8)
    rmask = np.zeros((B, L), np.uint8); vmask = np.zeros((B, L), np.uint8)
    for b in range(B):
        for r, (lo, hi) in enumerate(((L - 60, L), (190, L), (0, L))):
            rd[b, r, lo:hi] = rng.integers(1, 5, hi - lo)
            ql[b, r, lo:hi] = rng.integers(2, 42, hi - lo)
            st[b, r, lo:hi] = 1 + (r & 1)
        rmask[b, 195] = rf[b, 195]                       # the alleles sit inside the remainder tile
        vmask[b, 195] = 1 + rf[b, 195] % 4
        rd[b, 0, 195] = rmask[b, 195]; rd[b, 1, 195] = vmask[b, 195]
    assert rd[0, 0, L - 1] != 0 and rd[0, 1, 190] != 0 and not rd[0, 1, :190].any() and not rd[:, 3].any()
    cfg = wino(production_config(reads=R, length=L))
    sd = random_state_dict(cfg, seed=500 + L)
    _, taps = check_against_oracle(cfg, sd, (rd, ql, st, rf, rmask, vmask), "edge reads, L=%d" % L)
    assert np.abs(taps[7][:, :2, 190:, :]).max() > 0     # the remainder tile saw data


def forward(cfg, sd, arrs, form=None, **kw):
    net = DanNet(cfg, **kw).load_state_dict(sd)
    if form is not None:
        net.handle.set_pool_form(form)
    out = dict(net.forward_u8(*arrs, aux=True))
    ran = net.handle.query("pool_form")
    net.close()
    return out, ran


def test_site_owning_form_is_bit_identical_to_the_row_form():
    cfg = wino(production_config(reads=3))
    sd = random_state_dict(cfg, seed=11)
    arrs = synth.make_sites(4, reads=3, seed=12).arrays()
    want, f1 = forward(cfg, sd, arrs, 1)
    got, f2 = forward(cfg, sd, arrs, 2)
    assert (f1, f2) == (1, 2)
    for k in want:
        same_bits(got[k], want[k], k)


def test_chunk_size_and_batch_position_leave_every_bit_unchanged():
    """chunk_sites 256 against the automatic choice, and the site at batch index i against the same site at i + 256."""
    cfg = wino(production_config(reads=2))
    sd = random_state_dict(cfg, seed=13)
    few = synth.make_sites(24, reads=2, seed=14).arrays()
    idx = np.concatenate([np.arange(24), np.full(256 - 24, 23), np.arange(24)])       # sites 256 .. 279 repeat sites 0 .. 23
    arrs = tuple(np.ascontiguousarray(a[idx]) for a in few)
    auto, _ = forward(cfg, sd, arrs)
    c256, _ = forward(cfg, sd, arrs, chunk_sites=256, max_batch=256)
    for k in auto:
        same_bits(c256[k], auto[k], "chunk_sites 256: " + k)
        same_bits(auto[k][256:280], auto[k][:24], "site i + 256 against site i: " + k)


def test_skipping_empty_rows_leaves_every_bit_unchanged():
    cfg = wino(production_config(reads=4))
    sd = random_state_dict(cfg, seed=15)
    arrs = [a.copy() for a in synth.make_sites(4, reads=4, seed=16).arrays()]
    arrs[0][0, 2:] = 0; arrs[1][0, 2:] = 0; arrs[2][0, 2:] = 0          # two empty rows in site 0
    arrs[0][1] = 0; arrs[1][1] = 0; arrs[2][1] = 0                      # a site of only empty rows
    off, _ = forward(cfg, sd, arrs)
    on, _ = forward(dataclasses.replace(cfg, skip_empty_rows=True), sd, arrs)
    for k in off:
        same_bits(on[k], off[k], k)


def test_every_compute_unit_busy_for_several_sites():
    """1 024 sites x 2 reads x 201: the site-owning form against the row form bit for bit, and eight sites spread over the batch
    against the oracle."""
    cfg = wino(production_config(reads=2))
    sd = random_state_dict(cfg, seed=17)
    arrs = synth.make_sites(1024, reads=2, seed=18).arrays()
    want, f1 = forward(cfg, sd, arrs, 1, chunk_sites=1024, max_batch=1024)
    got, f2 = forward(cfg, sd, arrs, 2, chunk_sites=1024, max_batch=1024)
    assert (f1, f2) == (1, 2)
    for k in want:
        same_bits(got[k], want[k], k)
    spots = np.array([0, 1, 255, 256, 511, 700, 1022, 1023])
    ref = dan_forward_oracle(sd, cfg, *(a[spots] for a in arrs))
    for k in SCORES:
        close(got[k][spots], ref[k], SCORE_ATOL, "1024 sites:" + k)
    close(got["vt_logits"][spots], ref["vt_logits"], TAP_RTOL, "1024 sites:vt_logits")


STRUCTURES = {
    # layers 5-7 carry the 1x1 residual GEMM (twelve Winograd-mapped column tiles + the remainder tile): the production network
    "residual": dict(),
    "no_residual": dict(residual_start=0),
    # a residual layer opens the last segment: its x_in is re-read from HBM, in the remainder tile's mapping too
    "three_segments": dict(pool_layers=(2, 4)),
    # 40 of 128 channels: the pad channels of every tile stay zero
    "narrow": dict(c_init=40, c_final=40, bottleneck=8, fc_sizes=(32, 16)),
}


@pytest.mark.parametrize("which", sorted(STRUCTURES))
def test_structures(which):
    cfg = wino(dataclasses.replace(production_config(reads=3), **STRUCTURES[which]))
    sd = random_state_dict(cfg, seed=19)
    arrs = synth.make_sites(4, reads=3, seed=20).arrays()
    want, _ = check_against_oracle(cfg, sd, arrs, which, tap_layers=(5, 7))
    got, ran = forward(cfg, sd, arrs, 2)
    assert ran == 2
    for k in want:
        same_bits(got[k], want[k], "%s, site-owning form: %s" % (which, k))
