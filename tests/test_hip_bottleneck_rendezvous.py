"""The fp32 F(4,3) segment kernel requests the weight fragments of a layer's deferred highway bottleneck GEMM behind the conv GEMM of the
stage that hosts it (dan_kernels.hip WBOT_EARLY); the GEMM itself sits where it sat.  This file pins the `h` rows it writes.  GPU only.

In the six F(4,3) forms a layer's 128 -> 32 bottleneck GEMM runs inside the NEXT layer's conv stage, on the four older waves, while
the image is still that layer's output.  Whatever orders it against the younger waves' conv GEMM and epilogue --
today nothing but barrier A behind it; a rendezvous (a workgroup barrier or a token in LDS) was built, measured and not kept,
HISTORY section 41 -- can fail in two ways: wrong `h` rows (the GEMM read an image already overwritten, or ran before the previous
write-back had landed), or a hang, which the suite's per-test time limit catches.  So:

  forms     fold form (dan_set_pool_form 2) against row form (1), every output of `forward_u8(aux=True)` -- bin_logits, vt_logits,
            vt_prob, bp and the 22 columns of the auxiliary heads -- plus the feature rows and the pool image, bit for bit: windows
            24 (one short strip), 190 (the last without the remainder tile), 191 (the first with it), 201 (production), 206 (the
            last one-unit length), each at reads 1 and 2;
  rows      the persistent row walk: `skip_empty_rows` at 201 x 2 reads with one all-padding read per site, against every row computed;
  values    the highway half of the feature row, layer by layer, against oracle/dan_oracle.py (`hw{l}`), row form and fold form,
            at the bar of tests/test_hip_parity.py (1e-4 of the tensor's largest magnitude): the direct check on `h`;
  sequence  264 sites x 2 reads (eight workgroups walk two sites) and 520 x 2 at 201 columns: many rows per workgroup, across the
            row back edge and the site end; at 264 x 2 the highway half is also held to the oracle, layer by layer, in the fold
            form (both forms carry the same fragment request: only the oracle is independent of it);
  cuts      a first segment ending in a residual layer and a last segment ending in a plain one (the structures of
            tests/test_hip_fold_cells.py): another stage hosts the deferred GEMM.

The network is the production conv stack (7 layers of 128 channels, pool behind layer 2, residual layers 5-7, 32-channel highway,
FC 1024 / 256) with seeded weights."""
import dataclasses

import numpy as np
import pytest

from dl4vc_amd import synth
from dl4vc_amd.config import production_config
from dl4vc_amd.model import DanNet
from dl4vc_amd.synth import random_state_dict
from oracle.dan_oracle import dan_forward_oracle

pytestmark = pytest.mark.gpu

TAP_RTOL = 1e-4         # tests/test_hip_parity.py: intermediate tensors to 1e-4 of their largest magnitude (at least 1)
WINDOWS = [24, 190, 191, 201, 206]
SCORES = {"bin_logits", "vt_logits", "vt_prob", "bp", "af", "cov", "vb", "vr", "feature"}


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
    sd = random_state_dict(cfg, seed=1100 + seed)
    arrs = synth.make_sites(n_sites, reads=cfg.reads, length=cfg.length, seed=1150 + seed).arrays()
    net = DanNet(cfg, **kw).load_state_dict(sd)
    want = run(net, arrs, 1)
    got = run(net, arrs, 2)
    net.close()
    assert set(want) >= SCORES
    assert want["af"].shape[1] + want["cov"].shape[1] + want["vb"].shape[1] + want["vr"].shape[1] == 22
    for k in want:
        same_bits(got[k], want[k], "L %d R %d sites %d: %s" % (cfg.length, cfg.reads, n_sites, k))


@pytest.mark.parametrize("reads", [1, 2])
@pytest.mark.parametrize("length", WINDOWS)
def test_fold_form_against_row_form(length, reads):
    fold_against_rows(production_config(reads=reads, length=length), 3, seed=length + reads)


def test_persistent_row_walk_with_an_empty_read_per_site():
    """`skip_empty_rows`: the persistent form walks the list of rows to do; one all-padding read per site is computed once."""
    cfg = wino(production_config(reads=2, length=201))
    sd = random_state_dict(cfg, seed=1201)
    arrs = [a.copy() for a in synth.make_sites(5, reads=2, length=201, seed=1202).arrays()]
    reads, qual, strand = arrs[0], arrs[1], arrs[2]
    reads[:, 1], qual[:, 1], strand[:, 1] = 0, 0, 0
    assert (reads[:, 0].max(axis=1) > 0).all()
    outs = []
    for skip in (False, True):
        net = DanNet(dataclasses.replace(cfg, skip_empty_rows=skip)).load_state_dict(sd)
        outs.append(dict(net.forward_u8(*arrs, aux=True)))
        F = net.handle.query("feature_stride")
        outs[-1]["feature"] = net.handle.read_buffer("feature", 5 * F).copy()
        net.close()
    assert set(outs[0]) >= SCORES
    for k in outs[0]:
        same_bits(outs[1][k], outs[0][k], "skip_empty_rows: " + k)


@pytest.fixture(scope="module")
def highway_case():
    cfg = wino(production_config(reads=2, length=201))
    sd = random_state_dict(cfg, seed=1301)
    arrs = synth.make_sites(3, reads=2, length=201, seed=1302).arrays()
    want = dan_forward_oracle(sd, cfg, *arrs, taps=True)
    return cfg, sd, arrs, want


def highway_rows_against_the_oracle(cfg, sd, arrs, want, form, **kw):
    """Every layer's block of the feature row's highway half, relu(hw{l}), against the oracle's taps `want`."""
    net = DanNet(cfg, **kw).load_state_dict(sd)
    net.handle.set_pool_form(form)
    net.forward_u8(*arrs)
    assert net.handle.query("pool_form") == form
    F, Fs = net.handle.query("feature_width"), net.handle.query("feature_stride")
    B, R, L = arrs[0].shape
    feat = net.handle.read_buffer("feature", B * Fs).reshape(B, Fs)[:, :F].astype(np.float64)
    net.close()
    at = 2 * cfg.c_final * L
    assert F == at + sum(want["hw%d" % l].shape[1] for l in range(1, cfg.layers + 1))
    for l in range(1, cfg.layers + 1):
        ref = np.maximum(want["hw%d" % l].astype(np.float64), 0.0)
        got = feat[:, at:at + ref.shape[1]]
        at += ref.shape[1]
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(got - ref).max())
        print("%d sites, form %d hw%d: max abs err %.3g against a bar of %.3g (largest magnitude %.3g, %d of %d positive)"
              % (B, form, l, err, TAP_RTOL * scale, float(np.abs(ref).max()), int((ref > 0).sum()), ref.size))
        assert (ref > 0).any(), "hw%d is all zero: the comparison would be vacuous" % l
        assert err <= TAP_RTOL * scale, "%d sites, form %d hw%d: max abs err %.3g > %.3g" % (B, form, l, err, TAP_RTOL * scale)


@pytest.mark.parametrize("form", [1, 2])
def test_highway_rows_against_the_oracle(highway_case, form):
    cfg, sd, arrs, want = highway_case
    highway_rows_against_the_oracle(cfg, sd, arrs, want, form)


def test_highway_rows_of_two_sites_per_workgroup_against_the_oracle():
    """264 sites x 2 reads, fold form: eight workgroups walk a second site; every site's `h` rows against the oracle."""
    cfg = wino(production_config(reads=2, length=97))
    sd = random_state_dict(cfg, seed=1401)
    arrs = synth.make_sites(264, reads=2, length=97, seed=1402).arrays()
    want = dan_forward_oracle(sd, cfg, *arrs, taps=True)
    highway_rows_against_the_oracle(cfg, sd, arrs, want, 2, max_batch=264, chunk_sites=264)


def test_workgroups_walk_two_sites():
    fold_against_rows(production_config(reads=2, length=97), 264, seed=1, max_batch=264, chunk_sites=264)


def test_520_sites_at_201_columns():
    fold_against_rows(production_config(reads=2, length=201), 520, seed=2, max_batch=520, chunk_sites=520)


@pytest.mark.parametrize("which", ["last_segment_ends_plain", "first_segment_ends_residual"])
def test_segment_cuts(which):
    base = production_config(reads=3, length=201)
    cfg = {"last_segment_ends_plain": dataclasses.replace(base, c_final=64),
           "first_segment_ends_residual": dataclasses.replace(base, pool_layers=(5,), residual_start=5)}[which]
    last = {"last_segment_ends_plain": False, "first_segment_ends_residual": True}[which]
    first_end = min(cfg.pool_layers)
    assert cfg.is_residual(cfg.layers) == last and cfg.is_residual(first_end) == (which == "first_segment_ends_residual")
    fold_against_rows(cfg, 3, seed=len(which))
