"""The two reductions over the read axis behind the segment kernels (csrc/dan_reduce.h: one template, three activation formats)
against numpy, BIT FOR BIT, and the buffer each kernel family hands them.  GPU only.

The reference is the tap of the segment's closing layer.  It is the image the segment stores to y: the fp32 image itself at
precision 0, the bf16 image widened at precision 2, hi + lo of the two bf16 planes at precision 1 (`copy_tap` / `copy_out` in
the three segment kernels read the LDS image the row end then copies to y; checked in the source for all three families, so
none of them is held to a looser bar).  From it
    read mean   pool[s, p, c] = (((+0 + y[s, 0]) + y[s, 1]) + ...) / R
    final pool  feature[s, c * L + p] = max_r y,  feature[s, C * L + c * L + p] = (y[s, 0] + y[s, 1] + ...) / R   (both from row 0)
in float32, where the division is correctly rounded on both sides.  Compared through uint32 views.

The network is the smallest that has both tails: 4 layers, a pool layer behind the second, 24 channels (the mask c < C of the
feature rows and 104 zero channels in y), 3 sites.  Shapes (reads, window):
    (1, 8)    the loops over r >= 1 never run; a window shorter than one pass of positions of the final pool
    (9, 33)   one read past the unroll of 8; one column into a second 32-position tile
    (3, 209)  two units per read at precisions 0 and 1: the segments' y alternates between two buffers and the tail has to read
              the one just written; at precision 2 it never does
The row_src path is covered by the bit-identity tests of skip_empty_rows in test_hip_parity.py."""
import functools

import numpy as np
import pytest

from dl4vc_amd import synth
from dl4vc_amd.config import DanConfig, PRECISION_BF16, PRECISION_BF16X3, PRECISION_F32
from dl4vc_amd.model import DanNet
from dl4vc_amd.synth import random_state_dict

pytestmark = pytest.mark.gpu

SITES, C, CPAD = 3, 24, 128
SHAPES = [(1, 8), (9, 33), (3, 209)]
PRECISIONS = [PRECISION_F32, PRECISION_BF16X3, PRECISION_BF16]
CASES = [pytest.param(p, r, l, id="p%d-%dx%d" % (p, r, l)) for p in PRECISIONS for (r, l) in SHAPES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d words differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


@functools.lru_cache(maxsize=None)
def observe(precision, R, L):
    """Two forwards of one network: the tap behind the pool layer with the read mean, the tap of the last layer with the
    feature rows.  Computed once per case and shared (read-only) by the two tests."""
    cfg = DanConfig(reads=R, length=L, layers=4, pool_layers=(2,), residual_start=0, c_init=C, c_final=C, bottleneck=8,
                    fc_sizes=(32, 16), precision=precision, skip_empty_rows=False)
    net = DanNet(cfg).load_state_dict(random_state_dict(cfg, seed=100 * precision + R))
    h = net.handle
    assert h.query("cpad") == CPAD and h.query("segments") == 2
    if precision == PRECISION_F32:
        h.set_pool_form(1)                                     # the separate tail kernels, not the in-segment form
    arrs = synth.make_sites(SITES, reads=R, length=L, seed=7 + L).arrays()
    out = {}
    for layer, extra in ((2, "pool"), (4, "feature")):
        h.set_tap(layer)
        net.forward_u8(*arrs)
        assert h.query("tap_sites") == SITES and h.query("pool_form") == 1
        out["y%d" % layer] = h.read_buffer("tap", SITES * R * L * CPAD).reshape(SITES, R, L, CPAD).copy()
        n = SITES * L * CPAD if extra == "pool" else SITES * h.query("feature_stride")
        out[extra] = h.read_buffer(extra, n).reshape(SITES, -1).copy()
    net.close()
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("precision,R,L", CASES)
def test_read_mean(precision, R, L):
    o = observe(precision, R, L)
    y = o["y2"]
    assert np.abs(y[..., :C]).max() > 0 and not y[..., C:].any()             # real activations, zero channels behind them
    acc = np.zeros((SITES, L, CPAD), np.float32)
    for r in range(R):
        acc = acc + y[:, r]
    want = acc / np.float32(R)
    assert want.dtype == np.float32
    same_bits(o["pool"].reshape(SITES, L, CPAD), want, "read mean, precision %d, %d x %d" % (precision, R, L))


@pytest.mark.parametrize("precision,R,L", CASES)
def test_final_pool(precision, R, L):
    o = observe(precision, R, L)
    y = o["y4"]
    assert np.abs(y[..., :C]).max() > 0
    mx, acc = y[:, 0].copy(), y[:, 0].copy()
    for r in range(1, R):
        mx = np.maximum(mx, y[:, r])
        acc = acc + y[:, r]
    avg = acc / np.float32(R)
    # [site][p][c] -> the feature row's [c * L + p], channels below C only
    want = np.concatenate([mx[..., :C].transpose(0, 2, 1).reshape(SITES, C * L), avg[..., :C].transpose(0, 2, 1).reshape(SITES, C * L)], axis=1)
    assert want.dtype == np.float32
    same_bits(o["feature"][:, :2 * C * L], want, "final pool, precision %d, %d x %d" % (precision, R, L))
