"""The inference handle (``dan_*``, dl4vc_amd/csrc/dan_capi.cpp) over its life on the MI355X: every device resource of the handle is
a member that frees itself (dl4vc_amd/csrc/device_buffer.h), so what can go wrong is the order in which they go, two handles
sharing a process, resources that are made late (the asynchronous path's streams and slots, the tap buffer), and a handle that is
used again after a call was refused.  Each case repeats a forward whose result is known and compares byte for byte, no tolerance.

The network is the smallest with every structural feature: 3 reads, window 16, 3 layers of 16 channels, bottleneck 8, FC (32, 16),
a pool layer after layer 2 (two segments) and a residual on layer 3.  The batch is 5 sites with chunk_sites=2 and max_batch=4:
chunks of 2, 2 and 1 sites across a macro-batch boundary.  (The drain of a failed dan_forward_async is not tested: it would take
a provoked fault.)"""
import numpy as np
import pytest

from dl4vc_amd import synth
from dl4vc_amd.config import DanConfig
from dl4vc_amd.model import DanNet

pytestmark = pytest.mark.gpu
SITES, CHUNK, MAX_BATCH = 5, 2, 4
NET = dict(reads=3, length=16, layers=3, c_init=16, c_final=16, bottleneck=8, fc_sizes=(32, 16), pool_layers=(2,), residual_start=3)


def _cfg(**over):
    return DanConfig(**dict(NET, **over))


def _open(sd, chunk=CHUNK, **over):
    return DanNet(_cfg(**over), max_batch=MAX_BATCH, chunk_sites=chunk).load_state_dict(sd)


def _bytes(out):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in sorted(out))


def _sync(net, batch):
    return _bytes(net.forward_u8(*batch.arrays(), aux=True))


def _async(net, batch):
    """The batch in pieces of at most max_batch sites, two in flight."""
    tokens = [net.forward_u8_async(*batch.slice(lo, min(lo + MAX_BATCH, len(batch))).arrays(), aux=True) for lo in range(0, len(batch), MAX_BATCH)]
    outs = [net.wait(t) for t in tokens]
    return _bytes({k: np.concatenate([o[k] for o in outs]) for k in outs[0]})


@pytest.fixture(scope="module")
def sd():
    return synth.random_state_dict(_cfg(), seed=11)


@pytest.fixture(scope="module")
def batch():
    return synth.make_sites(SITES, reads=NET["reads"], length=NET["length"], seed=12)


@pytest.fixture(scope="module")
def first(sd, batch):
    """The result every later call is compared with, per precision: one handle, one synchronous call."""
    want = {}
    for precision in (0, 1, 2):
        net = _open(sd, precision=precision)
        assert net.handle.query("chunk_sites") == CHUNK and net.handle.query("max_batch") == MAX_BATCH and net.handle.query("segments") == 2
        want[precision] = _sync(net, batch)
        net.close()
    assert len({len(w) for w in want.values()}) == 1 and len(want[0]) == SITES * 31 * 4
    return want


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_handle_opened_and_closed_twice(sd, batch, first, precision):
    for _ in range(2):
        net = _open(sd, precision=precision)
        assert _sync(net, batch) == first[precision]
        assert _async(net, batch) == first[precision]
        net.close()


def test_two_handles_called_alternately(sd, batch, first):
    a, b = _open(sd, precision=0), _open(sd, precision=2)
    for _ in range(2):
        assert _sync(a, batch) == first[0]
        assert _async(b, batch) == first[2]
        assert _async(a, batch) == first[0]
        assert _sync(b, batch) == first[2]
    a.close()
    b.close()


def test_handle_after_refused_calls(sd, batch, first):
    net = _open(sd)
    h = net.handle

    def still_good():
        assert _sync(net, batch) == first[0]
        assert _async(net, batch) == first[0]

    with pytest.raises(RuntimeError, match=r"takes 0\.\.max_batch \(4\) sites per call, got 5"):
        net.forward_u8_async(*batch.arrays())
    still_good()
    with pytest.raises(RuntimeError, match=r"dan_wait\(99\): no such batch in flight"):
        net.wait((99, {}))
    still_good()
    two = [net.forward_u8_async(*batch.slice(0, 4).arrays(), aux=True), net.forward_u8_async(*batch.slice(4, 5).arrays(), aux=True)]
    with pytest.raises(RuntimeError, match="two batches are already in flight"):
        net.forward_u8_async(*batch.slice(0, 1).arrays())
    with pytest.raises(RuntimeError, match="while asynchronous batches are in flight"):
        net.forward_u8(*batch.arrays())
    outs = [net.wait(t) for t in two]
    assert _bytes({k: np.concatenate([o[k] for o in outs]) for k in outs[0]}) == first[0]
    still_good()
    with pytest.raises(RuntimeError, match="pool form 3"):
        h.set_pool_form(3)
    still_good()
    with pytest.raises(RuntimeError, match="unknown buffer 'nope'"):
        h.read_buffer("nope", 16)
    still_good()
    net.close()


def test_finalize_failures_close_cleanly(sd, batch, first):
    missing = {k: v for k, v in sd.items() if k != "fcHidden2VT.bias"}
    net = DanNet(_cfg(), max_batch=MAX_BATCH, chunk_sites=CHUNK)
    with pytest.raises(RuntimeError, match=r"dan_finalize failed \(-2\): missing tensor 'fcHidden2VT.bias'"):
        net.load_state_dict(missing)
    net.close()
    bad = dict(sd)
    bad["conv1D_layers.2.weight"] = bad["conv1D_layers.2.weight"][:, :8]
    net = DanNet(_cfg(), max_batch=MAX_BATCH, chunk_sites=CHUNK)
    with pytest.raises(RuntimeError, match=r"dan_finalize failed \(-3\): tensor 'conv1D_layers.2.weight' has shape \(16,8,1,3,\) but the "
                                           r"configuration needs \(16,16,1,3,\)"):
        net.load_state_dict(bad)
    net.close()
    net = _open(sd)
    assert _sync(net, batch) == first[0]
    net.close()


def test_async_path_and_tap_made_late(sd, batch, first):
    net = _open(sd)
    for _ in range(3):
        assert _sync(net, batch) == first[0]
    net.handle.set_tap(2)                          # the tap buffer is allocated here, behind the workspaces
    assert _sync(net, batch) == first[0]
    assert _async(net, batch) == first[0]          # streams, slots and events are made here
    assert _sync(net, batch) == first[0]
    net.handle.set_tap(-1)
    assert _async(net, batch) == first[0]
    net.close()


@pytest.mark.parametrize("precision", [0, 1, 2])
def test_tap_reads_back_the_same_bytes(sd, batch, first, precision):
    net = _open(sd, precision=precision)
    net.handle.set_tap(2)
    taps = []
    for _ in range(2):
        assert _sync(net, batch) == first[precision]
        assert net.handle.query("tap_sites") == 1                          # the last chunk
        taps.append(net.handle.read_buffer("tap", NET["reads"] * NET["length"] * 128).tobytes())
    assert len(taps[0]) == NET["reads"] * NET["length"] * 128 * 4 and any(taps[0]) and taps[0] == taps[1]
    net.close()


def _counts(net):
    return {k: net.handle.kernel_stats(k)[0] for k in ("row_map", "conv_segment", "pool", "highway", "fc")}


# The schedule of the 5-site call: 3 chunks x 2 segments; per chunk one read-mean behind the pool layer and one
# final pool, one highway; one FC stack per macro-batch (2); with skip_empty_rows one row map per chunk.  In-segment pooling (form 2,
# fp32) launches no pool kernel.  The same counts were read from a library built from the commit before the handle moved onto
# device_buffer.h (tools/forward_ab.py records them per case).
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_launch_counts_with_separate_pool_kernels(sd, batch, first, precision):
    net = _open(sd, precision=precision)
    net.handle.set_pool_form(1)
    net.handle.profile(True)
    assert _sync(net, batch) == first[precision]
    assert _counts(net) == {"row_map": 0, "conv_segment": 6, "pool": 6, "highway": 3, "fc": 2}
    net.handle.profile(True)                       # collects and resets
    assert _async(net, batch) == first[precision]
    assert _counts(net) == {"row_map": 0, "conv_segment": 6, "pool": 6, "highway": 3, "fc": 2}
    net.close()


def test_launch_counts_with_skip_empty_rows(sd, batch, first):
    net = _open(sd, skip_empty_rows=True)
    net.handle.set_pool_form(1)
    net.handle.profile(True)
    assert _sync(net, batch) == first[0]
    assert _counts(net) == {"row_map": 3, "conv_segment": 6, "pool": 6, "highway": 3, "fc": 2}
    net.close()


def test_launch_counts_with_in_segment_pooling(sd, batch, first):
    net = _open(sd)
    net.handle.set_pool_form(2)
    net.handle.profile(True)
    assert _sync(net, batch) == first[0]
    assert net.handle.query("pool_form") == 2
    assert _counts(net) == {"row_map": 0, "conv_segment": 6, "pool": 0, "highway": 3, "fc": 2}
    net.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_split_window_does_not_depend_on_the_chunking(precision):
    """Window 216 (> 208 columns): every read as two units and y alternating between its two buffers from segment to segment."""
    over = dict(reads=2, length=216, precision=precision)
    wsd = synth.random_state_dict(_cfg(**over), seed=13)
    wbatch = synth.make_sites(SITES, reads=2, length=216, seed=14)
    got = []
    for chunk in (CHUNK, 1):
        net = _open(wsd, chunk=chunk, **over)
        assert net.handle.query("chunk_sites") == chunk
        got.append(_sync(net, wbatch))
        assert _async(net, wbatch) == got[-1]
        net.close()
    assert got[0] == got[1] and any(got[0])
