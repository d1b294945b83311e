"""The zlib stream inflate kernel on the MI355X (``zi_inflate``): the grid of tests/zinflate_cases.py with the assertions of
tests/test_zinflate_host.py (the same text runs there on the CPU with one lane, and under sanitizers by tools/asan_zinflate.sh):
bytes and statuses equal the CPU twin's, into 0xAB-filled buffers; one launch that mixes deflated, raw and damaged streams; the
same launch twice and with the slots in reversed order; chunks the device compressor wrote."""
import zlib

import numpy as np
import pytest

from dl4vc_amd import pileup_gpu, zinflate
from tests import zinflate_cases as G

pytestmark = pytest.mark.gpu


def test_grid_equals_the_cpu_twin_and_zlib():
    cases = G.valid_cases()
    out, out_off, status = G.run(cases, 0)
    G.assert_valid(cases, out, out_off, status)
    host, host_off, host_status = G.run(cases)
    assert out_off == host_off and (status == host_status).all() and (out == host).all()


def test_one_launch_of_deflated_raw_and_damaged_streams_twice_and_reversed():
    """Good slots equal zlib whatever stands beside them; the damaged ones have the CPU twin's status; no byte outside the slots
    moves; a second launch and one with the slots laid out in reversed order give the same bytes in every good slot."""
    good = G.valid_cases()[1::4] + [c for c in G.valid_cases() if c.raw]
    bad = G.damaged_cases()
    cases = [c for pair in zip(good, bad * (len(good) // len(bad) + 1)) for c in pair]
    runs = [G.run(cases, 0, gap=3), G.run(cases, 0, gap=3), G.run(cases, 0, gap=21, order=list(range(len(cases)))[::-1])]
    _host, _off, host_status = G.run(cases, gap=3)
    assert any(c.raw and c.data is not None for c in cases) and any(c.raw and c.data is None for c in cases)
    for out, out_off, status in runs:
        assert (status == host_status).all()
        assert G.outside_untouched(cases, out, out_off)
        for c, o, s in zip(cases, out_off, status):
            if c.data is None:
                assert s != 0, c.name
            else:
                assert s == 0 and out[o:o + c.out_len].tobytes() == c.data, c.name


@pytest.mark.parametrize("codes", ["fixed", "dynamic"])
def test_chunks_the_device_compressor_wrote(codes):
    """Three chunks of 123 400 pileup-like bytes through ``zd_deflate`` on the device (the converter's compressor), then through
    the device inflate: the bytes that went in."""
    import torch
    n, chunk = 3, 123400
    data = np.frombuffer(G._PILEUP[:n * chunk], np.uint8)
    src = torch.from_numpy(data.copy()).cuda()
    cap = n * pileup_gpu.zd_bound(chunk)
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    offs, sizes, _adlers, store = pileup_gpu.zd_deflate_device(src.data_ptr(), chunk, n, dst.data_ptr(), cap,
                                                               flags=pileup_gpu.ZD_DYNAMIC if codes == "dynamic" else 0)
    torch.cuda.synchronize()
    comp = dst.cpu().numpy()
    assert not store.any() and int(sizes.max()) < chunk // 2
    assert zlib.decompress(comp[int(offs[1]):int(offs[1] + sizes[1])].tobytes()) == data[chunk:2 * chunk].tobytes()
    out = np.full(n * chunk + 32, G.FILL, np.uint8)
    status = zinflate.inflate_streams(comp, offs, sizes, out, [16 + i * chunk for i in range(n)], [chunk] * n, device=0)
    assert (status == 0).all() and (out[16:16 + n * chunk] == data).all()
    assert (out[:16] == G.FILL).all() and (out[-16:] == G.FILL).all()
