"""The zlib stream inflate's CPU twin (``zi_inflate_host``: the text of csrc/zinflate.h that ``zi_inflate_kernel`` runs, ring
included, with one lane) against Python's ``zlib`` on the grid of tests/zinflate_cases.py; damaged streams are statuses and
leave every byte outside their slot alone; plus the header, the exports and the ctypes binding of the ``zi_*`` entries."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import pileup_gpu, zinflate
from tests import zinflate_cases as G

HEADER = os.path.join(ROOT, "include", "dl4vc_chunks.h")


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not pileup_gpu.available():
        import __graft_entry__ as g
        g.build()
    return zinflate.load_library()


def GOOD():
    """A good stream that crosses a half boundary, to stand beside the damaged ones."""
    return next(c for c in G.valid_cases() if c.name.startswith("pileup-like x 32769 at alignment 13"))


def test_the_grid_is_what_it_says():
    """Every length, content, compressor and alignment occurs, the references are zlib's, and the streams hold the block types and
    distances the ring is there for."""
    cases = G.valid_cases()
    names = " | ".join(c.name for c in cases)
    for n in G.LENGTHS:
        assert " x %d" % n in names
    for word in ("zeros", "one byte", "period 3 x", "period 32768", "random", "pileup-like", "zlib 0", "zlib 1", "zlib 4", "zlib 9", "zd fixed",
                 "zd dynamic", "hand: stored", "hand: match", "hand: distance", "raw chunk"):
        assert word in names, word
    assert {c.align for c in cases} == set(range(16))
    for c in cases:
        if not c.raw:
            assert zlib.decompress(c.stream) == c.data, c.name
    assert max(c.out_len for c in cases) == 991720


def test_grid_equals_zlib_and_leaves_the_rest_alone():
    cases = G.valid_cases()
    out, out_off, status = G.run(cases)
    G.assert_valid(cases, out, out_off, status)


def test_slots_in_another_order_and_one_stream_at_a_time():
    """The bytes of a slot depend on its stream alone: slots laid out in reversed order, and each of a few streams on its own."""
    cases = G.valid_cases()[::5]
    out, out_off, status = G.run(cases, gap=3, order=list(range(len(cases)))[::-1])
    G.assert_valid(cases, out, out_off, status)
    for c in cases[:6]:
        out, out_off, status = G.run([c], gap=1)
        G.assert_valid([c], out, out_off, status)


@pytest.mark.parametrize("bad", G.damaged_cases(), ids=lambda c: c.name)
def test_damaged_stream_is_a_status(bad):
    """Between two good streams: the damaged one gets a non-zero status, its neighbours inflate, nothing outside the slots moves."""
    assert bad.name == "1 trailing byte" or G.zlib_refuses(bad)
    good = GOOD()
    cases = [good, bad, good]
    out, out_off, status = G.run(cases)
    print(bad.name, "->", zinflate.status_text(status[1]))
    assert status[1] != 0 and zinflate.status_text(status[1]) not in ("ok", "unknown status")
    for k in (0, 2):
        assert status[k] == 0 and out[out_off[k]:out_off[k] + good.out_len].tobytes() == good.data
    assert G.outside_untouched(cases, out, out_off)


def test_damage_has_the_status_that_names_it():
    want = {"CM 9": "ZI_BAD_ZLIB_HEADER", "CINFO 8": "ZI_BAD_ZLIB_HEADER", "bad FCHECK": "ZI_BAD_ZLIB_HEADER", "FDICT set": "ZI_BAD_ZLIB_HEADER",
            "flipped Adler byte": "ZI_ADLER_MISMATCH", "truncated to 1 bytes": "ZI_INPUT_EXHAUSTED", "truncated to 5 bytes": "ZI_INPUT_EXHAUSTED",
            "truncated mid-body": "ZI_INPUT_EXHAUSTED", "1 trailing byte": "ZI_TRAILING_INPUT",
            "expected length one more": "ZI_OUTPUT_SHORT_OF_LENGTH", "expected length one less": "ZI_OUTPUT_EXCEEDS_LENGTH",
            "distance before the start": "ZI_DISTANCE_BEFORE_START", "BTYPE 3": "ZI_BAD_BLOCK_TYPE",
            "BTYPE 3 after a flushed half": "ZI_BAD_BLOCK_TYPE", "raw chunk one byte short": "ZI_RAW_SIZE_MISMATCH",
            "raw chunk one byte long": "ZI_RAW_SIZE_MISMATCH"}
    cases = [c for c in G.damaged_cases() if c.name in want]
    assert len(cases) == len(want)
    _out, _off, status = G.run(cases)
    assert {c.name: int(s) for c, s in zip(cases, status)} == {k: zinflate.STATUS[v] for k, v in want.items()}


def test_ranges_and_slots_outside_the_buffers_are_statuses():
    c = GOOD()
    streams, off, length, out, out_off, out_len, raw = G.layout([c] * 4)
    off[1] = streams.size - 10                               # runs past the input
    out_off[2] = out.size - c.out_len + 1                    # runs past the output
    length[3] = 1 << 33
    status = zinflate.inflate_streams(streams, off, length, out, out_off, out_len, raw)
    assert list(status) == [0, zinflate.ZI_BAD_RANGE, zinflate.ZI_BAD_SLOT, zinflate.ZI_BAD_RANGE]
    assert out[out_off[0]:out_off[0] + c.out_len].tobytes() == c.data
    out[out_off[0]:out_off[0] + c.out_len] = G.FILL
    assert (out == G.FILL).all()
    with pytest.raises(ValueError):
        zinflate.inflate_streams(streams, off, length[:2], out, out_off, out_len)
    assert len(zinflate.inflate_streams(b"", [], [], np.zeros(0, np.uint8), [], [])) == 0


def test_header_exports_and_binding_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(zi_[a-z_]+)\s*\(", text))
    assert declared == set(zinflate.ZI_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("zi_")}
    assert exported == declared
    codes = {k: int(v) for k, v in re.findall(r"#define (ZI_[A-Z_0-9]+) (\d+)", text)}
    assert codes.pop("ZI_MAX_OUTPUT") == zinflate.ZI_MAX_OUTPUT
    assert codes == zinflate.STATUS
    # the shared causes keep the numbers of dl4vc_bgzf.h
    bz = dict(re.findall(r"#define (BZ_[A-Z_0-9]+) (\d+)", open(os.path.join(ROOT, "include", "dl4vc_bgzf.h")).read()))
    for zi_name, bz_name in (("ZI_BAD_BLOCK_TYPE", "BZ_BAD_BLOCK_TYPE"), ("ZI_BAD_STORED_LEN", "BZ_BAD_STORED_LEN"),
                             ("ZI_BAD_CODE_LENGTHS", "BZ_BAD_CODE_LENGTHS"), ("ZI_BAD_SYMBOL", "BZ_BAD_SYMBOL"),
                             ("ZI_DISTANCE_BEFORE_START", "BZ_DISTANCE_BEFORE_START"), ("ZI_OUTPUT_EXCEEDS_LENGTH", "BZ_OUTPUT_EXCEEDS_ISIZE"),
                             ("ZI_OUTPUT_SHORT_OF_LENGTH", "BZ_OUTPUT_SHORT_OF_ISIZE"), ("ZI_INPUT_EXHAUSTED", "BZ_INPUT_EXHAUSTED"),
                             ("ZI_TRAILING_INPUT", "BZ_TRAILING_INPUT"), ("ZI_BAD_SLOT", "BZ_BAD_SLOT")):
        assert codes[zi_name] == int(bz[bz_name])
    for name, code in zinflate.STATUS.items():
        assert zinflate.status_text(code) != "unknown status", name
    # pointers bind as void*, integers as themselves, in the header's order
    import ctypes as C
    for fn, n_params in (("zi_inflate", 12), ("zi_inflate_host", 11)):
        decl = re.search(r"int %s\((.*?)\);" % fn, text, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        argtypes = getattr(lib, fn).argtypes
        assert len(params) == len(argtypes) == n_params
        for p, t in zip(params, argtypes):
            assert t is (C.c_void_p if "*" in p else C.c_uint64 if p.startswith("uint64_t") else C.c_int64 if p.startswith("int64_t")
                         else C.c_int), p
