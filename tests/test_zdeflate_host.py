"""The zlib compressor's CPU twin (``zd_deflate_host``, the text of csrc/zdeflate.h that the GPU kernel runs) against Python's
``zlib``: every stream of the grid inflates to its input, stays within ``zd_bound`` and carries the right Adler-32; plus the
header, the exports and the ctypes binding of the ``zd_*`` entries and of the grown ``pg_stats``."""
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import pileup_gpu
from dl4vc_amd.hdf5_schema import record_dtype
from tests import zdeflate_cases as ZC

HEADER = os.path.join(ROOT, "include", "dl4vc_pileup_gpu.h")


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not pileup_gpu.available():
        import __graft_entry__ as g
        g.build()
    return pileup_gpu.load_library()


def test_grid_inflates_to_its_input_within_the_bound():
    stored = 0
    for name, seg, data in ZC.grid():
        stream, adler, store = pileup_gpu.zd_deflate_host(data, seg)
        assert zlib.decompress(stream) == data, name
        assert len(stream) <= pileup_gpu.zd_bound(len(data), seg), name
        assert adler == zlib.adler32(data) and stream[:2] == b"\x78\x01", name
        assert store == (len(stream) >= len(data)), name
        stored += store
        if name.startswith("random") and len(data) >= 257:
            assert store, name                         # incompressible: flagged, and still within the bound (above)
        if name.startswith(("zeros", "one byte", "period 3")) and len(data) >= 257:
            assert not store and len(stream) < len(data) // 4, (name, len(stream))
    assert stored


def test_a_chunk_of_zero_records_is_matches_not_stored_bytes():
    """8 records of the production layout, all zero: one length-258 match per 258 bytes at 13 bits each in fixed codes is
    3 844 matches = 6.3 KB; with the joins of the 61 segments the stream must be under 8 192 bytes (zlib itself: about 1 KB).  A
    store-everything or literal-only compressor does not pass."""
    n = 8 * record_dtype().itemsize
    assert n == 991720
    stream, adler, store = pileup_gpu.zd_deflate_host(bytes(n))
    assert zlib.decompress(stream) == bytes(n) and not store
    print("991 720 zero bytes -> %d" % len(stream))
    assert len(stream) < 8192


def test_pileup_records_compress_and_round_trip(tmp_path):
    """Records of the native encoder on a tests/pileup_cases.py case: the content the converter compresses."""
    from dl4vc_amd import pileup_encoder as PE
    from tests import pileup_cases as PC
    ref = PC.make_ref(3000, 3)
    reads = [PC.read(ref, s, ["100M", "50M1X49M", "40M2I58M", "30M3D67M"][i % 4], "r%d" % i, PC.FREV if i % 2 else 0, 10 + i % 30)
             for i, s in enumerate(range(100, 2700, 5))]
    bam, fa = PC.write_case(tmp_path, PC.Case("zd", [("chr20", ref)], reads, [], w=100, max_reads=50))
    locs = [PE.Location("chr20", p, "chr20:%d" % p, 2, "chr20\t%d\t.\tA\tC" % p) for p in range(300, 2500, 97)]
    recs, errors = PE.encode_locations(bam, fa, locs, PE.EncoderOptions(100, 50, 10, 50), native=True)
    assert len(recs) == len(locs) and int(recs["num_reads"].min()) >= 10
    raw = np.ascontiguousarray(recs).tobytes()
    for seg in (ZC.SEGMENT, pileup_gpu.ZD_DEFAULT_SEGMENT):
        stream, _adler, store = pileup_gpu.zd_deflate_host(raw, seg)
        assert zlib.decompress(stream) == raw and not store
        print("segment %d: %d -> %d (zlib level 4: %d)" % (seg, len(raw), len(stream), len(zlib.compress(raw, 4))))
        assert len(stream) < len(raw) // 2


def test_empty_input_and_refused_arguments():
    stream, adler, store = pileup_gpu.zd_deflate_host(b"")
    assert zlib.decompress(stream) == b"" and adler == 1 and store
    for seg in (0, 1023, 32769):
        with pytest.raises(RuntimeError, match="segment"):
            pileup_gpu.zd_bound(10, seg)
        with pytest.raises(RuntimeError, match="segment"):
            pileup_gpu.zd_deflate_host(b"abc", seg)
    with pytest.raises(RuntimeError, match="2\\^31"):
        pileup_gpu.zd_bound((1 << 31) + 1)


def test_header_exports_and_binding_agree_on_the_compressor(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(zd_[a-z_]+)\s*\(", text))
    assert declared == set(pileup_gpu.ZD_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("zd_")}
    assert exported == declared
    assert "pg_compress_records_device" in pileup_gpu.SYMBOLS
    for name in ("ZD_MIN_SEGMENT", "ZD_MAX_SEGMENT", "ZD_DEFAULT_SEGMENT", "ZD_REVERSED", "ZD_RAW_ON_STORE"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(pileup_gpu, name)
    # pg_stats: the binding's fields, in the header's order and types
    body = re.search(r"typedef struct \{([^}]*)\} pg_stats;", text, flags=re.S).group(1)
    fields = []
    for decl in re.findall(r"(double|int64_t)\s+([a-z_, ]+);", body):
        fields += [(n.strip(), decl[0]) for n in decl[1].split(",")]
    import ctypes as C
    assert fields == [(n, "double" if t is C.c_double else "int64_t") for n, t in pileup_gpu.Stats._fields_]
    # pg_compress_records_device: pointers bind as void*, integers as themselves, in the header's order
    decl = re.search(r"int pg_compress_records_device\((.*?)\);", text, flags=re.S).group(1)
    params = [p.strip() for p in decl.split(",")]
    assert len(params) == len(lib.pg_compress_records_device.argtypes) == 15
    for p, t in zip(params, lib.pg_compress_records_device.argtypes):
        if "**" in p:
            assert t is C.POINTER(C.c_void_p), p
        else:
            assert t is (C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int32), p
