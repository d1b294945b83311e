"""Dynamic Huffman codes in the zlib compressor's CPU twin (``zd_deflate_host_flags`` with ``ZD_DYNAMIC``, the text of
csrc/zdeflate.h that ``zd_deflate_dyn_kernel`` runs): every stream inflates to its input and is never larger than in fixed
codes, fixed mode keeps its bytes, the sizes the feature is for, the code construction on its own (``zd_code_lengths_host``)
against a ``heapq`` Huffman code, the contents at which it takes another path, ``hdf5io.ChunkWriter(codes="dynamic")``, the C ABI
and the converter's refusal."""
import ctypes as C
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import candgen, hdf5io, loader, pileup_gpu
from dl4vc_amd.hdf5_schema import record_dtype
from tests import zdeflate_cases as ZC
from tests import zdeflate_dynamic_cases as DC

HEADER = os.path.join(ROOT, "include", "dl4vc_pileup_gpu.h")


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not (pileup_gpu.available() and loader.available() and os.path.isfile(candgen.LIB_PATH)):
        import __graft_entry__ as g
        g.build()
    return pileup_gpu.load_library()


def dyn(data, seg=pileup_gpu.ZD_DEFAULT_SEGMENT):
    return pileup_gpu.zd_deflate_host(data, seg, codes="dynamic")


def test_grid_round_trip_never_larger_and_fixed_bytes_unchanged():
    smaller = 0
    for name, seg, data in ZC.grid() + DC.special_cases():
        fixed, f_adler, _f_store = pileup_gpu.zd_deflate_host(data, seg)
        stream, adler, store = dyn(data, seg)
        assert zlib.decompress(stream) == data, name
        assert len(stream) <= pileup_gpu.zd_bound(len(data), seg), name
        assert adler == f_adler == zlib.adler32(data) and stream[:2] == b"\x78\x01", name
        assert store == (len(stream) >= len(data)), name
        assert len(stream) <= len(fixed), (name, len(stream), len(fixed))
        smaller += len(stream) < len(fixed)
        assert pileup_gpu.zd_deflate_host_flags(data, seg, 0)[0] == fixed, name
        if name.startswith("random") and len(data) >= 257:
            assert store and stream == fixed, name             # stored segments: the same bytes
    assert smaller > 20
    assert pileup_gpu.zd_deflate_host(b"abc", codes="fixed")[0] == pileup_gpu.zd_deflate_host(b"abc")[0]
    with pytest.raises(ValueError, match="codes"):
        pileup_gpu.zd_deflate_host(b"abc", codes="best")
    with pytest.raises(RuntimeError, match="ZD_DYNAMIC"):
        pileup_gpu.zd_deflate_host_flags(b"abc", flags=pileup_gpu.ZD_REVERSED)


def test_size_of_pileup_like_rows():
    """The issue's model of this encoder gives 0.71 of the fixed stream and 1.16 of zlib level 4; the bars leave room for another
    run-length rule in the header."""
    data = ZC.pileup_like(3 * 16384 + 1)
    fixed, stream, z4 = pileup_gpu.zd_deflate_host(data, 16384)[0], dyn(data, 16384)[0], zlib.compress(data, 4)
    print("pileup-like x 49 153: fixed %d, dynamic %d, zlib level 4 %d" % (len(fixed), len(stream), len(z4)))
    assert len(stream) <= 0.8 * len(fixed)
    assert len(stream) <= 1.25 * len(z4)


def test_size_of_a_chunk_of_zero_records():
    n = 8 * record_dtype().itemsize
    assert n == 991720
    stream, _adler, store = dyn(bytes(n))
    assert zlib.decompress(stream) == bytes(n) and not store
    print("991 720 zero bytes -> %d" % len(stream))
    assert len(stream) < 3072


def test_size_of_encoder_records(tmp_path):
    """The records of tests/test_zdeflate_host.py::test_pileup_records_compress_and_round_trip, built the same way: the content the
    converter compresses.  Measured: 770 845 bytes -> fixed 52 952, dynamic 40 701, zlib level 4 34 014."""
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
    fixed, stream = pileup_gpu.zd_deflate_host(raw)[0], dyn(raw)[0]
    print("encoder records: %d -> fixed %d, dynamic %d, zlib level 4 %d" % (len(raw), len(fixed), len(stream), len(zlib.compress(raw, 4))))
    assert zlib.decompress(stream) == raw
    assert len(stream) < len(fixed)


# ---- the code construction on its own ------------------------------------------------------------------------------------------

def check_code(freq, limit):
    """Lengths within the limit, every used symbol coded, Kraft sum exactly 1 (two codes of length 1 where fewer than two symbols
    are used), and the ``heapq`` optimum's cost where its depth fits the limit.  -> (cost, the optimum's cost and depth)"""
    freq = [int(f) for f in freq]
    lens = pileup_gpu.zd_code_lengths(freq, limit).tolist()
    used = [s for s, f in enumerate(freq) if f]
    assert len(lens) == len(freq) and max(lens) <= limit
    assert all(lens[s] for s in used)
    if len(used) < 2:
        assert sorted(l for l in lens if l) == [1, 1]
    else:
        assert all((l > 0) == (f > 0) for l, f in zip(lens, freq))
    assert sum(1 << (limit - l) for l in lens if l) == 1 << limit
    cost = sum(f * l for f, l in zip(freq, lens))
    best, depth = DC.huffman(freq)
    assert cost >= best
    if depth <= limit:
        assert cost == best, (cost, best, depth)
    return cost, best, depth


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def test_code_lengths_of_0_1_2_and_286_used_symbols():
    for limit, n in ((15, 286), (7, 19), (15, 30)):
        check_code([0] * n, limit)
        for only in (0, 1, 2, n - 1):
            f = [0] * n
            f[only] = 7
            check_code(f, limit)
        f = [0] * n
        f[3], f[n - 1] = 1, 40000
        check_code(f, limit)
    rng = np.random.default_rng(1)
    _cost, _best, depth = check_code(rng.integers(1, 200, 286), 15)
    assert depth <= 15
    check_code([1] * 286, 15)
    check_code([1] * 256 + [0] * 30, 15)                  # a complete code of 8 bits
    check_code([229] * 286, 15)                           # the largest sum the entry takes: 65 494
    for bad in ([1], [1] * 287):
        with pytest.raises(RuntimeError, match="2..286 symbols"):
            pileup_gpu.zd_code_lengths(bad, 15)
    with pytest.raises(RuntimeError, match="65535"):
        pileup_gpu.zd_code_lengths([40000, 40000], 15)
    with pytest.raises(RuntimeError, match="limit"):
        pileup_gpu.zd_code_lengths([1] * 19, 4)             # 16 codes of 4 bits do not hold 19 symbols


def test_code_lengths_are_cut_at_the_limit():
    """Fibonacci counts make the Huffman code a chain: 20 symbols are 19 deep, 12 symbols 11 -- every optimal code, as the joins are
    forced -- so the limits of 15 and 7 bits cut them."""
    for n, limit in ((20, 15), (12, 7)):
        cost, best, depth = check_code(fib(n), limit)
        assert depth == n - 1 > limit and cost > best
        shuffled = np.random.default_rng(n).permutation(fib(n))
        assert check_code(shuffled, limit)[0] == cost           # the symbols' order does not matter to the cost
        padded = [0, 0] + fib(n) + [0]
        check_code(padded, limit)
    # one level too deep, and the deepest the 286 symbols' counts allow within 65 535 (22 Fibonacci counts: 21 deep)
    check_code(fib(17), 15)
    check_code(fib(9), 7)
    check_code(fib(22) + [1] * 200, 15)


def test_code_lengths_of_seeded_random_histograms():
    rng = np.random.default_rng(2024)
    cut = fit = 0
    for k in range(200):
        limit, top = ((15, 286), (7, 19), (15, 30))[k % 3]
        n = int(rng.integers(2, top + 1))
        kind = k % 4
        if kind == 0:
            f = rng.integers(0, 300, n)
        elif kind == 1:                                        # geometric: deep codes
            f = (rng.random(n) * 1.5 ** rng.integers(0, 24, n)).astype(np.int64)
        elif kind == 2:                                        # mostly unused
            f = rng.integers(0, 50, n) * (rng.random(n) < 0.2)
        else:                                                  # many equal counts
            f = rng.integers(1, 4, n)
        f = np.minimum(f, 65535 // n)
        _cost, _best, depth = check_code(f, limit)
        cut += depth > limit
        fit += depth <= limit
    assert cut >= 10 and fit >= 100


# ---- contents at which the encoder takes another path ----------------------------------------------------------------------------

def test_the_python_parse_is_the_compressors():
    """What the two tests below say about a segment's histograms comes from tests/zdeflate_dynamic_cases.parse_histograms: it
    gives the fixed block's size to the byte."""
    for data in (DC.fibonacci_bytes(), DC.fibonacci_run_bytes(), DC.de_bruijn_bytes(), ZC.pileup_like(16384)):
        assert DC.fixed_segment_bytes(data) == len(pileup_gpu.zd_deflate_host(data, 32768)[0]) - 6


def test_an_over_long_literal_code_through_a_stream():
    """A segment whose literal / length code is deeper than 15 bits without the limit: asserted first, with the ``heapq`` code
    over the segment's own histogram.

    Byte values with the counts 1, 1, 2, ... 1 597 in a shuffled order cannot be that segment.  Such bytes have 2.4 bits of
    entropy, so 4 180 of them repeat 4-grams whatever their order (counted: with every 4-gram distinct the 1 597 bytes of the
    commonest value need 4 721 4-grams, there are 4 177), the parse finds about 520 matches, and their length symbols and the
    literals they take away leave a code of depth 11 (seeds 8..13: 11 or 12).  That stream is checked for what it is; the code
    deeper than 15 comes from ``fibonacci_run_bytes``, where the Fibonacci counts lie on the length symbols and the parse keeps
    them: depth 17 in every optimal code."""
    data = DC.fibonacci_bytes()
    counts = np.bincount(np.frombuffer(data, np.uint8)).tolist()
    assert counts == fib(17) and DC.huffman(counts)[1] == 16
    ll, dd, _extra = DC.parse_histograms(data)
    print("shuffled Fibonacci bytes: %d matches, depth of the literal / length code %d" % (sum(dd), DC.huffman(ll)[1]))
    stream, _adler, store = dyn(data)
    assert zlib.decompress(stream) == data and not store
    assert len(stream) < len(pileup_gpu.zd_deflate_host(data)[0])

    data = DC.fibonacci_run_bytes()
    ll, dd, _extra = DC.parse_histograms(data)
    assert sorted(c for c in ll[256:] if c) == fib(17) and sum(ll[:256]) == sum(dd) == 4179
    depth = DC.huffman(ll)[1]
    assert depth > 15, depth
    assert len(data) <= 32768
    stream, _adler, store = dyn(data, 32768)
    assert zlib.decompress(stream) == data and not store
    fixed = pileup_gpu.zd_deflate_host(data, 32768)[0]
    print("Fibonacci runs: depth %d, fixed %d, dynamic %d" % (depth, len(fixed), len(stream)))
    assert len(stream) < len(fixed)
    assert inflate_as_bgzf(data, stream) == data


def inflate_as_bgzf(data, stream):
    """The stream's DEFLATE blocks as one BGZF block through the project's own inflate (``bz_inflate_host``)."""
    out = np.zeros(len(data) + 1, np.uint8)
    assert candgen.inflate_blocks(DC.bgzf_block(data, stream), [0], out, [0]) == [0]
    return out[:len(data)].tobytes()


def test_a_segment_without_a_match():
    data = DC.de_bruijn_bytes()
    assert len(data) == 84 and len(set(data)) == 3
    _ll, dd, _extra = DC.parse_histograms(data)
    assert sum(dd) == 0                                    # the distance code: two codes of length 1, neither used
    stream, _adler, _store = dyn(data)
    fixed = pileup_gpu.zd_deflate_host(data)[0]
    assert len(stream) < len(fixed)                        # dynamic was chosen
    assert zlib.decompress(stream) == data
    assert inflate_as_bgzf(data, stream) == data
    # several segments, the last one short, through the project's inflate as well
    data = ZC.pileup_like(3 * 16384 + 1)
    assert inflate_as_bgzf(data, dyn(data)[0]) == data


def test_flat_content_stays_in_fixed_codes():
    data = DC.permutation_bytes()
    assert sorted(data) == list(range(256))
    assert dyn(data)[0] == pileup_gpu.zd_deflate_host(data)[0]
    # (256 literals of 8 and 9 bits: that segment is stored in both modes.)  A block that fixed codes do hold: 40 literals of 8 bits
    # and the end-of-block symbol are fewer bits than the dynamic header and 6-bit codes
    data = bytes(range(40))
    fixed = pileup_gpu.zd_deflate_host(data)[0]
    assert dyn(data)[0] == fixed and fixed[2] & 7 == 0b011 and len(fixed) == 6 + 42        # BFINAL 1, BTYPE 01; 3 + 40 * 8 + 7 bits


# ---- the chunk writer, the ABI, the converter ------------------------------------------------------------------------------------

def test_chunk_writer_in_dynamic_codes(tmp_path):
    """13 + 11 records: the tail of 5 is carried into the second step's first chunk; three chunks from the CPU twin in dynamic
    codes read back through libhdf5's filter and through the native loader."""
    from tests.test_chunk_writer import CHUNK, DT, make_records, native_planes, read_all
    parts = [make_records(13, 13), make_records(11, 21)]
    recs = np.concatenate(parts)
    a, b, c = (str(tmp_path / n) for n in ("host.hdf", "dynamic.hdf", "fixed.hdf"))
    hdf5io.write_candidates(a, parts[0], chunk=CHUNK)
    hdf5io.append_candidates(a, parts[1])
    for path, codes in ((b, "dynamic"), (c, "fixed")):
        with hdf5io.ChunkWriter(path, DT, chunk=CHUNK, codes=codes) as w:
            for p in parts:
                w.append_records(p)
        assert w.host_chunks == 3 and w.codes == codes
    assert read_all(b).tobytes() == recs.tobytes() == read_all(a).tobytes()
    assert hdf5io.dataset_layout(b) == hdf5io.dataset_layout(a)
    assert os.path.getsize(b) < os.path.getsize(c)
    for x, y in zip(native_planes(a), native_planes(b)):
        for u, v in zip(x, y):
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v
    with pytest.raises(ValueError, match="codes"):
        hdf5io.ChunkWriter(str(tmp_path / "x.hdf"), DT, chunk=CHUNK, codes="static")


def test_header_exports_and_binding_agree_on_the_new_entries(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split()}
    for name, n_params in (("zd_deflate_host_flags", 9), ("zd_code_lengths_host", 4), ("pg_set_compress_codes", 2)):
        decl = re.search(r"int %s\((.*?)\);" % name, text, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        argtypes = getattr(lib, name).argtypes
        assert len(params) == len(argtypes) == n_params, name
        for p, t in zip(params, argtypes):
            if "*" in p:
                assert t is C.c_void_p or t in (C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)), (name, p)
            else:
                want = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "int": C.c_int}[p.split()[0]]
                assert t is want, (name, p)
        assert name in exported and name in pileup_gpu.SYMBOLS + pileup_gpu.ZD_SYMBOLS
    assert int(re.search(r"#define ZD_DYNAMIC (\d+)", text).group(1)) == pileup_gpu.ZD_DYNAMIC == 4
    assert pileup_gpu.COMPRESS_CODES == {"fixed": 0, "dynamic": 1}
    body = re.search(r"typedef struct \{([^}]*)\} pg_stats;", text, flags=re.S).group(1)
    fields = []
    for decl in re.findall(r"(double|int64_t)\s+([a-z_, ]+);", body):
        fields += [(n.strip(), decl[0]) for n in decl[1].split(",")]
    assert fields[-3:] == [("fixed_segments", "int64_t"), ("dynamic_segments", "int64_t"), ("stored_segments", "int64_t")]
    assert fields == [(n, "double" if t is C.c_double else "int64_t") for n, t in pileup_gpu.Stats._fields_]
    decl = re.search(r"int pg_compress_records_device\((.*?)\);", text, flags=re.S).group(1)
    assert len(decl.split(",")) == len(lib.pg_compress_records_device.argtypes) == 15
    assert lib.zd_deflate.argtypes == [C.c_void_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64] + [C.c_void_p] * 5


def test_compress_codes_is_refused_without_the_device_compressor():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convert_bam_single_reads as conv
    from dl4vc_amd import pileup_encoder as PE
    base = ["--input", "x.bam", "--fp_vcf", "x.vcf", "--output", "x.hdf", "--save-q-scores", "--save-strand", "--compress-codes", "dynamic"]
    for more in ([], ["--pileup-device", "gpu"]):
        with pytest.raises(SystemExit, match="give --compress-device gpu as well"):
            conv.main(base + more)
    with pytest.raises(ValueError, match="needs compress_device='gpu'"):
        PE.encode_locations("x.bam", "x.fa", [], PE.EncoderOptions(), device="gpu", compress_codes="dynamic")
    with pytest.raises(ValueError, match="compress_codes"):
        PE.encode_locations("x.bam", "x.fa", [], PE.EncoderOptions(), device="gpu", compress_device="gpu", compress_codes="best")
    for script, letters in (("call_variants.sh", "dzcyh"), (os.path.join("tools", "make_training_data.sh"), "cyh")):
        text = open(os.path.join(ROOT, script)).read()
        assert letters + '"' in text and "[-c [-y]]" in text and '--compress-codes "$CODES"' in text, script
