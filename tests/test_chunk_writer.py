"""``hdf5io.ChunkWriter``: chunks compressed by the compressor's CPU twin and written past the HDF5 filter read back as the
records ``write_candidates`` stores -- through ``CandidateFile`` (libhdf5's own deflate filter) and through the native loader --
with the same chunk size and filter pipeline; tails are carried across steps, a misaligned chunk is never written, and the
converter refuses ``--compress-device gpu`` without the GPU encoder."""
import os
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import hdf5io, loader, pileup_gpu
from dl4vc_amd.hdf5_schema import blob_dtype, record_dtype

DT = record_dtype(50, 201)
CHUNK = 8


@pytest.fixture(scope="module", autouse=True)
def built():
    if not (pileup_gpu.available() and loader.available()):
        import __graft_entry__ as g
        g.build()


def make_records(n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, DT)
    for i in range(n):
        k = int(rng.integers(1, 40))
        r["single_reads"][i, :k] = rng.integers(0, 9, (k, 201))
        r["q-scores"][i, :k] = rng.integers(0, 41, (k, 201))
        r["strand"][i, :k] = rng.integers(1, 3, (k, 1))
        r["ref_bases"][i] = rng.integers(1, 5, 201)
        r["num_reads"][i] = k
        r["label"][i] = i % 3
        r["name"][i] = b"chr20:%d" % (1000 + i)
        r["vcfrec"][i] = b"chr20\t%d\t.\tA\tC\t50\t.\tDP=30;AF=0.5\tGT\t0/1" % (1000 + i)
    return r


def read_all(path):
    with hdf5io.CandidateFile(path) as f:
        return f.read(0, len(f))


def native_planes(path):
    with loader.NativeLoader(path, 50, batch_sites=16, threads=2) as nl:
        out = [(b.reads.copy(), b.qual.copy(), b.strand.copy(), b.ref.copy(), list(b.vcfrec), b.num_reads.copy()) for b in nl]
    return out


@pytest.mark.parametrize("steps", [(1,), (7,), (8,), (9,), (16, 7), (13, 11), (3, 2, 1, 30)])
def test_chunk_written_file_equals_the_host_written_file(tmp_path, steps):
    """Last chunks of 1 and 7 records, whole chunks only, and steps of 13 + 11 records (the tail of 5 is carried into the
    second step's first chunk)."""
    parts = [make_records(n, 10 * i + n) for i, n in enumerate(steps)]
    recs = np.concatenate(parts)
    a, b = str(tmp_path / "host.hdf"), str(tmp_path / "chunks.hdf")
    hdf5io.write_candidates(a, parts[0], chunk=CHUNK)
    for p in parts[1:]:
        hdf5io.append_candidates(a, p)
    with hdf5io.ChunkWriter(b, DT, chunk=CHUNK) as w:
        for i, p in enumerate(parts):
            w.append_records(p)
            assert len(w) == sum(len(q) for q in parts[:i + 1]) and len(w.pending) < CHUNK
    assert w.host_chunks == -(-len(recs) // CHUNK)
    got = read_all(b)
    assert got.dtype == DT and got.tobytes() == recs.tobytes() == read_all(a).tobytes()
    n_b, chunk_b, filters_b = hdf5io.dataset_layout(b)
    n_a, chunk_a, filters_a = hdf5io.dataset_layout(a)
    assert n_b == n_a == len(recs) and chunk_b == CHUNK and filters_b == filters_a == [(hdf5io.FILTER_DEFLATE, (4,))]
    if len(parts[0]) >= CHUNK:
        assert chunk_a == CHUNK                                   # (write_candidates shrinks the chunk of a shorter first step)
    for x, y in zip(native_planes(a), native_planes(b)):
        for u, v in zip(x, y):
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v


def test_write_chunks_takes_streams_and_unfiltered_chunks(tmp_path):
    """``write_chunks`` as the device path calls it: streams of ``zd_deflate_host``, one chunk handed over raw with the filter
    skipped ("store"), the last chunk padded with zero records; then the same writer goes on with records."""
    recs = make_records(2 * CHUNK + 3, 7)
    raw = np.zeros(3 * CHUNK, DT)
    raw[:len(recs)] = recs
    pieces, store = [], []
    for c in range(3):
        image = raw[c * CHUNK:(c + 1) * CHUNK].tobytes()
        stream, _adler, _flag = pileup_gpu.zd_deflate_host(image)
        assert zlib.decompress(stream) == image
        pieces.append(image if c == 1 else stream)
        store.append(c == 1)
    sizes = np.array([len(p) for p in pieces], np.uint64)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    chunks = pileup_gpu.CompressedChunks(len(recs), np.frombuffer(b"".join(pieces), np.uint8), offs, sizes, np.zeros(3, np.uint32),
                                         np.array(store, np.uint8))
    path = str(tmp_path / "direct.hdf")
    with hdf5io.ChunkWriter(path, DT, chunk=CHUNK) as w:
        assert w.need() == 0
        w.write_chunks(chunks)
        assert w.direct_chunks == 3 and w.stored_chunks == 1
        with pytest.raises(ValueError, match="multiple of 8"):
            w.append_records(make_records(CHUNK, 1))              # the padded last chunk is written: nothing may follow it
        w.pending = w.pending[:0]
    assert read_all(path).tobytes() == recs.tobytes()


def test_a_misaligned_chunk_is_never_written(tmp_path):
    path = str(tmp_path / "m.hdf")
    one = pileup_gpu.CompressedChunks(CHUNK, np.zeros(10, np.uint8), np.zeros(1, np.uint64), np.full(1, 10, np.uint64),
                                      np.zeros(1, np.uint32), np.zeros(1, np.uint8))
    with hdf5io.ChunkWriter(path, DT, chunk=CHUNK) as w:
        w.append_records(make_records(3, 1))
        assert w.need() == 5
        with pytest.raises(ValueError, match="3 carried records"):
            w.write_chunks(one)
        with pytest.raises(ValueError, match="in 1 chunks"):
            hdf5io.ChunkWriter(str(tmp_path / "n.hdf"), DT, chunk=CHUNK).write_chunks(
                pileup_gpu.CompressedChunks(CHUNK + 1, one.data, one.offsets, one.sizes, one.adlers, one.store))
    assert len(read_all(path)) == 3
    # appending: onto a whole number of chunks it goes on; onto a partial last chunk it is refused, with the reason
    with pytest.raises(ValueError, match="holds 3 records, not a multiple of the chunk size 8"):
        hdf5io.ChunkWriter(path, DT, chunk=CHUNK, append=True)
    a, b = make_records(2 * CHUNK, 2), make_records(5, 3)
    with hdf5io.ChunkWriter(path, DT, chunk=CHUNK) as w:
        w.append_records(a)
    with hdf5io.ChunkWriter(path, DT, chunk=CHUNK, append=True) as w:
        w.append_records(b)
    assert read_all(path).tobytes() == np.concatenate([a, b]).tobytes()
    host = str(tmp_path / "small_chunk.hdf")
    hdf5io.write_candidates(host, make_records(3, 1), chunk=CHUNK)          # (chunks of 3 records)
    with pytest.raises(ValueError, match="chunks of 3 records"):
        hdf5io.ChunkWriter(host, DT, chunk=CHUNK, append=True)


def test_blob_dtype_is_the_record_without_its_planes():
    for mr, w in ((200, 201), (50, 201), (7, 33)):
        rec, blob = record_dtype(mr, w), blob_dtype(w)
        assert blob.itemsize == 149 + 16 * w == rec.itemsize - 3 * mr * w
        assert blob.names == tuple(n for n in rec.names if n not in ("single_reads", "q-scores", "strand"))
        head = rec.fields["single_reads"][1]
        for n in blob.names:
            off = rec.fields[n][1]
            assert blob.fields[n][1] == (off if off < head else off - mr * w) and blob.fields[n][0] == rec.fields[n][0]


def test_compress_device_is_refused_without_the_gpu_encoder():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import convert_bam_single_reads as conv
    from dl4vc_amd import pileup_encoder as PE
    with pytest.raises(SystemExit, match="--pileup-device gpu as well"):
        conv.main(["--input", "x.bam", "--fp_vcf", "x.vcf", "--output", "x.hdf", "--save-q-scores", "--save-strand", "--compress-device", "gpu"])
    with pytest.raises(ValueError, match="needs device='gpu'"):
        PE.encode_locations("x.bam", "x.fa", [], PE.EncoderOptions(), compress_device="gpu")
    with pytest.raises(ValueError, match="compress_device"):
        PE.encode_locations("x.bam", "x.fa", [], PE.EncoderOptions(), device="gpu", compress_device="cpu")
