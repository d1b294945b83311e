"""Fixtures of the device loader's tests (tests/test_loader_device_cli.py on the CPU, tests/test_loader_device_gpu.py on the GPU):
45 synthetic records -- five whole chunks of 8 and one of 5 -- and the ways a file of them is written."""
import ctypes as C

import numpy as np

from dl4vc_amd import hdf5io, pileup_gpu, synth

N = 45                      # five whole chunks of 8 and one of 5
SEED = 5
RAW_CHUNK = 2               # records 16..23: the chunk one file holds raw, its filter mask skipping deflate


def make_records(stored, reads):
    """45 synthetic records: sites deeper than ``reads`` (their subset is drawn with the seed), sites at exactly ``reads`` and
    below, one without any read, a blacklisted record (REF does not match the window), two contigs."""
    batch = synth.make_sites(N, reads=reads, seed=31)
    recs = hdf5io.records_from_sites(batch, store_reads=stored)
    rng = np.random.default_rng(3)
    for i in (2, 9, 17, 30, 44):                                  # deeper than `reads`
        n = stored - (i % 4)
        recs[i]["num_reads"] = n
        for f in ("single_reads", "q-scores", "strand"):
            recs[i][f][reads:n] = recs[i][f][rng.integers(0, max(1, int(batch.num_reads[i])), n - reads)]
    for i in (5, 21):                                             # exactly `reads`
        recs[i]["num_reads"] = reads
        for f in ("single_reads", "q-scores", "strand"):
            recs[i][f][:reads] = recs[i][f][rng.integers(0, max(1, int(batch.num_reads[i])), reads)]
    recs[11]["num_reads"] = 0                                     # no read at all: zero rows
    for f in ("single_reads", "q-scores", "strand"):
        recs[11][f][:] = 0
    cols = recs[7]["vcfrec"].decode().split("\t")                 # a REF base the window does not hold: the blacklist fallback
    cols[3] = next(b for b in "ACGT" if b not in (cols[3][0], cols[4][0])) + cols[3][1:]
    recs[7]["vcfrec"] = "\t".join(cols).encode()
    for i in range(30, N):                                        # a second contig
        recs[i]["vcfrec"] = recs[i]["vcfrec"].decode().replace("chr20", "chr21", 1).encode()
    return recs


def _padded(recs):
    out = np.zeros(8, recs.dtype)
    out[:len(recs)] = recs
    return out


def write_chunks(path, recs, raw=(), damage=()):
    """The file written chunk by chunk past the filter (``ChunkWriter.write_chunks``): zlib streams of the compressor's CPU twin,
    the chunks in ``raw`` as their bytes with the filter mask set, those in ``damage`` with one byte of the stream flipped."""
    pieces = []
    for c in range(0, len(recs), 8):
        image = np.ascontiguousarray(_padded(recs[c:c + 8]))
        piece = image.tobytes() if c // 8 in raw else pileup_gpu.zd_deflate_host(image)[0]
        if c // 8 in damage:
            piece = bytearray(piece)
            piece[len(piece) // 2] ^= 0x40
        pieces.append(bytes(piece))
    sizes = np.array([len(s) for s in pieces], np.uint64)
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
    store = np.array([c in raw for c in range(len(pieces))], np.uint8)
    chunks = pileup_gpu.CompressedChunks(len(recs), np.frombuffer(b"".join(pieces), np.uint8), offs, sizes, np.zeros(len(pieces), np.uint32), store)
    with hdf5io.ChunkWriter(path, recs.dtype, chunk=8) as w:
        w.write_chunks(chunks)
    return w


def chunk_written(path, recs, codes):
    with hdf5io.ChunkWriter(path, recs.dtype, chunk=8, codes=codes) as w:
        w.append_records(recs)
    return w


def create_dataset(path, recs, chunked, shuffle):
    """A dataset the loader must refuse: contiguous, or chunked with shuffle in front of deflate."""
    lib = hdf5io.libhdf5()
    lib.H5Pset_shuffle.restype, lib.H5Pset_shuffle.argtypes = C.c_int, [hdf5io.hid_t]
    fid = lib.H5Fcreate(path.encode(), hdf5io.H5F_ACC_TRUNC, 0, 0)
    tid = hdf5io._h5_compound_type(lib, recs.dtype)
    dims = (hdf5io.hsize_t * 1)(len(recs))
    sid = lib.H5Screate_simple(1, dims, None)
    pl = lib.H5Pcreate(lib._g("H5P_CLS_DATASET_CREATE_ID_g"))
    if chunked:
        lib.H5Pset_chunk(pl, 1, (hdf5io.hsize_t * 1)(8))
    if shuffle:
        lib.H5Pset_shuffle(pl)
        lib.H5Pset_deflate(pl, 4)
    did = lib.H5Dcreate2(fid, hdf5io.DATASET_NAME.encode(), tid, sid, 0, pl, 0)
    assert did >= 0
    buf = np.ascontiguousarray(recs)
    assert lib.H5Dwrite(did, tid, 0, 0, 0, buf.ctypes.data_as(C.c_void_p)) >= 0
    for closer, h in ((lib.H5Dclose, did), (lib.H5Pclose, pl), (lib.H5Sclose, sid), (lib.H5Tclose, tid), (lib.H5Fclose, fid)):
        closer(h)
