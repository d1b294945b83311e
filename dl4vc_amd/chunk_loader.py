"""The candidate file's chunks inflated and its sites assembled on the GPU (``cl_*`` of libdl4vc_pileup.so,
``include/dl4vc_chunks.h``): where ``loader.NativeLoader`` inflates every chunk with host zlib and assembles every site on host
threads, ``DeviceChunkLoader`` reads the chunks as the file holds them (``hdf5io.RawChunkFile``), uploads those 3-7 KB per site,
inflates them on the device (``zi_inflate_kernel``), brings back only each record's members outside the three planes, plans rows
and allele masks on the host (``site_assembly.plan_sites``, the definition ``--test_bam`` uses) and assembles the six planes of
the forward in device memory (``cl_assemble_device``).  Same planes, byte for byte.

torch is imported before the library is loaded: the loader shares device buffers and streams with it (one HIP runtime per
process)."""
from __future__ import annotations

import ctypes as C
import threading
import time
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import pileup_gpu
from .hdf5_schema import PLANE_FIELDS, blob_dtype
from .hdf5io import RawChunkFile
from .site_assembly import SitePlan, plan_records, plan_sites

CL_SYMBOLS = ("cl_open", "cl_close", "cl_last_error", "cl_inflate_chunks_device", "cl_assemble_device", "cl_get_stats",
              "cl_center_counts_device", "cl_center_counts_host",
              "cl_store_open", "cl_store_close", "cl_store_last_error", "cl_store_append_device", "cl_store_assemble_device",
              "cl_store_center_counts_device", "cl_store_extent_host", "cl_store_pack_host", "cl_store_assemble_host", "cl_store_record",
              "cl_store_slab", "cl_store_debug_fill", "cl_store_get_stats",
              "cl_store_append_planes_device", "cl_store_extent_planes_host", "cl_store_pack_planes_host",
              "cl_store_set_format", "cl_store_record_span", "cl_store_get_format_stats", "cl_store_spans_host",
              "cl_store_spans_planes_host")
RECORD_FORMATS = {"rows": 0, "compact": 1}   # ``cl_store_set_format``
COMPACT_MAX_WINDOW = 255
STORE_SLAB_BYTES = 256 << 20        # the record store grows in device slabs of this size
FILL_ROUND_LOCATIONS = 4096         # locations one round of the store's fill from a BAM encodes (3 x 4096 x 200 x 201 bytes of staging)
FILL_GROUP_CHUNKS = 512             # chunks one inflate launch of the store's fill holds (a chunk keeps one lane busy whatever else runs)
_bound = None
# libhdf5 is not thread-safe: the raw chunk reads of every loader of the process (the training file's and the test file's workers)
# take this lock, so at most one thread is inside the library
HDF5_LOCK = threading.Lock()


class Stats(C.Structure):
    """``cl_stats``."""
    _fields_ = [(n, C.c_double) for n in ("upload_ms", "inflate_ms", "blob_copy_back_ms", "assemble_ms")] + \
               [(n, C.c_int64) for n in ("chunks", "compressed_bytes", "inflated_bytes", "raw_chunks")]


class StoreStats(C.Structure):
    """``cl_store_stats``."""
    _fields_ = [(n, C.c_int64) for n in ("records", "stored_bytes", "inflated_bytes", "slabs", "refused_fit_records", "refused_fit_bytes")] + \
               [(n, C.c_double) for n in ("extent_ms", "pack_ms", "assemble_ms")]


class StoreFormatStats(C.Structure):
    """``cl_store_format_stats``."""
    _fields_ = [(n, C.c_int64) for n in ("format", "rows_records", "rows_bytes", "compact_records", "compact_bytes")] + \
               [("spans_ms", C.c_double)]


def load_library() -> C.CDLL:
    global _bound
    if _bound is None:
        lib = pileup_gpu.load_library()
        vp = C.c_void_p
        lib.cl_open.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64, C.c_int32, C.POINTER(vp)]
        lib.cl_close.argtypes = [vp]
        lib.cl_close.restype = None
        lib.cl_last_error.argtypes = [vp]
        lib.cl_last_error.restype = C.c_char_p
        lib.cl_inflate_chunks_device.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_int64, vp, C.POINTER(vp), vp]
        lib.cl_assemble_device.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32] + [vp] * 6 + [vp]
        lib.cl_get_stats.argtypes = [vp, C.POINTER(Stats)]
        for fn in (lib.cl_center_counts_device, lib.cl_center_counts_host):
            fn.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, vp]
        lib.cl_store_open.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(vp)]
        lib.cl_store_close.argtypes = [vp]
        lib.cl_store_close.restype = None
        lib.cl_store_last_error.argtypes = [vp]
        lib.cl_store_last_error.restype = C.c_char_p
        lib.cl_store_append_device.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp]
        for fn in (lib.cl_store_assemble_device, lib.cl_store_assemble_host):
            fn.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32] + [vp] * 6 + [vp]
        lib.cl_store_center_counts_device.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, vp]
        lib.cl_store_extent_host.argtypes = [vp, C.c_uint64, C.c_int64, vp, C.c_int32, C.c_int32, vp, C.c_int64, vp]
        lib.cl_store_pack_host.argtypes = [vp, vp, C.c_uint64, C.c_int64, vp, vp, vp, C.c_int64, vp]
        lib.cl_store_append_planes_device.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp]
        lib.cl_store_extent_planes_host.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int64, vp]
        lib.cl_store_pack_planes_host.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, vp]
        lib.cl_store_record.argtypes = [vp, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        lib.cl_store_slab.argtypes = [vp, C.c_int32, vp, C.c_uint64] + [C.POINTER(C.c_int64)] * 3
        lib.cl_store_debug_fill.argtypes = [vp, C.c_int32]
        lib.cl_store_get_stats.argtypes = [vp, C.POINTER(StoreStats)]
        lib.cl_store_set_format.argtypes = [vp, C.c_int32]
        lib.cl_store_record_span.argtypes = [vp, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        lib.cl_store_get_format_stats.argtypes = [vp, C.POINTER(StoreFormatStats)]
        lib.cl_store_spans_host.argtypes = [vp, C.c_uint64, C.c_int64, vp, C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, vp, vp]
        lib.cl_store_spans_planes_host.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int64, vp, vp, vp, vp]
        _bound = lib
    return _bound


class DamagedChunk(ValueError):
    """A chunk of the file does not inflate: ``chunk at record N: <status text>``."""


def center_counts_host(reads) -> np.ndarray:
    """``cl_center_counts_host``: reads ``[m][R][L]`` uint8 -> counts ``[m][2][16]`` int32 of the tokens 0..15 at columns
    ``(L - 1) // 2`` and the one after it over the R rows -- the CPU definition of ``cl_center_counts_device``."""
    reads = np.ascontiguousarray(reads, np.uint8)
    m, R, L = reads.shape                                  # (L odd: the centre column is (L - 1) // 2)
    out = np.zeros((m, 2, 16), np.int32)
    lib = load_library()
    if lib.cl_center_counts_host(None, reads.ctypes.data_as(C.c_void_p), m, R, L, out.ctypes.data_as(C.c_void_p), None) != 0:
        raise RuntimeError("cl_center_counts_host failed: %s" % lib.cl_last_error(None).decode())
    return out


def check_layout(f: RawChunkFile, reads: int):
    """What the device loader needs of a file's records beyond ``RawChunkFile``'s own refusals -> (window, stored rows, the three
    plane offsets).  Needs no device: the command line refuses a file with these texts before it touches one."""
    path = f.path
    miss = [k for k in PLANE_FIELDS + ("ref_bases", "num_reads", "vcfrec") if k not in f.offsets]
    if miss:
        raise ValueError("%s: the records have no member %s" % (path, miss))
    p = [f.offsets[k] for k in PLANE_FIELDS]
    W = (p[0] - 16) // 15 if p[0] >= 31 else 0
    S = (p[2] - p[1]) // W if W else 0
    if W != 201:
        raise ValueError("%s holds windows of %d columns: the allele masks are defined on the 201-column window (window size 100)"
                         % (path, W))
    if reads > S:
        raise ValueError("the model reads %d rows per site but %s stores only %d" % (reads, path, S))
    return W, S, p


@dataclass
class IndexedSites:
    """What ``DeviceChunkLoader.load_indices`` hands back beside the planes it enqueued."""
    plan: SitePlan
    label: np.ndarray        # (m,) the records' ``label`` member
    counts: np.ndarray       # (m,2,16) i32 ``cl_center_counts_device`` of the assembled reads plane


class DeviceChunkLoader:
    """Records ``[lo, hi)`` of a candidate file, ``batch_sites`` at a time, as planes in device memory.

    ``load(b0, b1, outs, stream)`` inflates the chunks that cover ``[b0, b1)`` (the range need not be chunk-aligned; the records
    of those chunks outside it, and the padding of an edge chunk, are never planned), and assembles the records' sites into
    ``outs`` -- six device addresses (reads, qual, strand ``[m][reads][window]``, ref, ref_mask, var_mask ``[m][window]``).
    Record ``i`` of the file draws the read subset of a deep pileup with ``seed + i``, whatever the range.

    Device memory: the inflated records, ``(batch_sites + 2 * chunk - 1) * record_bytes`` rounded up to chunks (512 MB at 4096
    sites of the production layout), and the compressed chunks.

    ``shuffled=G`` (``True`` = 1) opens the handle for ``load_indices`` / ``inflate_lists`` of G index lists at a time: every one of
    ``G * batch_sites`` records may lie in a chunk of its own, so the record buffer holds that many whole chunks (79 MB per list
    of 80 sites of the production layout) -- or, with ``chunks``, that many to begin with: ``reserve`` reopens the handle for more,
    up to that bound and never more than the file has, so a caller that knows its index lists (sequential evaluation batches
    span ``batch_sites / chunk`` chunks, not ``batch_sites``) pays for what they touch.  At the command line's default batch of
    1 000 sites a shuffled epoch over a large file needs 4 x 1 000 chunks: 4 GB of the production layout."""

    def __init__(self, path: str, reads: int, batch_sites: int = 4096, seed: int = 0, device: int = 0, use_q: bool = True,
                 use_strand: bool = True, shuffled: int = 0, chunks: Optional[int] = None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("the device loader needs a HIP device visible to torch; there is no CPU path (NativeLoader is it)")
        self.torch = torch
        self.file = RawChunkFile(path)
        self._h = None
        try:
            f = self.file
            W, S, p = check_layout(f, reads)
            self.window, self.stored_rows, self.reads, self.B = W, S, int(reads), int(batch_sites)
            self.seed, self.use_q, self.use_strand, self.device = seed, use_q, use_strand, device
            self.blob_dtype = blob_dtype(W)
            self.lib = load_library()
            offs = (C.c_int64 * 3)(*p)
            self.ahead = int(shuffled)
            self.chunk_limit = min(self.ahead * self.B, -(-len(f) // f.chunk)) if shuffled else 0
            self.max_chunks = max(1, min(self.chunk_limit, chunks or self.chunk_limit)) if shuffled else -(-(self.B + f.chunk) // f.chunk) + 1
            self._open_args = (f.itemsize, f.chunk, W, S, offs, int(device))
            self._open(self.max_chunks * f.chunk if shuffled else self.B + f.chunk)
            if self.blob_dtype.itemsize != f.itemsize - 3 * S * W:
                raise ValueError("%s: records of %d bytes do not match the schema" % (path, f.itemsize))
            # pinned staging of the raw chunks, grown on demand
            self._comp = torch.empty(0, dtype=torch.uint8)
            self._counts = None                              # load_indices: device counts and their pinned copy
            self._group = None                               # inflate_lists: (chunk numbers, the records' non-plane members)
            self.stage = {k: 0.0 for k in ("read_ms", "upload_ms", "inflate_ms", "blob_copy_back_ms", "plan_ms", "assemble_ms")}
            self.stage.update({k: 0 for k in ("chunks", "compressed_bytes", "inflated_bytes", "raw_chunks", "records")})
        except Exception:
            self.close()
            raise

    def __len__(self):
        return len(self.file)

    def _open(self, max_records: int) -> None:
        itemsize, chunk, W, S, offs, device = self._open_args
        h = C.c_void_p()
        if self.lib.cl_open(itemsize, chunk, W, S, offs, max_records, device, C.byref(h)) != 0:
            raise RuntimeError("cl_open failed: %s" % self.lib.cl_last_error(None).decode())
        self._h = h

    def reserve(self, n_chunks: int) -> None:
        """Room for ``n_chunks`` chunks in one ``inflate_lists`` (a handle opened with ``shuffled``): the handle is closed and
        opened again when it holds fewer.  The inflated records of the last call are gone afterwards."""
        n_chunks = int(n_chunks)
        if n_chunks > self.chunk_limit:
            raise ValueError("%d chunks, the handle is limited to %d (shuffled=%d lists of %d sites, %d chunks in the file)"
                             % (n_chunks, self.chunk_limit, self.ahead, self.B, -(-len(self.file) // self.file.chunk)))
        if n_chunks <= self.max_chunks:
            return
        self._group = None
        self.lib.cl_close(self._h)                          # (waits for what the handle has in flight)
        self._h = None
        self._open(n_chunks * self.file.chunk)
        self.max_chunks = n_chunks

    def chunks_of(self, lists) -> int:
        """Distinct chunks the indices of ``lists`` fall in: what one ``inflate_lists`` of them needs."""
        lists = [np.asarray(i, np.int64).reshape(-1) for i in lists]
        return len(np.unique(np.concatenate(lists) // self.file.chunk)) if lists else 0

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, self.lib.cl_last_error(self._h).decode()))

    def _read_chunks(self, c0: int, c1: int):
        """The raw chunks [c0, c1) into pinned memory -> (buffer, offsets, sizes, raw flags)."""
        return self._read_chunk_list(range(c0, c1))

    def _read_chunk_list(self, chunks):
        """The raw chunks named in ``chunks`` into pinned memory, in that order."""
        f, torch = self.file, self.torch
        with HDF5_LOCK:
            sizes = np.array([f.stored_size(c) for c in chunks], np.uint64)
            offs = np.zeros(len(sizes), np.uint64)
            offs[1:] = np.cumsum((sizes[:-1] + np.uint64(15)) & ~np.uint64(15))     # every chunk at a 16-byte boundary
            total = int(offs[-1] + sizes[-1]) if len(sizes) else 0
            if self._comp.numel() < total:
                self._comp = torch.empty(total + total // 4 + 4096, dtype=torch.uint8).pin_memory()
            base = self._comp.data_ptr()
            raw = np.zeros(len(sizes), np.uint8)
            for k, c in enumerate(chunks):
                raw[k] = f.read_chunk(int(c), base + int(offs[k])) & 1
        return total, offs, sizes, raw

    def load(self, b0: int, b1: int, outs, stream: int = 0) -> SitePlan:
        """Records ``[b0, b1)`` (at most ``batch_sites``) -> their plan; the planes are enqueued on ``stream`` (a raw
        hipStream_t) into ``outs``.  The chunk inflate has been waited for, the assembly has not."""
        f = self.file
        b1 = min(b1, len(f))
        if not (0 <= b0 <= b1) or b1 - b0 > self.B:
            raise ValueError("records [%d, %d): at most %d per call, inside the file's %d" % (b0, b1, self.B, len(f)))
        if b0 == b1:
            return plan_sites(np.zeros(0, np.int8), np.zeros(0, np.int32), np.zeros((0, self.window), np.uint8), [], self.reads,
                              self.stored_rows, self.seed, first_record=b0)
        c0, c1 = b0 // f.chunk, -(-b1 // f.chunk)
        n = c1 - c0
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        t0 = time.perf_counter()
        total, offs, sizes, raw = self._read_chunks(c0, c1)
        t1 = time.perf_counter()
        blob_p = C.c_void_p()
        status = np.zeros(n, np.int32)
        self._check(self.lib.cl_inflate_chunks_device(self._h, C.c_void_p(self._comp.data_ptr()), total, p(offs), p(sizes), p(raw), n,
                                                      C.c_void_p(stream or None), C.byref(blob_p), p(status)), "cl_inflate_chunks_device")
        bad = np.flatnonzero(status)
        if len(bad):
            from . import zinflate
            raise DamagedChunk("%s: chunk at record %d: %s" % (f.path, (c0 + int(bad[0])) * f.chunk, zinflate.status_text(status[bad[0]])))
        t2 = time.perf_counter()
        n_slots = n * f.chunk
        blob = np.ctypeslib.as_array(C.cast(blob_p, C.POINTER(C.c_uint8)), (n_slots * self.blob_dtype.itemsize,)).view(self.blob_dtype)
        inside = np.zeros(n_slots, np.int8)
        inside[b0 - c0 * f.chunk:b1 - c0 * f.chunk] = 1
        texts = [bytes(v).decode() for v in blob["vcfrec"]]
        plan = plan_sites(inside, blob["num_reads"].reshape(-1), blob["ref_bases"].reshape(n_slots, self.window), texts, self.reads,
                          self.stored_rows, self.seed, first_record=b0)
        t3 = time.perf_counter()
        first = np.ascontiguousarray(plan.first_rows, np.uint8)
        rows = np.ascontiguousarray(plan.rows, np.int16) if not first.all() else None
        lines = [np.ascontiguousarray(a, np.uint8) for a in (plan.ref, plan.ref_mask, plan.var_mask)]
        q = lambda a: p(a) if a is not None else None   # noqa: E731
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        self._check(self.lib.cl_assemble_device(self._h, p(np.ascontiguousarray(plan.slots, np.int32)), q(rows), p(first), len(plan),
                                                self.reads, *[p(a) for a in lines], int(bool(self.use_q)), int(bool(self.use_strand)),
                                                *[v(x) for x in outs], v(stream)), "cl_assemble_device")
        st = Stats()
        self._check(self.lib.cl_get_stats(self._h, C.byref(st)), "cl_get_stats")
        for k, _t in Stats._fields_:
            self.stage[k] += getattr(st, k)
        self.stage["read_ms"] += (t1 - t0) * 1e3
        self.stage["plan_ms"] += (t3 - t2) * 1e3
        self.stage["records"] += len(plan)
        return plan

    def load_indices(self, indices, seed: int, outs, stream: int = 0, downsample_rate: float = 0.0,
                     downsample_prob: float = 0.0) -> IndexedSites:
        """The records at ``indices`` -- absolute record indices in any order, at most ``batch_sites`` -- as the sites of ``outs``
        in that order: site i is record ``indices[i]`` and draws the subset of a deep pileup with ``seed + indices[i]``
        (``train_data.assemble_training_batch``'s rule).  Every distinct chunk an index falls in is read once, in ascending
        chunk order, and inflated on the device; two indices of one chunk share it.  After the assembly the reads plane's centre
        tokens are counted (``cl_center_counts_device``) for the targets.  Everything is enqueued on ``stream`` and waited for:
        the planes are complete when the call returns.  The handle must have been opened with ``shuffled``.
        = ``inflate_lists([indices])`` + ``assemble_list(indices)``.  ``downsample_rate`` / ``downsample_prob``: dynamic read
        down-sampling of a training batch (``site_assembly.plan_records``)."""
        self.inflate_lists([indices], stream)
        return self.assemble_list(indices, seed, outs, stream, downsample_rate, downsample_prob)

    def inflate_lists(self, lists, stream: int = 0) -> None:
        """The chunks of SEVERAL index lists (at most ``shuffled`` of them, each of at most ``batch_sites`` indices) read and
        inflated in one launch: a chunk takes one decoding lane tens of milliseconds whatever the launch holds, so the lists
        of a few batches share that time.  ``assemble_list`` then serves each of the lists from the inflated records, until the
        next ``inflate_lists``."""
        f = self.file
        lists = [np.asarray(i, np.int64).reshape(-1) for i in lists]
        if len(lists) > self.ahead:
            raise ValueError("%d index lists, the handle was opened for %d at a time (shuffled=)" % (len(lists), self.ahead))
        for idx in lists:
            if len(idx) > self.B:
                raise ValueError("%d indices: at most %d per call" % (len(idx), self.B))
            if len(idx) and (idx.min() < 0 or idx.max() >= len(f)):
                raise ValueError("record indices %d..%d outside the file's %d records" % (idx.min(), idx.max(), len(f)))
        self._group = None
        chunks = np.unique(np.concatenate(lists) // f.chunk) if lists else np.zeros(0, np.int64)      # ascending
        n = len(chunks)
        if n > self.max_chunks:
            raise ValueError("the indices lie in %d chunks, the handle was opened for %d: reserve() more" % (n, self.max_chunks))
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        t0 = time.perf_counter()
        total, offs, sizes, raw = self._read_chunk_list(chunks)
        t1 = time.perf_counter()
        blob_p = C.c_void_p()
        status = np.zeros(n, np.int32)
        self._check(self.lib.cl_inflate_chunks_device(self._h, C.c_void_p(self._comp.data_ptr()), total, p(offs), p(sizes), p(raw), n,
                                                      C.c_void_p(stream or None), C.byref(blob_p), p(status)), "cl_inflate_chunks_device")
        bad = np.flatnonzero(status)
        if len(bad):
            from . import zinflate
            raise DamagedChunk("%s: chunk at record %d: %s" % (f.path, int(chunks[bad[0]]) * f.chunk, zinflate.status_text(status[bad[0]])))
        n_slots = n * f.chunk
        blob = np.ctypeslib.as_array(C.cast(blob_p, C.POINTER(C.c_uint8)), (n_slots * self.blob_dtype.itemsize,)).view(self.blob_dtype) \
            if n_slots else np.zeros(0, self.blob_dtype)
        self._group = (chunks, blob)
        st = Stats()
        self._check(self.lib.cl_get_stats(self._h, C.byref(st)), "cl_get_stats")
        for k, _t in Stats._fields_:
            if k != "assemble_ms":
                self.stage[k] += getattr(st, k)
        self.stage["read_ms"] += (t1 - t0) * 1e3

    def assemble_list(self, indices, seed: int, outs, stream: int = 0, downsample_rate: float = 0.0,
                      downsample_prob: float = 0.0) -> IndexedSites:
        """One of the lists of the last ``inflate_lists`` (or any indices inside its chunks) assembled into ``outs``; the second
        half of ``load_indices``."""
        f, torch = self.file, self.torch
        if self._group is None:
            raise RuntimeError("assemble_list: no inflated records (inflate_lists first)")
        chunks, blob = self._group
        idx = np.asarray(indices, np.int64).reshape(-1)
        m = len(idx)
        if m > self.B:
            raise ValueError("%d indices: at most %d per call" % (m, self.B))
        where = np.searchsorted(chunks, idx // f.chunk)
        if m and ((where >= len(chunks)).any() or (chunks[np.minimum(where, len(chunks) - 1)] != idx // f.chunk).any()):
            raise ValueError("an index lies outside the chunks of the last inflate_lists")
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        t2 = time.perf_counter()
        n_slots = len(chunks) * f.chunk
        slots = (where * f.chunk + idx % f.chunk).astype(np.int32)
        texts = [None] * n_slots                               # (only the wanted records' text is decoded)
        for s in set(slots.tolist()):
            texts[s] = bytes(blob["vcfrec"][s]).decode()
        plan = plan_records(slots, idx, blob["num_reads"].reshape(-1), blob["ref_bases"].reshape(n_slots, self.window), texts,
                            self.reads, self.stored_rows, seed, downsample_rate, downsample_prob)
        label = np.array(blob["label"].reshape(-1)[slots]) if "label" in self.blob_dtype.names else np.zeros(m, np.uint8)
        t3 = time.perf_counter()
        counts = np.zeros((m, 2, 16), np.int32)
        if m:
            first = np.ascontiguousarray(plan.first_rows, np.uint8)
            rows = np.ascontiguousarray(plan.rows, np.int16) if not first.all() else None
            lines = [np.ascontiguousarray(a, np.uint8) for a in (plan.ref, plan.ref_mask, plan.var_mask)]
            self._check(self.lib.cl_assemble_device(self._h, p(plan.slots), p(rows) if rows is not None else None, p(first), m, self.reads,
                                                    *[p(a) for a in lines], int(bool(self.use_q)), int(bool(self.use_strand)),
                                                    *[v(x) for x in outs], v(stream)), "cl_assemble_device")
            if self._counts is None:
                dev = torch.device("cuda", self.device)
                self._counts = (torch.empty((self.B, 2, 16), dtype=torch.int32, device=dev),
                                torch.empty((self.B, 2, 16), dtype=torch.int32).pin_memory())
            d_counts, h_counts = self._counts
            self._check(self.lib.cl_center_counts_device(self._h, v(outs[0]), m, self.reads, self.window, v(d_counts.data_ptr()), v(stream)),
                        "cl_center_counts_device")
            ts = torch.cuda.ExternalStream(stream, device=d_counts.device) if stream else torch.cuda.default_stream(d_counts.device)
            with torch.cuda.stream(ts):
                h_counts[:m].copy_(d_counts[:m], non_blocking=True)
            ts.synchronize()
            counts[:] = h_counts[:m].numpy()
            st = Stats()
            self._check(self.lib.cl_get_stats(self._h, C.byref(st)), "cl_get_stats")
            self.stage["assemble_ms"] += st.assemble_ms
        t4 = time.perf_counter()
        self.stage["plan_ms"] += (t3 - t2) * 1e3
        self.stage["counts_ms"] = self.stage.get("counts_ms", 0.0) + (t4 - t3) * 1e3      # assembly + counts + their copy back, host clock
        self.stage["records"] += m
        return IndexedSites(plan, label, counts)

    def assemble(self, plan: SitePlan, outs, stream: int = 0) -> None:
        """``cl_assemble_device`` of ``plan`` against the records of the last ``load`` (the tests' door to its range checks)."""
        first = np.ascontiguousarray(plan.first_rows, np.uint8)
        rows = np.ascontiguousarray(plan.rows, np.int16)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        lines = [np.ascontiguousarray(a, np.uint8) for a in (plan.ref, plan.ref_mask, plan.var_mask)]
        self._check(self.lib.cl_assemble_device(self._h, p(np.ascontiguousarray(plan.slots, np.int32)), p(rows), p(first), len(plan),
                                                plan.rows.shape[1], *[p(a) for a in lines], int(bool(self.use_q)),
                                                int(bool(self.use_strand)), *[v(x) for x in outs], v(stream)), "cl_assemble_device")

    def batches(self, lo: int = 0, hi: Optional[int] = None):
        """-> (plan, [six uint8 tensors on the device]) per batch of ``batch_sites`` records of ``[lo, hi)``; the tensors are
        filled with 0xAB before the assembly writes them."""
        torch = self.torch
        hi = len(self) if hi is None else min(hi, len(self))
        dev = torch.device("cuda", self.device)
        for b0 in range(lo, hi, self.B):
            b1 = min(hi, b0 + self.B)
            m = b1 - b0
            outs = [torch.full((m, self.reads, self.window), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)] + \
                   [torch.full((m, self.window), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)]
            s = torch.cuda.current_stream(dev)
            plan = self.load(b0, b1, [t.data_ptr() for t in outs], s.cuda_stream)
            s.synchronize()
            yield plan, outs

    def close(self):
        if self._h is not None:
            self.lib.cl_close(self._h)
            self._h = None
        self.file.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


# ---- the record store: a file's records inflated once and kept in device memory (--train-cache-device gpu) ------------------------
class StoreFull(ValueError):
    """The records do not fit the store's capacity (``--train-cache-bytes``)."""


def record_extents_host(inflated, record_bytes: int, plane_off, stored_rows: int, window: int, slots=None) -> np.ndarray:
    """``cl_store_extent_host``: ``kept`` of the records ``slots`` (all of them by default) of the inflated bytes."""
    inflated = np.ascontiguousarray(inflated, np.uint8).reshape(-1)
    slots = np.arange(len(inflated) // record_bytes, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
    kept = np.zeros(len(slots), np.int32)
    lib = load_library()
    offs = (C.c_int64 * 3)(*[int(x) for x in plane_off])
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if lib.cl_store_extent_host(p(inflated), inflated.nbytes, record_bytes, offs, stored_rows, window, p(slots), len(slots), p(kept)) != 0:
        raise ValueError(lib.cl_store_last_error(None).decode())
    return kept


def plane_extents_host(reads, qual, strand, slots=None) -> np.ndarray:
    """``cl_store_extent_planes_host``: ``kept`` of the slots ``slots`` (all of them by default) of three arrays ``[n][S][W]``."""
    planes = [np.ascontiguousarray(a, np.uint8) for a in (reads, qual, strand)]
    n, S, W = planes[0].shape
    slots = np.arange(n, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
    kept = np.zeros(len(slots), np.int32)
    lib = load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if lib.cl_store_extent_planes_host(*[p(a) for a in planes], n, S, W, p(slots), len(slots), p(kept)) != 0:
        raise ValueError(lib.cl_store_last_error(None).decode())
    return kept


def _spans_out(n: int, stored_rows: int):
    return np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, stored_rows), np.uint16)


def record_spans_host(inflated, record_bytes: int, plane_off, stored_rows: int, window: int, slots=None):
    """``cl_store_spans_host``: the compact format's spans of the records ``slots`` (all of them by default) of the inflated bytes
    -> (kept, cells, mergeable, rowspans ``[n][stored_rows]`` uint16 = ``c0 | n << 8``)."""
    inflated = np.ascontiguousarray(inflated, np.uint8).reshape(-1)
    slots = np.arange(len(inflated) // record_bytes, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
    out = _spans_out(len(slots), stored_rows)
    lib = load_library()
    offs = (C.c_int64 * 3)(*[int(x) for x in plane_off])
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if lib.cl_store_spans_host(p(inflated), inflated.nbytes, record_bytes, offs, stored_rows, window, p(slots), len(slots), *[p(a) for a in out]) != 0:
        raise ValueError(lib.cl_store_last_error(None).decode())
    return out


def plane_spans_host(reads, qual, strand, slots=None):
    """``cl_store_spans_planes_host``: the same of the slots ``slots`` (all of them by default) of three arrays ``[n][S][W]``."""
    planes = [np.ascontiguousarray(a, np.uint8) for a in (reads, qual, strand)]
    n, S, W = planes[0].shape
    slots = np.arange(n, dtype=np.int32) if slots is None else np.ascontiguousarray(slots, np.int32)
    out = _spans_out(len(slots), S)
    lib = load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if lib.cl_store_spans_planes_host(*[p(a) for a in planes], n, S, W, p(slots), len(slots), *[p(a) for a in out]) != 0:
        raise ValueError(lib.cl_store_last_error(None).decode())
    return out


class RecordStore:
    """A ``cl_store_t``: trimmed records in slabs, on ``device`` or (``device < 0``) in host memory, where the CPU definitions
    ``pack_host`` / ``assemble_host`` stand in for ``append_device`` / ``assemble_device``.  A refused call raises ``ValueError``
    (``StoreFull`` for the capacity) with the library's text and leaves the store as it was.  ``record_format="compact"``
    (``cl_store_set_format``): every record that can be is stored as row spans with token and strand in one byte; the assembled
    planes are the same."""

    def __init__(self, window: int, stored_rows: int, n_records: int, capacity_bytes: int, slab_bytes: int = STORE_SLAB_BYTES,
                 device: int = 0, record_format: str = "rows"):
        if record_format not in RECORD_FORMATS:
            raise ValueError("record_format must be one of %s, not %r" % (", ".join(RECORD_FORMATS), record_format))
        self.record_format = record_format
        self.lib = load_library()
        self.window, self.stored_rows, self.n_records, self.device = int(window), int(stored_rows), int(n_records), int(device)
        self.capacity_bytes, self.slab_bytes = int(capacity_bytes), int(slab_bytes)
        h = C.c_void_p()
        if self.lib.cl_store_open(self.window, self.stored_rows, self.n_records, self.capacity_bytes, self.slab_bytes, self.device,
                                  C.byref(h)) != 0:
            raise ValueError("cl_store_open failed: %s" % self.lib.cl_store_last_error(None).decode())
        self._h = h
        if record_format != "rows":
            try:
                self.set_format(record_format)
            except Exception:
                self.close()
                raise

    def _check(self, rc):
        if rc != 0:
            raise (StoreFull if rc == -3 else ValueError if rc == -1 else RuntimeError)(self.lib.cl_store_last_error(self._h).decode())

    def debug_fill(self, value: int) -> None:
        self._check(self.lib.cl_store_debug_fill(self._h, value))

    def set_format(self, record_format) -> None:
        """``cl_store_set_format``: a name of ``RECORD_FORMATS`` (or the library's number); before the first append."""
        self._check(self.lib.cl_store_set_format(self._h, RECORD_FORMATS.get(record_format, record_format)))

    def format_stats(self) -> StoreFormatStats:
        st = StoreFormatStats()
        self._check(self.lib.cl_store_get_format_stats(self._h, C.byref(st)))
        return st

    def record_span(self, i: int):
        """-> (format, bytes) of record ``i``: 0 rows, 1 compact; the bytes it takes in its slab."""
        fmt, b = C.c_int32(), C.c_int64()
        self._check(self.lib.cl_store_record_span(self._h, int(i), C.byref(fmt), C.byref(b)))
        return fmt.value, b.value

    def stats(self) -> StoreStats:
        st = StoreStats()
        self._check(self.lib.cl_store_get_stats(self._h, C.byref(st)))
        return st

    def span(self, kept):
        """Bytes the records of these extents take in a slab."""
        return (3 * np.asarray(kept, np.int64) * self.window + 15) & ~np.int64(15)

    def pack_host(self, inflated, record_bytes: int, plane_off, slots, records) -> np.ndarray:
        inflated = np.ascontiguousarray(inflated, np.uint8).reshape(-1)
        slots, records = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(records, np.int32)
        kept = np.zeros(len(slots), np.int32)
        offs = (C.c_int64 * 3)(*[int(x) for x in plane_off])
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        self._check(self.lib.cl_store_pack_host(self._h, p(inflated), inflated.nbytes, record_bytes, offs, p(slots), p(records), len(slots),
                                                p(kept)))
        return kept

    def append_device(self, loader_handle, slots, records, stream: int = 0) -> np.ndarray:
        slots, records = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(records, np.int32)
        kept = np.zeros(len(slots), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        self._check(self.lib.cl_store_append_device(self._h, loader_handle, p(slots), p(records), len(slots), C.c_void_p(stream or None),
                                                    p(kept)))
        return kept

    def pack_planes_host(self, reads, qual, strand, slots, records) -> np.ndarray:
        """``cl_store_pack_planes_host``: slots ``slots`` of three host arrays ``[n_slots][stored_rows][window]`` become the
        records ``records`` of a host store."""
        planes = [np.ascontiguousarray(a, np.uint8) for a in (reads, qual, strand)]
        for a in planes:
            if a.shape != (planes[0].shape[0], self.stored_rows, self.window):
                raise ValueError("planes: three arrays [n][%d][%d], not %s" % (self.stored_rows, self.window, a.shape))
        slots, records = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(records, np.int32)
        kept = np.zeros(len(slots), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        self._check(self.lib.cl_store_pack_planes_host(self._h, *[p(a) for a in planes], len(planes[0]), p(slots), p(records), len(slots),
                                                       p(kept)))
        return kept

    def append_planes_device(self, planes, n_slots: int, slots, records, stream: int = 0) -> np.ndarray:
        """``cl_store_append_planes_device``: ``planes`` = the device addresses of three arrays ``[n_slots][stored_rows][window]``
        (the pileup encoder's output; read only, any alignment)."""
        slots, records = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(records, np.int32)
        kept = np.zeros(len(slots), np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        self._check(self.lib.cl_store_append_planes_device(self._h, *[v(x) for x in planes], int(n_slots), p(slots), p(records), len(slots),
                                                           C.c_void_p(stream or None), p(kept)))
        return kept

    def _assemble(self, fn, records, rows, first_rows, reads, lines, use_q, use_strand, outs, stream):
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        records = np.ascontiguousarray(records, np.int32)
        rows = np.ascontiguousarray(rows, np.int16) if rows is not None else None
        first = np.ascontiguousarray(first_rows, np.uint8) if first_rows is not None else None
        lines = [np.ascontiguousarray(a, np.uint8) for a in lines]
        self._check(fn(self._h, p(records), p(rows), p(first), len(records), int(reads), *[p(a) for a in lines], int(bool(use_q)),
                       int(bool(use_strand)), *[v(x) for x in outs], v(stream)))

    def assemble_device(self, records, rows, first_rows, reads, lines, use_q, use_strand, outs, stream: int = 0) -> None:
        """``cl_store_assemble_device``: ``lines`` = (ref, ref_mask, var_mask) ``[m][window]`` host arrays, ``outs`` six device
        addresses; asynchronous on ``stream``."""
        self._assemble(self.lib.cl_store_assemble_device, records, rows, first_rows, reads, lines, use_q, use_strand, outs, stream)

    def assemble_host(self, records, rows, first_rows, reads, lines, use_q=True, use_strand=True):
        """``cl_store_assemble_host`` -> the six planes as numpy arrays."""
        m, L = len(records), self.window
        outs = [np.full((m, reads, L), 0xAB, np.uint8) for _ in range(3)] + [np.full((m, L), 0xAB, np.uint8) for _ in range(3)]
        self._assemble(self.lib.cl_store_assemble_host, records, rows, first_rows, reads, lines, use_q, use_strand,
                       [a.ctypes.data for a in outs], 0)
        return outs

    def record(self, i: int):
        """-> (slab, offset, kept) of record ``i``; of a device store, as the table in device memory has it."""
        slab, off, kept = C.c_int32(), C.c_int64(), C.c_int32()
        self._check(self.lib.cl_store_record(self._h, int(i), C.byref(slab), C.byref(off), C.byref(kept)))
        return slab.value, off.value, kept.value

    def slab(self, k: int):
        """-> (the slab's whole allocation as bytes, offset of its data in it, used bytes, capacity)."""
        off, used, cap = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.cl_store_slab(self._h, int(k), None, 0, C.byref(off), C.byref(used), C.byref(cap)))
        buf = np.zeros(cap.value + (0 if self.device < 0 else off.value + 16), np.uint8)
        self._check(self.lib.cl_store_slab(self._h, int(k), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(off), C.byref(used), C.byref(cap)))
        return buf, off.value, used.value, cap.value

    def close(self):
        if self._h is not None:
            self.lib.cl_store_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


@dataclass
class BamSource:
    """What ``ResidentRecords.from_bam`` reads instead of a candidate file (``--train_bam`` / ``--test_bam`` beside it)."""
    bam: str
    fasta: str
    locations: list                      # ``pileup_encoder.Location``s, in the order the converter would write their records
    inflate_device: Optional[str] = None
    encoder_options: object = None       # ``pileup_encoder.EncoderOptions``; None = what ``--test_bam`` uses
    threads: int = 0


class _RecordTexts:
    """``vcfrec`` of the records of a blob array, decoded when asked for."""

    def __init__(self, blob):
        self.vcfrec = blob["vcfrec"]

    def __getitem__(self, i):
        return bytes(self.vcfrec[i]).decode()


class ResidentRecords:
    """A candidate file resident on the device (``--train-cache-device gpu``): ``_fill_from_file`` inflates every chunk of the file once, in
    groups of ``group_chunks`` through a ``DeviceChunkLoader``'s handle (``cl_inflate_chunks_device``), appends each group's records
    to a ``RecordStore`` (trimmed of their trailing all-zero rows: 0.36 of the inflated bytes on the synthetic 100-read records measured; a sixth is the
    estimate for a 30x pileup, not measured) and keeps every
    record's non-plane members (3 365 bytes a record) in one host array; then it closes the inflate handle and the file.  From
    then on ``assemble_list`` is ``DeviceChunkLoader.assemble_list`` with the record indices as the slots and the store as the
    source: no file read, no upload, no inflate launch.

    The whole file is resident or the fill ends with ``StoreFull`` (how many records fit, in how many bytes, the budget); a damaged
    chunk ends it with ``DamagedChunk`` wherever it lies.

    ``ResidentRecords.from_bam`` (a ``BamSource`` as the source) fills the same store from the GPU pileup encoder instead
    (``_fill_from_bam``, ``--train_bam``): no file at all."""

    def __init__(self, source, reads: int, batch_sites: int, device: int = 0, use_q: bool = True, use_strand: bool = True,
                 capacity_bytes=0, slab_bytes: int = STORE_SLAB_BYTES, group_chunks: int = FILL_GROUP_CHUNKS, stream: int = 0,
                 debug_fill: Optional[int] = None, round_locations: int = FILL_ROUND_LOCATIONS, record_format: str = "rows"):
        """``source``: the candidate file's path (``group_chunks`` is its fill's option), or a ``BamSource`` (``round_locations`` is;
        see ``from_bam``).  ``debug_fill`` (tests): every slab is filled with this byte before anything is packed.
        ``record_format``: ``RecordStore``'s (``--train-cache-format``); the batches are the same."""
        self._inflater = self.store = self._counts = self.torch = None
        self.record_format = record_format
        bam = source if isinstance(source, BamSource) else None
        self.path, self.reads, self.B = bam.bam if bam else source, int(reads), int(batch_sites)
        self.use_q, self.use_strand, self.device = use_q, use_strand, int(device)
        if bam:
            from .location_round import default_encoder_options
            opt = bam.encoder_options or default_encoder_options()
            self.window, self.stored_rows = 2 * opt.window_size + 1, opt.max_reads
            if self.window != 201:
                raise ValueError("the encoder gives windows of %d columns: the allele masks are defined on the 201-column window (window size "
                                 "100)" % self.window)
            if self.reads > self.stored_rows:
                raise ValueError("the model reads %d rows per site but the encoder stores only %d" % (self.reads, self.stored_rows))
        else:
            with RawChunkFile(source) as f:
                n_chunks, chunk = -(-len(f) // f.chunk), f.chunk
            group = max(1, min(int(group_chunks), n_chunks))
            # (a sequential handle for ``group`` whole chunks at a time; it knows the file's layout)
            self._inflater = DeviceChunkLoader(source, reads, batch_sites=group * chunk, device=device, use_q=use_q, use_strand=use_strand)
            self.window, self.stored_rows = self._inflater.window, self._inflater.stored_rows
        if self.device >= 0:
            import torch
            self.torch = torch
        self.blob_dtype = blob_dtype(self.window)
        self.n, self.blob, self.capacity_bytes, self.stage = 0, None, 0, {}
        self.inflated_bytes = self._num_reads = self._ref_bases = self._label = None          # (``_filled``)
        try:
            self.lib = load_library()
            if bam:
                self._fill_from_bam(bam, opt, capacity_bytes, slab_bytes, stream, debug_fill, round_locations)
            else:
                self._fill_from_file(n_chunks, group, capacity_bytes, slab_bytes, stream, debug_fill)
        except Exception:
            self.close()
            raise

    @classmethod
    def from_bam(cls, bam: str, fasta: str, locations, reads: int, batch_sites: int, device: int = 0, use_q: bool = True,
                 use_strand: bool = True, capacity_bytes=0, slab_bytes: int = STORE_SLAB_BYTES, stream: int = 0,
                 debug_fill: Optional[int] = None, encoder_options=None, inflate_device: Optional[str] = None, threads: int = 0,
                 round_locations: int = FILL_ROUND_LOCATIONS, record_format: str = "rows", subsample=None):
        """The resident records of a BAM (``--train_bam``): what ``tools/convert_bam_single_reads.py`` would write for ``locations``
        (``pileup_encoder.Location``s, in the converter's order) and ``ResidentRecords(path)`` would then inflate, without the file
        (``_fill_from_bam``).

        ``capacity_bytes``: the budget, or a function that gives it -- called once the staging planes (3 x ``round_locations`` x
        ``max_reads`` x window bytes) are allocated, so that a budget taken from the free device memory does not count them.
        ``device < 0``: the CPU definition -- ``pe_encode`` for every location, a host store, ``cl_store_pack_planes_host``; no GPU.

        ``stage`` also holds the encoders' counts (``location_round.ENCODER_COUNTS``) and ``encode_ms``.

        ``subsample=(fraction, seed)``: every encoder of the fill drops the reads ``bamio.SampleRule`` drops (it is
        ``encoder_options.subsample`` for this store): the records are those of the BAM ``tools/subsample_bam.py`` writes."""
        if subsample is not None:
            from .location_round import default_encoder_options, with_subsample
            encoder_options = with_subsample(encoder_options or default_encoder_options(), subsample)
        return cls(BamSource(bam, fasta, locations, inflate_device, encoder_options, threads), reads, batch_sites, device, use_q,
                   use_strand, capacity_bytes, slab_bytes, stream=stream, debug_fill=debug_fill, round_locations=round_locations,
                   record_format=record_format)

    def _open_store(self, n_records: int, capacity_bytes: int, slab_bytes: int, debug_fill: Optional[int]) -> None:
        self.capacity_bytes = int(capacity_bytes)
        self.store = RecordStore(self.window, self.stored_rows, n_records, self.capacity_bytes, slab_bytes, self.device, self.record_format)
        if debug_fill is not None:
            self.store.debug_fill(debug_fill)

    def __len__(self):
        return self.n

    def _fill_from_file(self, n_chunks: int, group: int, capacity_bytes: int, slab_bytes: int, stream: int, debug_fill) -> None:
        """Every chunk of the file through the inflate handle, ``group`` at a time, into the store; then the handle and the file go."""
        dl, f = self._inflater, self._inflater.file
        self.n = len(dl)
        self.blob = np.zeros(self.n, self.blob_dtype)
        self._open_store(self.n, capacity_bytes, slab_bytes, debug_fill)
        self.stage.update(dl.stage)
        self.stage.update(counts_ms=0.0, fill_ms=0.0, store_bytes=0, store_records=0, extent_ms=0.0, pack_ms=0.0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        t_fill = time.perf_counter()
        for c0 in range(0, n_chunks, group):
            c1 = min(n_chunks, c0 + group)
            n = c1 - c0
            t0 = time.perf_counter()
            total, offs, sizes, raw = dl._read_chunks(c0, c1)
            self.stage["read_ms"] += (time.perf_counter() - t0) * 1e3
            blob_p = C.c_void_p()
            status = np.zeros(n, np.int32)
            dl._check(dl.lib.cl_inflate_chunks_device(dl._h, C.c_void_p(dl._comp.data_ptr()), total, p(offs), p(sizes), p(raw), n,
                                                      C.c_void_p(stream or None), C.byref(blob_p), p(status)), "cl_inflate_chunks_device")
            bad = np.flatnonzero(status)
            if len(bad):
                from . import zinflate
                raise DamagedChunk("%s: chunk at record %d: %s" % (f.path, (c0 + int(bad[0])) * f.chunk, zinflate.status_text(status[bad[0]])))
            r0 = c0 * f.chunk
            n_rec = min(self.n, c1 * f.chunk) - r0               # (the padding of the edge chunk is not a record)
            blob = np.ctypeslib.as_array(C.cast(blob_p, C.POINTER(C.c_uint8)), (n * f.chunk * self.blob_dtype.itemsize,)).view(self.blob_dtype)
            self.blob[r0:r0 + n_rec] = blob[:n_rec]
            st = Stats()
            dl._check(dl.lib.cl_get_stats(dl._h, C.byref(st)), "cl_get_stats")
            for k, _t in Stats._fields_:
                if k != "assemble_ms":
                    self.stage[k] += getattr(st, k)
            slots = np.arange(n_rec, dtype=np.int32)
            try:
                self.store.append_device(dl._h, slots, r0 + slots, stream)
            except StoreFull:
                have = self.store.stats()                   # (the library counted what of the refused group would fit)
                raise StoreFull("%s does not fit the record store: %d of its %d records fit, in %d bytes of the budget of %d bytes; raise "
                                "--train-cache-bytes or drop --train-cache-device"
                                % (f.path, have.records + have.refused_fit_records, self.n, have.refused_fit_bytes, self.capacity_bytes)) from None
        # the inflate handle's record buffer and the file go: every batch from here on comes from the store
        self._inflater.close()
        self._inflater = None
        self._filled(t_fill)

    def _filled(self, t_fill: float) -> None:
        """What both fills end with: the store's figures and the members every plan reads."""
        have = self.store.stats()
        self.stage.update(store_bytes=have.stored_bytes, store_records=have.records, extent_ms=have.extent_ms, pack_ms=have.pack_ms)
        by = self.store.format_stats()
        self.stage.update(store_rows_records=by.rows_records, store_rows_bytes=by.rows_bytes, store_compact_records=by.compact_records,
                          store_compact_bytes=by.compact_bytes, spans_ms=by.spans_ms)
        self.inflated_bytes = have.inflated_bytes
        # contiguous once (a field of the blob array is a strided view)
        self._num_reads = np.ascontiguousarray(self.blob["num_reads"].reshape(-1))
        self._ref_bases = np.ascontiguousarray(self.blob["ref_bases"].reshape(self.n, self.window))
        self._label = np.ascontiguousarray(self.blob["label"].reshape(-1)) if "label" in self.blob_dtype.names else np.zeros(self.n, np.uint8)
        self.stage["fill_ms"] = (time.perf_counter() - t_fill) * 1e3

    def _fill_from_bam(self, src: BamSource, opt, capacity_bytes, slab_bytes: int, stream: int, debug_fill, round_locations: int) -> None:
        """Per round of ``round_locations`` locations: the location round (``location_round.LocationRounds.encode``) leaves the planes
        of every location that gives a record in its slot of three staging arrays; those locations are the records, in input order,
        and their slots go into the store (``cl_store_append_planes_device``: the same extent and pack kernels as the file fill,
        reading the planes where the encoder left them); their other members (``hdf5_schema.blob_dtype``, the texts cut as the file
        cuts them) are appended to the host array the plans read.  Afterwards the encoders are closed and the staging is freed."""
        from .location_round import ENCODER_COUNTS, LocationRounds, record_members
        locations = list(src.locations)
        self.stage.update({k: 0.0 for k in ("plan_ms", "assemble_ms", "counts_ms", "fill_ms", "encode_ms", "extent_ms", "pack_ms")})
        self.stage.update({k: 0 for k in ("records", "store_bytes", "store_records") + ENCODER_COUNTS})
        B = max(1, min(int(round_locations), len(locations)))
        ts = None
        if self.device >= 0:
            dev = self.torch.device("cuda", self.device)
            ts = self.torch.cuda.ExternalStream(stream, device=dev) if stream else self.torch.cuda.current_stream(dev)
        rounds = LocationRounds(src.bam, src.fasta, opt, B, self.device, inflate_device=src.inflate_device, threads=src.threads, stream=ts,
                                counts=self.stage)
        try:
            # (the budget is asked for now that the staging planes are allocated; the table's size is an upper bound: a location
            # without a record leaves no hole among the records)
            self._open_store(len(locations), capacity_bytes() if callable(capacity_bytes) else capacity_bytes, slab_bytes, debug_fill)
            blobs = [np.zeros(0, self.blob_dtype)]
            t_fill = time.perf_counter()
            for l0 in range(0, len(locations), B):
                locs = locations[l0:l0 + B]
                t0 = time.perf_counter()
                ref, num, status = rounds.encode(locs)
                self.stage["encode_ms"] += (time.perf_counter() - t0) * 1e3
                keep = np.flatnonzero(status == 1).astype(np.int32)
                m = len(keep)
                records = self.n + np.arange(m, dtype=np.int32)
                try:
                    if self.device >= 0:
                        self.store.append_planes_device([t.data_ptr() for t in rounds.stored], len(locs), keep, records, ts.cuda_stream)
                    else:
                        self.store.pack_planes_host(*[a[:len(locs)] for a in rounds.stored], keep, records)
                except StoreFull:
                    have = self.store.stats()
                    raise StoreFull("the records of %s do not fit the record store: %d records (of the first %d of its %d locations) fit, in "
                                    "%d bytes of the budget of %d bytes; raise --train-cache-bytes"
                                    % (src.bam, have.records + have.refused_fit_records, l0 + len(locs), len(locations),
                                       have.refused_fit_bytes, self.capacity_bytes)) from None
                blobs.append(record_members(locs, keep, ref, num, self.blob_dtype))
                self.n += m
            self.blob = np.concatenate(blobs)
            self._filled(t_fill)
        finally:
            # the encoder's buffers, the host encoders' files and the staging planes go: every batch comes from the store
            rounds.close()

    def chromosomes(self):
        """The text before the first tab of every record's ``vcfrec``: what ``inference.select_sites`` holds out by."""
        return [bytes(v).split(b"\t", 1)[0].decode() for v in self.blob["vcfrec"]]

    def assemble_list(self, indices, seed: int, outs, stream: int = 0, downsample_rate: float = 0.0,
                      downsample_prob: float = 0.0) -> IndexedSites:
        """``DeviceChunkLoader.assemble_list`` from the store: site i is record ``indices[i]`` of the file.  A host store
        (``device < 0``) takes six numpy arrays as ``outs`` and assembles and counts on the host."""
        torch = self.torch
        idx = np.asarray(indices, np.int64).reshape(-1)
        m = len(idx)
        if m > self.B:
            raise ValueError("%d indices: at most %d per call" % (m, self.B))
        if m and (idx.min() < 0 or idx.max() >= self.n):
            raise ValueError("record indices %d..%d outside the file's %d records" % (idx.min(), idx.max(), self.n))
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        t2 = time.perf_counter()
        slots = idx.astype(np.int32)
        plan = plan_records(slots, idx, self._num_reads, self._ref_bases, _RecordTexts(self.blob), self.reads, self.stored_rows, seed,
                            downsample_rate, downsample_prob)
        label = np.array(self._label[slots])
        t3 = time.perf_counter()
        counts = np.zeros((m, 2, 16), np.int32)
        if m and self.device < 0:
            # the CPU definition: ``outs`` are six numpy arrays with room for the m sites
            first = np.ascontiguousarray(plan.first_rows, np.uint8)
            rows = np.ascontiguousarray(plan.rows, np.int16) if not first.all() else None
            got = self.store.assemble_host(plan.slots, rows, first, self.reads, (plan.ref, plan.ref_mask, plan.var_mask), self.use_q,
                                           self.use_strand)
            for dst, src in zip(outs, got):
                dst[:m] = src
            counts[:] = center_counts_host(got[0])
        elif m:
            first = np.ascontiguousarray(plan.first_rows, np.uint8)
            rows = np.ascontiguousarray(plan.rows, np.int16) if not first.all() else None
            self.store.assemble_device(plan.slots, rows, first, self.reads, (plan.ref, plan.ref_mask, plan.var_mask), self.use_q,
                                       self.use_strand, outs, stream)
            if self._counts is None:
                dev = torch.device("cuda", self.device)
                self._counts = (torch.empty((self.B, 2, 16), dtype=torch.int32, device=dev),
                                torch.empty((self.B, 2, 16), dtype=torch.int32).pin_memory())
            d_counts, h_counts = self._counts
            self.store._check(self.lib.cl_store_center_counts_device(self.store._h, v(outs[0]), m, self.reads, self.window,
                                                                     v(d_counts.data_ptr()), v(stream)))
            ts = torch.cuda.ExternalStream(stream, device=d_counts.device) if stream else torch.cuda.default_stream(d_counts.device)
            with torch.cuda.stream(ts):
                h_counts[:m].copy_(d_counts[:m], non_blocking=True)
            ts.synchronize()
            counts[:] = h_counts[:m].numpy()
            self.stage["assemble_ms"] += self.store.stats().assemble_ms
        t4 = time.perf_counter()
        self.stage["plan_ms"] += (t3 - t2) * 1e3
        self.stage["counts_ms"] += (t4 - t3) * 1e3
        self.stage["records"] += m
        return IndexedSites(plan, label, counts)

    def close(self):
        if self._inflater is not None:
            self._inflater.close()
            self._inflater = None
        if self.store is not None:
            self.store.close()
            self.store = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
