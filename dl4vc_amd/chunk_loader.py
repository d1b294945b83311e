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
              "cl_center_counts_device", "cl_center_counts_host")
_bound = None
# libhdf5 is not thread-safe: the raw chunk reads of every loader of the process (the training file's and the test file's workers)
# take this lock, so at most one thread is inside the library
HDF5_LOCK = threading.Lock()


class Stats(C.Structure):
    """``cl_stats``."""
    _fields_ = [(n, C.c_double) for n in ("upload_ms", "inflate_ms", "blob_copy_back_ms", "assemble_ms")] + \
               [(n, C.c_int64) for n in ("chunks", "compressed_bytes", "inflated_bytes", "raw_chunks")]


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

    def load_indices(self, indices, seed: int, outs, stream: int = 0) -> IndexedSites:
        """The records at ``indices`` -- absolute record indices in any order, at most ``batch_sites`` -- as the sites of ``outs``
        in that order: site i is record ``indices[i]`` and draws the subset of a deep pileup with ``seed + indices[i]``
        (``train_data.assemble_training_batch``'s rule).  Every distinct chunk an index falls in is read once, in ascending
        chunk order, and inflated on the device; two indices of one chunk share it.  After the assembly the reads plane's centre
        tokens are counted (``cl_center_counts_device``) for the targets.  Everything is enqueued on ``stream`` and waited for:
        the planes are complete when the call returns.  The handle must have been opened with ``shuffled``.
        = ``inflate_lists([indices])`` + ``assemble_list(indices)``."""
        self.inflate_lists([indices], stream)
        return self.assemble_list(indices, seed, outs, stream)

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

    def assemble_list(self, indices, seed: int, outs, stream: int = 0) -> IndexedSites:
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
                            self.reads, self.stored_rows, seed)
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
