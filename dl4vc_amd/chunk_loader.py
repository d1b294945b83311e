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
import time
from typing import Optional

import numpy as np

from . import pileup_gpu
from .hdf5_schema import PLANE_FIELDS, blob_dtype
from .hdf5io import RawChunkFile
from .site_assembly import SitePlan, plan_sites

CL_SYMBOLS = ("cl_open", "cl_close", "cl_last_error", "cl_inflate_chunks_device", "cl_assemble_device", "cl_get_stats")
_bound = None


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
        _bound = lib
    return _bound


class DamagedChunk(ValueError):
    """A chunk of the file does not inflate: ``chunk at record N: <status text>``."""


class DeviceChunkLoader:
    """Records ``[lo, hi)`` of a candidate file, ``batch_sites`` at a time, as planes in device memory.

    ``load(b0, b1, outs, stream)`` inflates the chunks that cover ``[b0, b1)`` (the range need not be chunk-aligned; the records
    of those chunks outside it, and the padding of an edge chunk, are never planned), and assembles the records' sites into
    ``outs`` -- six device addresses (reads, qual, strand ``[m][reads][window]``, ref, ref_mask, var_mask ``[m][window]``).
    Record ``i`` of the file draws the read subset of a deep pileup with ``seed + i``, whatever the range.

    Device memory: the inflated records, ``(batch_sites + 2 * chunk - 1) * record_bytes`` rounded up to chunks (512 MB at 4096
    sites of the production layout), and the compressed chunks."""

    def __init__(self, path: str, reads: int, batch_sites: int = 4096, seed: int = 0, device: int = 0, use_q: bool = True,
                 use_strand: bool = True):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("the device loader needs a HIP device visible to torch; there is no CPU path (NativeLoader is it)")
        self.torch = torch
        self.file = RawChunkFile(path)
        self._h = None
        try:
            f = self.file
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
            self.window, self.stored_rows, self.reads, self.B = W, S, int(reads), int(batch_sites)
            self.seed, self.use_q, self.use_strand, self.device = seed, use_q, use_strand, device
            self.blob_dtype = blob_dtype(W)
            self.lib = load_library()
            h = C.c_void_p()
            offs = (C.c_int64 * 3)(*p)
            if self.lib.cl_open(f.itemsize, f.chunk, W, S, offs, self.B + f.chunk, int(device), C.byref(h)) != 0:
                raise RuntimeError("cl_open failed: %s" % self.lib.cl_last_error(None).decode())
            self._h = h
            if self.blob_dtype.itemsize != f.itemsize - 3 * S * W:
                raise ValueError("%s: records of %d bytes do not match the schema" % (path, f.itemsize))
            # pinned staging of the raw chunks, grown on demand
            self._comp = torch.empty(0, dtype=torch.uint8)
            self.stage = {k: 0.0 for k in ("read_ms", "upload_ms", "inflate_ms", "blob_copy_back_ms", "plan_ms", "assemble_ms")}
            self.stage.update({k: 0 for k in ("chunks", "compressed_bytes", "inflated_bytes", "raw_chunks", "records")})
        except Exception:
            self.close()
            raise

    def __len__(self):
        return len(self.file)

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, self.lib.cl_last_error(self._h).decode()))

    def _read_chunks(self, c0: int, c1: int):
        """The raw chunks [c0, c1) into pinned memory -> (buffer, offsets, sizes, raw flags)."""
        f, torch = self.file, self.torch
        sizes = np.array([f.stored_size(c) for c in range(c0, c1)], np.uint64)
        offs = np.zeros(len(sizes), np.uint64)
        offs[1:] = np.cumsum((sizes[:-1] + np.uint64(15)) & ~np.uint64(15))     # every chunk at a 16-byte boundary
        total = int(offs[-1] + sizes[-1]) if len(sizes) else 0
        if self._comp.numel() < total:
            self._comp = torch.empty(total + total // 4 + 4096, dtype=torch.uint8).pin_memory()
        base = self._comp.data_ptr()
        raw = np.zeros(len(sizes), np.uint8)
        for k, c in enumerate(range(c0, c1)):
            raw[k] = f.read_chunk(c, base + int(offs[k])) & 1
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
