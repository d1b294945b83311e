"""ctypes binding of libdl4vc_pileup.so (``include/dl4vc_pileup_gpu.h``): the pileup encoder of ``loader.NativePileupEncoder``
(``pe_*``) with the record planes built on the GPU.

Status per location: 1 = planes byte-identical to ``pe_encode``'s, 0 = no record (only where ``pe_encode`` also gives 0),
2 = declined -- ``pileup_encoder.encode_locations(device="gpu")`` hands those to ``pe_encode`` and what that declines to the
Python encoder."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .loader import PileupOptions

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libdl4vc_pileup.so")
SYMBOLS = ("pg_open", "pg_encode", "pg_encode_device", "pg_assemble_device", "pg_close", "pg_last_error",
           "pg_set_inflate_device", "pg_get_stats", "pg_debug_run_records", "pg_compress_records_device", "pg_set_compress_codes",
           "pg_census", "pg_set_subsample", "pg_get_subsample_stats", "pg_set_read_filter", "pg_set_read_stats", "pg_get_read_stats")
# the zlib compressor of the same library (csrc/zdeflate.h)
ZD_SYMBOLS = ("zd_bound", "zd_deflate_host", "zd_deflate", "zd_deflate_host_flags", "zd_code_lengths_host")
ZD_MIN_SEGMENT, ZD_MAX_SEGMENT, ZD_DEFAULT_SEGMENT = 1024, 32768, 16384
ZD_REVERSED, ZD_RAW_ON_STORE, ZD_DYNAMIC = 1, 2, 4
COMPRESS_CODES = {"fixed": 0, "dynamic": 1}          # pg_set_compress_codes' modes
MAX_TRACKS = 1024            # PG_MAX_TRACKS
MAX_WINDOW = 100             # PG_MAX_WINDOW
_lib = None


class Stats(C.Structure):
    """``pg_stats``: the stages of the last ``pg_encode`` / ``pg_encode_device`` call (times in ms)."""
    _fields_ = [(n, C.c_double) for n in ("host_frame_ms", "read_ms", "upload_ms", "inflate_ms", "frame_ms", "encode_ms", "copy_back_ms",
                                          "census_ms")] + \
               [(n, C.c_int64) for n in ("host_records", "blocks", "compressed_bytes", "inflated_bytes", "records", "groups")] + \
               [(n, C.c_double) for n in ("pack_ms", "deflate_ms", "gather_ms", "compress_copy_back_ms")] + \
               [(n, C.c_int64) for n in ("chunks", "raw_bytes", "chunk_bytes_out", "stored_chunks", "fixed_segments", "dynamic_segments",
                                         "stored_segments")]


class SubsampleStats(C.Structure):
    """``pg_subsample_stats``: records in front of the sample rule and behind it, of the last call."""
    _fields_ = [("records_seen", C.c_int64), ("records_kept", C.c_int64)]


class RecView(C.Structure):
    """``pg_rec_view``: one framed record of ``pg_debug_run_records``."""
    _fields_ = [(n, C.c_int32) for n in ("pos", "end", "res", "l_seq")] + \
               [(n, C.c_uint32) for n in ("cigar_off", "seq_off", "qual_off", "n_cig", "l_name", "bits")] + [("bytes_hash", C.c_uint64)]


def _bind_debug(lib):
    lib.pg_debug_run_records.argtypes = [C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_int, C.POINTER(RecView), C.c_int64,
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.pg_last_error.argtypes = [C.c_void_p]
    lib.pg_last_error.restype = C.c_char_p


def debug_run_records(bam_path: str, bai_path: str, tid: int, s0: int, stop: int, path: int, lib=None):
    """``pg_debug_run_records`` -> (list of field tuples, max_nref, sorted); no GPU is touched.  ``path`` 0: the host framing, 1: the
    CPU twin of the device path.  ``lib``: another build of the entry point (the sanitizer build)."""
    if lib is None:
        lib = load_library()
    else:
        _bind_debug(lib)
    n, mx, srt = C.c_int64(0), C.c_int64(0), C.c_int32(0)
    cap = 1 << 12
    while True:
        buf = (RecView * cap)()
        rc = lib.pg_debug_run_records(bam_path.encode(), bai_path.encode(), tid, s0, stop, path, buf, cap, C.byref(n), C.byref(mx), C.byref(srt))
        if rc != 0:
            raise RuntimeError("pg_debug_run_records failed: %s" % lib.pg_last_error(None).decode())
        if n.value <= cap:
            break
        cap = n.value
    names = [f[0] for f in RecView._fields_]
    return [tuple(getattr(buf[i], k) for k in names) for i in range(n.value)], mx.value, bool(srt.value)


def available() -> bool:
    return os.path.isfile(LIB_PATH)


def load_library() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError("%s is not built (make -C dl4vc_amd/csrc)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        vp = C.c_void_p
        lib.pg_open.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(PileupOptions), C.c_int32, C.POINTER(vp)]
        lib.pg_encode.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
        lib.pg_encode_device.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp]
        lib.pg_census.argtypes = [vp, vp, vp, C.c_int64, vp, vp]
        lib.pg_assemble_device.argtypes = ([vp] * 4 + [C.c_int64, C.c_int32, C.c_int32] + [vp] * 3 + [C.c_int64, C.c_int32] + [vp] * 3 +
                                           [C.c_int32, C.c_int32] + [vp] * 6 + [vp])
        lib.pg_set_inflate_device.argtypes = [vp, C.c_int, C.c_uint64]
        lib.pg_get_stats.argtypes = [vp, C.POINTER(Stats)]
        lib.pg_set_subsample.argtypes = [vp, C.c_double, C.c_uint32]
        lib.pg_get_subsample_stats.argtypes = [vp, C.POINTER(SubsampleStats)]
        from .read_filter import ReadStats
        lib.pg_set_read_filter.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32]
        lib.pg_set_read_stats.argtypes = [vp, C.c_int]
        lib.pg_get_read_stats.argtypes = [vp, C.POINTER(ReadStats)]
        lib.pg_compress_records_device.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int64, C.c_int32, C.POINTER(vp), vp, vp, vp, vp, vp]
        lib.zd_bound.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        lib.zd_deflate_host.argtypes = [vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_int32)]
        lib.zd_deflate_host_flags.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_int32, vp, C.c_uint64, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
        lib.zd_code_lengths_host.argtypes = [vp, C.c_int32, C.c_int32, vp]
        lib.pg_set_compress_codes.argtypes = [vp, C.c_int]
        lib.zd_deflate.argtypes = [vp, C.c_uint64, C.c_int64, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp, vp, vp, vp]
        _bind_debug(lib)
        lib.pg_close.argtypes = [vp]
        lib.pg_close.restype = None
        lib.pg_last_error.argtypes = [vp]
        lib.pg_last_error.restype = C.c_char_p
        _lib = lib
    return _lib


def _zd_check(lib, rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, lib.pg_last_error(None).decode()))


def zd_bound(n: int, segment: int = ZD_DEFAULT_SEGMENT) -> int:
    """``zd_bound``: no stream of ``n`` input bytes is longer."""
    lib = load_library()
    b = C.c_uint64(0)
    _zd_check(lib, lib.zd_bound(int(n), int(segment), C.byref(b)), "zd_bound")
    return b.value


def _codes_mode(codes: str) -> int:
    if codes not in COMPRESS_CODES:
        raise ValueError("codes: 'fixed' or 'dynamic', not %r" % (codes,))
    return COMPRESS_CODES[codes]


def zd_code_lengths(freq, limit: int = 15):
    """``zd_code_lengths_host``: the compressor's code construction, counts -> code lengths of at most ``limit`` bits."""
    lib = load_library()
    f = np.ascontiguousarray(freq, np.uint32)
    lens = np.zeros(f.size, np.uint8)
    _zd_check(lib, lib.zd_code_lengths_host(f.ctypes.data_as(C.c_void_p), f.size, int(limit), lens.ctypes.data_as(C.c_void_p)),
              "zd_code_lengths_host")
    return lens


def zd_deflate_host(data, segment: int = ZD_DEFAULT_SEGMENT, codes: str = "fixed"):
    """``zd_deflate_host`` (``codes="dynamic"``: ``zd_deflate_host_flags`` with ``ZD_DYNAMIC``) -> (the zlib stream as bytes,
    Adler-32, store): the CPU twin of the device compressor.  ``store``: the stream is not smaller than ``data`` (it is still a
    valid stream within ``zd_bound``)."""
    if _codes_mode(codes):
        return zd_deflate_host_flags(data, segment, ZD_DYNAMIC)
    lib = load_library()
    src = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    out = np.empty(zd_bound(src.size, segment), np.uint8)
    size, adler, store = C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
    _zd_check(lib, lib.zd_deflate_host(src.ctypes.data_as(C.c_void_p) if src.size else None, src.size, int(segment),
                                       out.ctypes.data_as(C.c_void_p), out.size, C.byref(size), C.byref(adler), C.byref(store)),
              "zd_deflate_host")
    return out[:size.value].tobytes(), adler.value, bool(store.value)


def zd_deflate_host_flags(data, segment: int = ZD_DEFAULT_SEGMENT, flags: int = 0):
    """``zd_deflate_host_flags`` -> as ``zd_deflate_host``; ``flags``: 0 or ``ZD_DYNAMIC``."""
    lib = load_library()
    src = np.frombuffer(data, np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    out = np.empty(zd_bound(src.size, segment), np.uint8)
    size, adler, store = C.c_uint64(0), C.c_uint32(0), C.c_int32(0)
    _zd_check(lib, lib.zd_deflate_host_flags(src.ctypes.data_as(C.c_void_p) if src.size else None, src.size, int(segment), int(flags),
                                             out.ctypes.data_as(C.c_void_p), out.size, C.byref(size), C.byref(adler), C.byref(store)),
              "zd_deflate_host_flags")
    return out[:size.value].tobytes(), adler.value, bool(store.value)


def zd_deflate_device(in_ptr: int, chunk_bytes: int, n_chunks: int, out_ptr: int, out_cap: int, segment: int = ZD_DEFAULT_SEGMENT,
                      flags: int = 0, stream: int = 0):
    """``zd_deflate``: ``n_chunks`` streams of the device buffer at ``in_ptr`` into the device buffer at ``out_ptr`` ->
    (offsets, sizes u64, adlers u32, store u8), host arrays, one entry per chunk.  ``flags``: ``ZD_REVERSED | ZD_RAW_ON_STORE |
    ZD_DYNAMIC``."""
    lib = load_library()
    offs, sizes = np.zeros(n_chunks, np.uint64), np.zeros(n_chunks, np.uint64)
    adlers, store = np.zeros(n_chunks, np.uint32), np.zeros(n_chunks, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    _zd_check(lib, lib.zd_deflate(C.c_void_p(in_ptr), int(chunk_bytes), int(n_chunks), int(segment), int(flags), C.c_void_p(out_ptr),
                                  int(out_cap), p(offs), p(sizes), p(adlers), p(store), C.c_void_p(stream or None)), "zd_deflate")
    return offs, sizes, adlers, store


class CompressedChunks:
    """Chunks of the candidate dataset as ``hdf5io.ChunkWriter.write_chunks`` takes them: ``n_records`` records in
    ``len(sizes)`` chunks; chunk ``c`` is ``data[offsets[c]:offsets[c] + sizes[c]]`` -- its zlib stream, or its raw bytes where
    ``store[c]`` is set."""

    def __init__(self, n_records, data, offsets, sizes, adlers, store):
        self.n_records, self.data, self.offsets, self.sizes, self.adlers, self.store = n_records, data, offsets, sizes, adlers, store

    def __len__(self):
        return len(self.sizes)

    def chunk(self, c: int) -> bytes:
        o = int(self.offsets[c])
        return self.data[o:o + int(self.sizes[c])].tobytes()


class GpuPileupEncoder:
    """Image planes of a list of locations, in input order; the same outputs as ``loader.NativePileupEncoder.encode``."""

    def __init__(self, bam_path: str, fasta_path: str, window_size: int, max_reads: int, max_insert_length: int,
                 max_insert_length_variant: int, min_base_quality: int = 0, bai_path: Optional[str] = None, device: int = 0,
                 inflate_device: Optional[str] = None, max_inflated_bytes: int = 0, compress_codes: str = "fixed", subsample=None,
                 read_filter=None, read_stats: bool = False):
        """``read_filter=(exclude, require, min_mapq)``: reads are dropped by flags and mapping quality where the framing runs, in
        front of the sample rule (``pg_set_read_filter``, ``bamio.ReadFilter``); ``read_stats``: the read census is collected
        without a filter too (``pg_set_read_stats``); ``read_stats()`` gives it.
        ``subsample=(fraction, seed)``: reads are subsampled by name hash where the framing runs, on the host threads or in the
        device's frame kernel (``pg_set_subsample``, ``bamio.SampleRule``); ``subsample_stats()`` counts them.
        ``inflate_device="gpu"``: the BGZF blocks are inflated and the records framed on the device (``pg_set_inflate_device``;
        needs the ``.bai``), same outputs.  ``max_inflated_bytes``: inflated bytes per group of runs, 0 = the default.
        ``compress_codes``: ``"fixed"`` or ``"dynamic"``, the codes ``compress_records`` writes (``pg_set_compress_codes``)."""
        from .bamio import ReadFilter, SampleRule
        mode = _codes_mode(compress_codes)
        rule = SampleRule.of(subsample)
        flt = ReadFilter.of(read_filter)
        if inflate_device not in (None, "gpu"):
            raise ValueError("inflate_device: None or 'gpu', not %r" % (inflate_device,))
        self.lib = load_library()
        self._h = C.c_void_p()
        self.subsample = rule
        self.read_filter, self.collects = flt, bool(read_stats) or flt is not None
        self.window, self.max_reads, self.device = 2 * window_size + 1, max_reads, device
        opt = PileupOptions(window_size, max_reads, max_insert_length, max_insert_length_variant, min_base_quality)
        rc = self.lib.pg_open(bam_path.encode(), bai_path.encode() if bai_path else None, fasta_path.encode(), C.byref(opt),
                              int(device), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise RuntimeError("pg_open failed: %s" % self.lib.pg_last_error(None).decode())
        if mode:
            self._check(self.lib.pg_set_compress_codes(self._h, mode), "pg_set_compress_codes")
        try:
            if rule is not None:
                self.set_subsample(rule.fraction, rule.seed)
            if flt is not None:
                self.set_read_filter(*flt.as_tuple())
            if read_stats:
                self._check(self.lib.pg_set_read_stats(self._h, 1), "pg_set_read_stats")
            if inflate_device == "gpu":
                self.set_inflate_device(True, max_inflated_bytes)
        except RuntimeError:
            self.close()
            raise

    @classmethod
    def from_options(cls, bam, fasta, opt, device: int = 0, inflate_device: Optional[str] = None, compress_codes: str = "fixed"):
        """The encoder of a ``pileup_encoder.EncoderOptions``."""
        return cls(bam, fasta, opt.window_size, opt.max_reads, opt.max_insert_length, opt.max_insert_length_variant,
                   opt.min_base_quality, device=device, inflate_device=inflate_device, compress_codes=compress_codes,
                   subsample=getattr(opt, "subsample", None), read_filter=getattr(opt, "read_filter", None),
                   read_stats=getattr(opt, "read_stats", False))

    def set_read_filter(self, exclude: int = 0, require: int = 0, min_mapq: int = 0) -> None:
        """``pg_set_read_filter``; all zero turns it off again."""
        self._check(self.lib.pg_set_read_filter(self._h, int(exclude), int(require), int(min_mapq)), "pg_set_read_filter")

    def read_stats(self) -> dict:
        """The read census of the last ``encode`` / ``encode_device`` / ``census`` call (``read_filter.ReadStats.flat``): all zero
        unless a filter is on or the stats were asked for."""
        from .read_filter import ReadStats
        st = ReadStats()
        self._check(self.lib.pg_get_read_stats(self._h, C.byref(st)), "pg_get_read_stats")
        return st.flat()

    def set_subsample(self, fraction: float, seed: int = 0) -> None:
        """``pg_set_subsample``; fraction 0 turns it off again."""
        self._check(self.lib.pg_set_subsample(self._h, float(fraction), int(seed)), "pg_set_subsample")

    def subsample_stats(self) -> dict:
        """``records_seen`` / ``records_kept`` of the last ``encode`` / ``encode_device`` / ``census`` call."""
        st = SubsampleStats()
        self._check(self.lib.pg_get_subsample_stats(self._h, C.byref(st)), "pg_get_subsample_stats")
        return {"records_seen": st.records_seen, "records_kept": st.records_kept}

    def set_inflate_device(self, on: bool, max_inflated_bytes: int = 0) -> None:
        self._check(self.lib.pg_set_inflate_device(self._h, int(bool(on)), int(max_inflated_bytes)), "pg_set_inflate_device")

    def stats(self) -> dict:
        """The stages of the last ``encode`` / ``encode_device`` call (``pg_stats``)."""
        st = Stats()
        self._check(self.lib.pg_get_stats(self._h, C.byref(st)), "pg_get_stats")
        out = {n: getattr(st, n) for n, _ in Stats._fields_}
        if self.subsample is not None:                       # (only with the option: the stages stay pg_stats' otherwise)
            out.update(("subsample_" + k, v) for k, v in self.subsample_stats().items())
        if self.collects:
            out.update(self.read_stats())
        return out

    def _args(self, contigs: Sequence[str], positions):
        n = len(positions)
        names = (C.c_char_p * max(n, 1))(*[c.encode() for c in contigs])
        pos = np.ascontiguousarray(positions, np.int32)
        ref = np.zeros((n, self.window), np.uint8)
        num = np.zeros(n, np.int32)
        status = np.zeros(n, np.int8)
        return n, names, pos, ref, num, status

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, self.lib.pg_last_error(self._h).decode()))

    def encode(self, contigs: Sequence[str], positions):
        """-> (reads, qual, strand [n][max_reads][W] u8, ref [n][W] u8, num_reads [n] i32, status [n] i8), host arrays."""
        n, names, pos, ref, num, status = self._args(contigs, positions)
        reads, qual, strand = (np.zeros((n, self.max_reads, self.window), np.uint8) for _ in range(3))
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        self._check(self.lib.pg_encode(self._h, C.cast(names, C.c_void_p), p(pos), n, p(reads), p(qual), p(strand), p(ref),
                                       p(num), p(status)), "pg_encode")
        return reads, qual, strand, ref, num, status

    def encode_device(self, contigs: Sequence[str], positions, stream=None, out=None):
        """-> (reads, qual, strand: torch uint8 [n][max_reads][W] on the encoder's device, ref, num_reads, status: host).
        ``stream``: a ``torch.cuda.Stream`` the planes are ordered after (default: the current stream).  ``out``: three
        contiguous uint8 tensors on the encoder's device with room for n locations, written instead of new ones (their first
        n slots are returned)."""
        import torch
        n, names, pos, ref, num, status = self._args(contigs, positions)
        dev = torch.device("cuda", self.device)
        if out is not None:
            for x in out:
                if x.dtype != torch.uint8 or not x.is_contiguous() or x.device != dev or x.numel() < n * self.max_reads * self.window:
                    raise ValueError("out: three contiguous uint8 tensors on %s with room for %d locations" % (dev, n))
            reads, qual, strand = (x.view(-1)[:n * self.max_reads * self.window].view(n, self.max_reads, self.window) for x in out)
        else:
            reads, qual, strand = (torch.empty((n, self.max_reads, self.window), dtype=torch.uint8, device=dev) for _ in range(3))
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        t = lambda x: C.c_void_p(x.data_ptr() if x.numel() else None)   # noqa: E731
        self._check(self.lib.pg_encode_device(self._h, C.cast(names, C.c_void_p), p(pos), n, t(reads), t(qual), t(strand),
                                              p(ref), p(num), p(status), C.c_void_p(s.cuda_stream)), "pg_encode_device")
        return reads, qual, strand, ref, num, status

    def census(self, contigs: Sequence[str], positions, stream=None):
        """``pg_census`` -> status [n] i8 (host): exactly what ``encode_device`` returns as status, with no plane written."""
        import torch
        n, names, pos, _ref, _num, status = self._args(contigs, positions)
        s = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.device))
        self._check(self.lib.pg_census(self._h, C.cast(names, C.c_void_p), pos.ctypes.data_as(C.c_void_p), n,
                                       status.ctypes.data_as(C.c_void_p), C.c_void_p(s.cuda_stream)), "pg_census")
        return status

    def assemble_device(self, src_ptrs, n_slots: int, plan, out_ptrs, use_q: bool = True, use_strand: bool = True,
                        stream: int = 0, stored_rows: Optional[int] = None, window: Optional[int] = None) -> None:
        """``pg_assemble_device``: the stored planes at the device addresses ``src_ptrs`` (reads, qual, strand:
        ``[n_slots][stored_rows][window]``) -> the six planes of ``plan``'s sites (``site_assembly.SitePlan``) at the device
        addresses ``out_ptrs`` (reads, qual, strand, ref, ref_mask, var_mask), enqueued on ``stream`` (a raw hipStream_t, 0 = the
        default stream).  Asynchronous: the caller synchronises the stream."""
        m = len(plan)
        if m == 0:
            return
        R = plan.rows.shape[1]
        slots = np.ascontiguousarray(plan.slots, np.int32)
        first = np.ascontiguousarray(plan.first_rows, np.uint8)
        rows = np.ascontiguousarray(plan.rows, np.int16) if not first.all() else None
        lines = [np.ascontiguousarray(a, np.uint8) for a in (plan.ref, plan.ref_mask, plan.var_mask)]
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
        v = lambda x: C.c_void_p(int(x)) if x else None   # noqa: E731
        self._check(self.lib.pg_assemble_device(self._h, *[v(x) for x in src_ptrs], int(n_slots),
                                                int(stored_rows if stored_rows is not None else self.max_reads),
                                                int(window if window is not None else self.window), p(slots), p(rows), p(first), m, R,
                                                *[p(a) for a in lines], int(bool(use_q)), int(bool(use_strand)),
                                                *[v(x) for x in out_ptrs], v(stream)), "pg_assemble_device")

    def compress_records(self, planes, slots, blob: np.ndarray, records_per_chunk: int = 8, stream=None) -> CompressedChunks:
        """``pg_compress_records_device``: the records whose stored planes lie at ``slots`` of ``planes`` (the three device
        tensors ``encode_device`` returned) and whose other members are ``blob`` (``hdf5_schema.blob_dtype``, one entry per
        record) -> the dataset's chunks, packed and compressed on the device.  The last chunk is padded with zero records.
        The returned bytes are a copy: they stay valid after the next call."""
        import torch
        reads, qual, strand = planes
        n_slots = int(reads.shape[0])
        slots = np.ascontiguousarray(slots, np.int32)
        n = len(slots)
        blob = np.ascontiguousarray(blob)
        want = 149 + 16 * self.window
        if blob.dtype.itemsize != want or len(blob) != n:
            raise ValueError("blob: %d entries of %d bytes, not %d of %d" % (n, want, len(blob), blob.dtype.itemsize))
        for x in planes:
            if x.dtype != torch.uint8 or not x.is_contiguous() or tuple(x.shape) != (n_slots, self.max_reads, self.window):
                raise ValueError("planes: three contiguous uint8 tensors [%d][%d][%d]" % (n_slots, self.max_reads, self.window))
        nc = -(-n // records_per_chunk)
        offs, sizes = np.zeros(nc, np.uint64), np.zeros(nc, np.uint64)
        adlers, store = np.zeros(nc, np.uint32), np.zeros(nc, np.uint8)
        out = C.c_void_p()
        s = stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.device))
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        t = lambda x: C.c_void_p(x.data_ptr() if x.numel() else None)   # noqa: E731
        self._check(self.lib.pg_compress_records_device(self._h, t(reads), t(qual), t(strand), n_slots, p(slots), p(blob), n,
                                                        int(records_per_chunk), C.byref(out), p(offs), p(sizes), p(adlers), p(store),
                                                        C.c_void_p(s.cuda_stream)), "pg_compress_records_device")
        total = int(offs[-1] + sizes[-1]) if nc else 0
        data = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint8)), (total,)).copy() if total else np.zeros(0, np.uint8)
        return CompressedChunks(n, data, offs, sizes, adlers, store)

    def close(self):
        if self._h is not None:
            self.lib.pg_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
