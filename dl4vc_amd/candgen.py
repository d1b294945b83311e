"""ctypes binding of libdl4vc_cand.so (``include/dl4vc_candgen.h``): BAM + subregions -> per-subregion allele counts that
pass the frequency filter.  The host logic around it (regions, BED, groups, the multi-allele rule, VCF text) is
``dl4vc_amd/candidates.py``."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libdl4vc_cand.so")
MAX_ALLELE_LEN = 63          # CG_MAX_ALLELE_LEN
SYMBOLS = ("cg_open", "cg_run", "cg_last_error", "cg_close", "cg_n_refs", "cg_ref_name", "cg_ref_length",
           "cg_set_inflate_device", "cg_get_inflate_stats", "cg_debug_ranges", "cg_set_subsample", "cg_get_subsample_stats",
           "cg_set_read_filter", "cg_set_read_stats", "cg_get_read_stats",
           "cg_set_reference", "cg_get_reference_stats", "cg_reference_codes", "cg_reference_codes_host",
           "cg_set_left_align", "cg_get_left_align_stats", "cg_left_align_host",
           "bz_inflate", "bz_inflate_host", "bz_status_text", "bz_last_error")
INFLATE_DEVICES = ("gpu",)


class Options(C.Structure):
    _fields_ = [("threads", C.c_int32), ("max_len_indel_allele", C.c_int32), ("snp_min_freq", C.c_double),
                ("indel_min_freq", C.c_double), ("device", C.c_int32)]


class Region(C.Structure):
    _fields_ = [("tid", C.c_int32), ("start", C.c_int32), ("end", C.c_int32)]


class Candidate(C.Structure):
    _fields_ = [("region", C.c_int32), ("tid", C.c_int32), ("pos0", C.c_int32), ("depth", C.c_int32), ("count", C.c_int32),
                ("ref", C.c_char * (MAX_ALLELE_LEN + 1)), ("alt", C.c_char * (MAX_ALLELE_LEN + 1))]


class Stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("reads", "reads_no_md", "reads_no_pairs", "reads_unsupported", "reads_malformed",
                                         "reads_deletions_dropped", "allele_events", "alleles", "candidates", "batches")] + \
               [(n, C.c_double) for n in ("host_frame_ms", "upload_ms", "device_ms", "total_ms")]

    def as_dict(self) -> Dict[str, float]:
        return {n: getattr(self, n) for n, _ in self._fields_}


class InflateStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("blocks", "compressed_bytes", "inflated_bytes", "records")] + \
               [(n, C.c_double) for n in ("read_ms", "inflate_ms", "walk_frame_ms")]

    def as_dict(self) -> Dict[str, float]:
        return {n: getattr(self, n) for n, _ in self._fields_}


class ReferenceStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("reads", "contigs", "bases", "other_bytes")] + \
               [(n, C.c_double) for n in ("read_ms", "upload_convert_ms")]

    def as_dict(self) -> Dict[str, float]:
        return {n: getattr(self, n) for n, _ in self._fields_}


class LeftAlignStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("observations", "shifted", "bases_shifted", "clamped", "not_eligible")]

    def as_dict(self) -> Dict[str, int]:
        return {n: getattr(self, n) for n, _ in self._fields_}


class SubsampleStats(C.Structure):
    _fields_ = [("records_seen", C.c_int64), ("records_kept", C.c_int64)]


_lib = None


def load_library() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError("%s is not built (make -C dl4vc_amd/csrc)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.cg_open.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Options), C.POINTER(C.c_void_p)]
        lib.cg_run.argtypes = [C.c_void_p, C.POINTER(Region), C.c_int64, C.POINTER(C.POINTER(Candidate)), C.POINTER(C.c_int64),
                               C.POINTER(Stats)]
        lib.cg_last_error.restype = C.c_char_p
        lib.cg_close.argtypes = [C.c_void_p]
        lib.cg_n_refs.argtypes = [C.c_void_p]
        lib.cg_ref_name.argtypes = [C.c_void_p, C.c_int32]
        lib.cg_ref_name.restype = C.c_char_p
        lib.cg_ref_length.argtypes = [C.c_void_p, C.c_int32]
        lib.cg_ref_length.restype = C.c_int64
        lib.cg_set_inflate_device.argtypes = [C.c_void_p, C.c_int]
        lib.cg_get_inflate_stats.argtypes = [C.c_void_p, C.POINTER(InflateStats)]
        lib.cg_debug_ranges.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
                                        C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
        lib.cg_set_subsample.argtypes = [C.c_void_p, C.c_double, C.c_uint32]
        lib.cg_get_subsample_stats.argtypes = [C.c_void_p, C.POINTER(SubsampleStats)]
        from .read_filter import ReadStats
        lib.cg_set_read_filter.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        lib.cg_set_read_stats.argtypes = [C.c_void_p, C.c_int]
        lib.cg_get_read_stats.argtypes = [C.c_void_p, C.POINTER(ReadStats)]
        lib.cg_set_reference.argtypes = [C.c_void_p, C.c_char_p]
        lib.cg_get_reference_stats.argtypes = [C.c_void_p, C.POINTER(ReferenceStats)]
        lib.cg_reference_codes.argtypes = [C.c_char_p, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64),
                                           C.c_int]
        lib.cg_reference_codes_host.argtypes = lib.cg_reference_codes.argtypes[:-1]
        lib.cg_set_left_align.argtypes = [C.c_void_p, C.c_int]
        lib.cg_get_left_align_stats.argtypes = [C.c_void_p, C.POINTER(LeftAlignStats)]
        lib.cg_left_align_host.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32,
                                           C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int32)]
        lib.bz_inflate.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_int]
        lib.bz_inflate_host.argtypes = lib.bz_inflate.argtypes[:-1]
        lib.bz_status_text.argtypes = [C.c_int]
        lib.bz_status_text.restype = C.c_char_p
        lib.bz_last_error.restype = C.c_char_p
        _lib = lib
    return _lib


def default_threads() -> int:
    return min(16, len(os.sched_getaffinity(0)))


def status_text(status: int) -> str:
    return load_library().bz_status_text(int(status)).decode()


def inflate_blocks(blocks: bytes, block_off, out, out_off, device: Optional[int] = None) -> List[int]:
    """Inflates the whole BGZF blocks that start at ``blocks[block_off[i]]`` into ``out[out_off[i]:]`` (``out``: a writable
    uint8 numpy array, changed in place) and returns one status per block (0 = ok, else ``status_text``).  ``device`` None runs
    the decode core on the CPU (``bz_inflate_host``), an ordinal runs the kernel on that GPU (``bz_inflate``)."""
    import numpy as np
    host_lib = os.environ.get("DL4VC_BGZF_HOST_LIB")     # (a sanitizer build of the decode core: tools/asan_bgzf.sh)
    if device is None and host_lib:
        lib = C.CDLL(host_lib)
        lib.bz_inflate_host.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.bz_last_error.restype = C.c_char_p
    else:
        lib = load_library()
    boff = np.ascontiguousarray(block_off, dtype=np.uint64)
    ooff = np.ascontiguousarray(out_off, dtype=np.uint64)
    if boff.shape != ooff.shape or boff.ndim != 1:
        raise ValueError("block_off and out_off must be one-dimensional and of one length")
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable):
        raise ValueError("out must be a writable contiguous uint8 array")
    blocks = bytes(blocks)
    status = np.zeros(len(boff), np.int32)
    args = [blocks, len(blocks), boff.ctypes.data, len(boff), out.ctypes.data, out.size, ooff.ctypes.data, status.ctypes.data]
    rc = lib.bz_inflate_host(*args) if device is None else lib.bz_inflate(*args, int(device))
    if rc != 0:
        raise RuntimeError("bz_inflate: %s" % lib.bz_last_error().decode())
    return [int(v) for v in status]


def reference_codes(raw: bytes, linebases: int, linewidth: int, length: int, device: Optional[int] = None):
    """The BAM nibble codes of the ``length`` bases in ``raw`` (a FASTA contig's bytes from its first base on, line breaks
    included, ``linebases`` bases on lines of ``linewidth`` bytes) as a uint8 numpy array, and the count of bytes outside the
    alphabet (read as N).  ``device`` None runs the rule on the CPU (``cg_reference_codes_host``), an ordinal runs the kernel on
    that GPU (``cg_reference_codes``).  Raises RuntimeError when the layout does not describe the bytes."""
    import numpy as np
    lib = load_library()
    raw = bytes(raw)
    out = np.zeros(max(1, length), np.uint8)
    other = C.c_int64()
    args = [raw, len(raw), linebases, linewidth, length, out.ctypes.data, C.byref(other)]
    rc = lib.cg_reference_codes_host(*args) if device is None else lib.cg_reference_codes(*args, int(device))
    if rc != 0:
        raise RuntimeError(lib.cg_last_error().decode())
    return out[:max(0, length)], other.value


LEFT_ALIGN_INS, LEFT_ALIGN_DEL = 1, 2
LEFT_ALIGN_ELIGIBLE, LEFT_ALIGN_CLAMPED = 1, 2


def left_align_host(codes, kind: int, anchor_aligned: bool, anchor_pos: int, anchor_code: int, bases: Sequence[int], floor: int = 0):
    """The left-alignment rule of ``csrc/cand_left_align.h`` for one observation, on the CPU (``cg_left_align_host``).  ``codes``:
    the contig as a uint8 numpy array of BAM nibble codes; ``kind``: ``LEFT_ALIGN_INS`` / ``LEFT_ALIGN_DEL``; ``bases``: the
    inserted or deleted bases as codes.  Returns ``(pos, anchor_code, bases, flags)``."""
    import numpy as np
    lib = load_library()
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    b = np.ascontiguousarray(bases, dtype=np.uint8)
    out = np.zeros(len(b) + 1, np.uint8)
    pos, flags = C.c_int64(), C.c_int32()
    rc = lib.cg_left_align_host(codes.ctypes.data, len(codes), kind, int(bool(anchor_aligned)), anchor_pos, anchor_code, b.ctypes.data,
                                len(b), floor, C.byref(pos), out.ctypes.data, C.byref(flags))
    if rc != 0:
        raise RuntimeError(lib.cg_last_error().decode())
    return pos.value, int(out[0]), [int(v) for v in out[1:]], flags.value


class CandidateCounter:
    """One open BAM.  ``run(subregions)`` -> ``[(region_index, tid, pos0, ref, alt, depth, count)]`` (unordered) and stats.
    ``inflate_device="gpu"`` sends each batch's BGZF blocks to the device compressed (inflate, record walk and framing there;
    needs the ``.bai``); the stats then carry ``inflate_*`` entries as well.  ``reference="ref.fa"``: a read without an MD tag is
    walked against the FASTA's bases of its contig (whole contigs, resident on the device, 1 byte per base) instead of giving
    no alleles; reads with MD are walked by their MD as before.  The stats then carry ``reference_*`` entries.
    ``left_align=True`` (needs ``reference``): every insertion and deletion is moved to its left-most placement on the
    reference bases before it is counted (``cg_set_left_align``), so the placements of one event in a repeat give one candidate;
    the stats then carry ``left_align_*`` entries.
    ``subsample=(fraction, seed)``: reads are subsampled by name hash (``bamio.SampleRule``, ``cg_set_subsample``) where a read
    outside the subregion is dropped, on the host or in the device's frame kernel; the stats then carry ``subsample_records_seen``
    and ``subsample_records_kept``.  ``read_filter=(exclude, require, min_mapq)``: reads are dropped by flags and mapping quality
    at the same place, in front of that rule (``bamio.ReadFilter``, ``cg_set_read_filter``); ``read_stats=True`` collects the read
    census without a filter too.  With either, the stats carry the ``read_*`` entries (``read_filter.ReadStats.flat``)."""

    def __init__(self, bam_path: str, bai_path: Optional[str] = None, threads: Optional[int] = None,
                 max_len_indel_allele: int = 60, snp_min_freq: float = 0.01, indel_min_freq: float = 0.01, device: int = 0,
                 inflate_device: Optional[str] = None, reference: Optional[str] = None, subsample=None,
                 read_filter=None, read_stats: bool = False, left_align: bool = False):
        from .bamio import ReadFilter, SampleRule
        if left_align and reference is None:
            raise ValueError("left_align needs reference: left-alignment is defined by the reference bases")
        self.subsample = SampleRule.of(subsample)
        self.read_filter = ReadFilter.of(read_filter)
        self.collects = bool(read_stats) or self.read_filter is not None
        if inflate_device is not None and inflate_device not in INFLATE_DEVICES:
            raise ValueError("inflate_device must be None or one of %s" % (INFLATE_DEVICES,))
        self.lib = load_library()
        if bai_path is None and os.path.isfile(bam_path + ".bai"):
            bai_path = bam_path + ".bai"
        opt = Options(threads or default_threads(), max_len_indel_allele, snp_min_freq, indel_min_freq, device)
        h = C.c_void_p()
        rc = self.lib.cg_open(bam_path.encode(), (bai_path or "").encode(), C.byref(opt), C.byref(h))
        if rc != 0:
            raise RuntimeError("cg_open: %s" % self.lib.cg_last_error().decode())
        self.h = h
        self.inflate_device = inflate_device
        if inflate_device is not None and self.lib.cg_set_inflate_device(h, 1) != 0:
            msg = self.lib.cg_last_error().decode()
            self.close()
            raise RuntimeError("cg_set_inflate_device: %s" % msg)
        self.reference = reference
        if reference is not None and self.lib.cg_set_reference(h, os.fsencode(reference)) != 0:
            msg = self.lib.cg_last_error().decode()
            self.close()
            raise RuntimeError("cg_set_reference: %s" % msg)
        self.left_align = bool(left_align)
        if self.left_align and self.lib.cg_set_left_align(h, 1) != 0:
            msg = self.lib.cg_last_error().decode()
            self.close()
            raise RuntimeError("cg_set_left_align: %s" % msg)
        if self.subsample is not None and self.lib.cg_set_subsample(h, self.subsample.fraction, self.subsample.seed) != 0:
            msg = self.lib.cg_last_error().decode()
            self.close()
            raise RuntimeError("cg_set_subsample: %s" % msg)
        if (self.read_filter is not None and self.lib.cg_set_read_filter(h, *self.read_filter.as_tuple()) != 0) or \
                (read_stats and self.lib.cg_set_read_stats(h, 1) != 0):
            msg = self.lib.cg_last_error().decode()
            self.close()
            raise RuntimeError("cg_set_read_filter: %s" % msg)
        n = self.lib.cg_n_refs(h)
        self.references: List[str] = [self.lib.cg_ref_name(h, i).decode() for i in range(n)]
        self.lengths: List[int] = [int(self.lib.cg_ref_length(h, i)) for i in range(n)]

    def run(self, subregions: Sequence[Tuple[int, int, int]]):
        regs = (Region * max(1, len(subregions)))(*[Region(t, s, e) for t, s, e in subregions])
        out = C.POINTER(Candidate)()
        n = C.c_int64()
        st = Stats()
        rc = self.lib.cg_run(self.h, regs, len(subregions), C.byref(out), C.byref(n), C.byref(st))
        if rc != 0:
            raise RuntimeError("cg_run: %s" % self.lib.cg_last_error().decode())
        res = [(c.region, c.tid, c.pos0, c.ref.decode(), c.alt.decode(), c.depth, c.count) for c in out[:n.value]]
        stats = st.as_dict()
        if self.inflate_device is not None:
            ist = InflateStats()
            self.lib.cg_get_inflate_stats(self.h, C.byref(ist))
            stats.update((k if k == "inflate_ms" else "inflate_" + k, v) for k, v in ist.as_dict().items())
        if self.reference is not None:
            rst = ReferenceStats()
            self.lib.cg_get_reference_stats(self.h, C.byref(rst))
            stats.update(("reference_" + k, v) for k, v in rst.as_dict().items())
        if self.left_align:
            lst = LeftAlignStats()
            self.lib.cg_get_left_align_stats(self.h, C.byref(lst))
            stats.update(("left_align_" + k, v) for k, v in lst.as_dict().items())
        if self.subsample is not None:
            sst = SubsampleStats()
            self.lib.cg_get_subsample_stats(self.h, C.byref(sst))
            stats.update(subsample_records_seen=sst.records_seen, subsample_records_kept=sst.records_kept)
        if self.collects:
            from .read_filter import ReadStats
            rs = ReadStats()
            self.lib.cg_get_read_stats(self.h, C.byref(rs))
            stats.update(rs.flat())
        return res, stats

    def debug_ranges(self, tid: int, start: int, end: int):
        """``(ranges, bounds)`` of the device inflate path for one region, as BGZF virtual offsets: merged ``[begin, end)``
        pairs and the sorted walk boundaries (for tests; reads the index only)."""
        import numpy as np
        nr, nb = C.c_int64(), C.c_int64()
        if self.lib.cg_debug_ranges(self.h, tid, start, end, None, 0, C.byref(nr), None, 0, C.byref(nb)) != 0:
            raise RuntimeError("cg_debug_ranges: %s" % self.lib.cg_last_error().decode())
        ranges, bounds = np.zeros(2 * max(1, nr.value), np.uint64), np.zeros(max(1, nb.value), np.uint64)
        self.lib.cg_debug_ranges(self.h, tid, start, end, ranges.ctypes.data, nr.value, C.byref(nr), bounds.ctypes.data, nb.value,
                                 C.byref(nb))
        return [(int(ranges[2 * i]), int(ranges[2 * i + 1])) for i in range(nr.value)], [int(v) for v in bounds[:nb.value]]

    def close(self) -> None:
        if self.h:
            self.lib.cg_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
