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
SYMBOLS = ("cg_open", "cg_run", "cg_last_error", "cg_close", "cg_n_refs", "cg_ref_name", "cg_ref_length")


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
        _lib = lib
    return _lib


def default_threads() -> int:
    return min(16, len(os.sched_getaffinity(0)))


class CandidateCounter:
    """One open BAM.  ``run(subregions)`` -> ``[(region_index, tid, pos0, ref, alt, depth, count)]`` (unordered) and stats."""

    def __init__(self, bam_path: str, bai_path: Optional[str] = None, threads: Optional[int] = None,
                 max_len_indel_allele: int = 60, snp_min_freq: float = 0.01, indel_min_freq: float = 0.01, device: int = 0):
        self.lib = load_library()
        if bai_path is None and os.path.isfile(bam_path + ".bai"):
            bai_path = bam_path + ".bai"
        opt = Options(threads or default_threads(), max_len_indel_allele, snp_min_freq, indel_min_freq, device)
        h = C.c_void_p()
        rc = self.lib.cg_open(bam_path.encode(), (bai_path or "").encode(), C.byref(opt), C.byref(h))
        if rc != 0:
            raise RuntimeError("cg_open: %s" % self.lib.cg_last_error().decode())
        self.h = h
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
        return res, st.as_dict()

    def close(self) -> None:
        if self.h:
            self.lib.cg_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
