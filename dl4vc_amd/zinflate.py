"""ctypes binding of the zlib stream inflate of libdl4vc_pileup.so (``include/dl4vc_chunks.h``): whole zlib streams of any
length -- the deflated chunks of a candidate HDF5 -- inflated by ``zi_inflate_kernel`` on the GPU (``device`` = its index) or by
the same text on the CPU (``device=None``)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import pileup_gpu

ZI_SYMBOLS = ("zi_inflate", "zi_inflate_host", "zi_status_text", "zi_last_error")
# per-stream status (the ZI_* of the header; 0..12 are the BZ_* numbers)
STATUS = {"ZI_OK": 0, "ZI_BAD_BLOCK_TYPE": 1, "ZI_BAD_STORED_LEN": 2, "ZI_BAD_CODE_LENGTHS": 3, "ZI_BAD_SYMBOL": 4,
          "ZI_DISTANCE_BEFORE_START": 5, "ZI_OUTPUT_EXCEEDS_LENGTH": 6, "ZI_OUTPUT_SHORT_OF_LENGTH": 7, "ZI_INPUT_EXHAUSTED": 8,
          "ZI_TRAILING_INPUT": 9, "ZI_BAD_SLOT": 12, "ZI_BAD_ZLIB_HEADER": 13, "ZI_ADLER_MISMATCH": 14, "ZI_RAW_SIZE_MISMATCH": 15,
          "ZI_BAD_RANGE": 16}
globals().update(STATUS)
ZI_MAX_OUTPUT = 1 << 30
_bound = None


def load_library() -> C.CDLL:
    global _bound
    if _bound is None:
        lib = pileup_gpu.load_library()
        vp = C.c_void_p
        lib.zi_inflate_host.argtypes = [vp, C.c_uint64, vp, vp, C.c_int64, vp, C.c_uint64, vp, vp, vp, vp]
        lib.zi_inflate.argtypes = lib.zi_inflate_host.argtypes + [C.c_int]
        lib.zi_status_text.argtypes = [C.c_int]
        lib.zi_status_text.restype = C.c_char_p
        lib.zi_last_error.argtypes = []
        lib.zi_last_error.restype = C.c_char_p
        _bound = lib
    return _bound


def status_text(status: int) -> str:
    return load_library().zi_status_text(int(status)).decode()


def inflate_streams(streams, off: Sequence[int], length: Sequence[int], out: np.ndarray, out_off: Sequence[int], out_len: Sequence[int],
                    raw: Optional[Sequence[int]] = None, device: Optional[int] = None) -> np.ndarray:
    """``zi_inflate`` (``device`` = a GPU's index) or ``zi_inflate_host`` (``device=None``): stream ``i`` is
    ``streams[off[i]:off[i] + length[i]]`` and goes to ``out[out_off[i]:out_off[i] + out_len[i]]`` (``out``: a writable
    contiguous uint8 array, changed in place); ``raw[i]`` non-zero: the bytes are the chunk itself.  -> status, int32 per stream."""
    lib = load_library()
    src = np.frombuffer(streams, np.uint8) if not isinstance(streams, np.ndarray) else streams
    if src.dtype != np.uint8 or not src.flags.c_contiguous or out.dtype != np.uint8 or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError("streams and out: contiguous uint8 arrays, out writable")
    n = len(off)
    a64 = lambda x: np.ascontiguousarray(x, np.uint64)   # noqa: E731
    off, length, out_off, out_len = a64(off), a64(length), a64(out_off), a64(out_len)
    if not (len(length) == len(out_off) == len(out_len) == n) or (raw is not None and len(raw) != n):
        raise ValueError("off, length, out_off, out_len and raw: one entry per stream")
    rawa = np.ascontiguousarray(raw, np.uint8) if raw is not None else None
    status = np.full(n, -1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None   # noqa: E731
    args = [p(src), src.size, p(off), p(length), n, p(out), out.size, p(out_off), p(out_len), p(rawa), p(status)]
    rc = lib.zi_inflate_host(*args) if device is None else lib.zi_inflate(*args, int(device))
    if rc != 0:
        raise RuntimeError("%s failed: %s" % ("zi_inflate_host" if device is None else "zi_inflate", lib.zi_last_error().decode()))
    return status
