"""The case grid of the zlib compressor (csrc/zdeflate.h), shared by tests/test_zdeflate_host.py (CPU) and
tests/test_compress_gpu.py: every length at which the code takes another path -- below, at and above the shortest and the
longest match, one byte either side of a segment boundary, several segments with a short last one -- times the contents that
matter: runs (distance 1), one repeated byte, a period of 3 (matches that overlap their own output), incompressible bytes
(segments that are stored), pileup records, and a run that straddles a segment boundary."""
import os

import numpy as np

SEGMENT = 4096                      # the grid's segment size: small, so that "three segments plus 1" stays small
_RANDOM = os.urandom(3 * 16384 + 1)


def lengths(seg):
    return [1, 2, 257, 258, 259, seg - 1, seg, seg + 1, 3 * seg + 1]


def _pileup_like(n, seed=5):
    """Bytes shaped like candidate records: rows of tokens 1..4 that repeat their neighbours, qualities, strands 1 / 2, zero rows."""
    rng = np.random.default_rng(seed)
    W, out = 201, []
    ref = rng.integers(1, 5, W, dtype=np.uint8)
    while sum(len(x) for x in out) < n:
        depth = int(rng.integers(3, 12))
        for plane in range(3):
            rows = np.zeros((16, W), np.uint8)
            for r in range(depth):
                a = int(rng.integers(0, 100))
                rows[r, a:a + 100] = ref[a:a + 100] if plane == 0 else rng.integers(15, 41, 100) if plane == 1 else 1 + r % 2
            out.append(rows.tobytes())
    return b"".join(out)[:n]


_PILEUP = _pileup_like(3 * 16384 + 1)


def pileup_like(n):
    return _PILEUP[:n]


def contents(n, seg):
    """-> [(name, bytes of length n)]"""
    cut = max(0, min(n, seg) - 100)          # a run of 5s from 100 bytes before the first boundary to 100 after it, random around it
    straddle = (_RANDOM[:cut] + b"\x05" * 200 + _RANDOM[cut:])[:n]
    return [("zeros", bytes(n)), ("one byte", b"\x07" * n), ("period 3", (b"abc" * (n // 3 + 1))[:n]), ("random", _RANDOM[:n]),
            ("pileup-like", pileup_like(n)), ("straddling run", straddle)]


def grid(seg=SEGMENT):
    """-> [(name, segment size, bytes)]: the lengths x the contents at ``seg``, plus the boundary lengths at the default segment."""
    out = [("%s x %d" % (name, n), seg, data) for n in lengths(seg) for name, data in contents(n, seg)]
    for n in (16383, 16384, 16385, 3 * 16384 + 1):
        out += [("%s x %d (segment 16384)" % (name, n), 16384, data) for name, data in contents(n, 16384)]
    return out
