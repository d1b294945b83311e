"""The command-line face of the read filter by flags and mapping quality (``bamio.ReadFilter``) and of the read census:
``--min-mapq Q --exclude-flags F --require-flags F --read-stats`` on every tool that reads a BAM (the masks decimal or ``0x...``
as for ``samtools view -F / -f``), the refusals they share, the ctypes mirror of ``dl4vc_read_stats`` and the lines they print.
"""
from __future__ import annotations

import argparse
import ctypes as C
from typing import Dict, Optional, Tuple

from .bamio import ReadFilter

FLAG_NAMES = ("PAIRED", "PROPER_PAIR", "UNMAP", "MUNMAP", "REVERSE", "MREVERSE", "READ1", "READ2", "SECONDARY", "QCFAIL", "DUP",
              "SUPPLEMENTARY", "0x1000", "0x2000", "0x4000", "0x8000")
TOTALS = ("seen", "dropped_flags", "dropped_mapq", "kept")


class ReadStats(C.Structure):
    """``dl4vc_read_stats`` (include/dl4vc_loader.h): the read census of the last call of a ``cg_`` / ``pg_`` / ``pe_`` handle."""
    _fields_ = [("mapq_hist", C.c_uint64 * 256), ("flag_bits", C.c_uint64 * 16)] + [(n, C.c_uint64) for n in TOTALS]

    def flat(self) -> Dict[str, int]:
        """Numeric entries that add up over calls and processes: ``read_seen`` ..., and the bins that are not zero as
        ``read_mapq_<Q>`` / ``read_flag_<bit>``."""
        out = {"read_" + n: int(getattr(self, n)) for n in TOTALS}
        out.update(("read_mapq_%d" % q, int(v)) for q, v in enumerate(self.mapq_hist) if v)
        out.update(("read_flag_%d" % k, int(v)) for k, v in enumerate(self.flag_bits) if v)
        return out


def census_of(flat: Dict[str, int]) -> dict:
    """``{"mapq_hist": [256], "flag_bits": [16], "seen": ..}`` from the ``read_*`` entries of a stats dict."""
    out = {n: int(flat.get("read_" + n, 0)) for n in TOTALS}
    out["mapq_hist"] = [int(flat.get("read_mapq_%d" % q, 0)) for q in range(256)]
    out["flag_bits"] = [int(flat.get("read_flag_%d" % k, 0)) for k in range(16)]
    return out


def _mask(text: str) -> int:
    try:
        return int(text, 0)
    except ValueError:
        raise argparse.ArgumentTypeError("%r is not a number (decimal or 0x...)" % (text,))


def add_flags(p: argparse.ArgumentParser) -> None:
    p.add_argument("--min-mapq", dest="min_mapq", type=int, default=None, metavar="Q",
                   help="Drop the reads of the BAM whose mapping quality is below Q in [0, 255] (samtools view -q), where a read "
                   "outside the region is dropped: every stage given the same filter sees the same reads")
    p.add_argument("--exclude-flags", dest="exclude_flags", type=_mask, default=None, metavar="F",
                   help="Drop the reads with any of these flag bits set (samtools view -F; decimal or 0x...), e.g. 0x704, the mask "
                   "the pileup encoders drop anyway")
    p.add_argument("--require-flags", dest="require_flags", type=_mask, default=None, metavar="F",
                   help="Drop the reads that lack any of these flag bits (samtools view -f; decimal or 0x...)")
    p.add_argument("--read-stats", dest="read_stats", action="store_true",
                   help="Print the read census of the run: totals, the flag bits by name, the MAPQ histogram's bins that are not zero "
                   "(counted in front of the filter, once per region a read belongs to); with or without a filter")


def given(args) -> bool:
    return any(getattr(args, n, None) is not None for n in ("min_mapq", "exclude_flags", "require_flags")) or \
        bool(getattr(args, "read_stats", False))


def check(args, fail, reads_bam: bool = True, what: str = "a BAM") -> Optional[Tuple[int, int, int]]:
    """``(exclude, require, min_mapq)`` of the parsed flags, or None without a filter; every refusal goes to ``fail(reason)``
    (which does not return), before any device work."""
    q, ex, rq = (getattr(args, n, None) for n in ("min_mapq", "exclude_flags", "require_flags"))
    if not given(args):
        return None
    if not reads_bam:
        fail("--min-mapq / --exclude-flags / --require-flags / --read-stats act on the reads of %s, and this run reads none" % what)
    if q is not None and not (0 <= q <= 255):
        fail("--min-mapq %d: a mapping quality lies in [0, 255]" % q)
    for name, v in (("--exclude-flags", ex), ("--require-flags", rq)):
        if v is not None and not (0 <= v <= 0xffff):
            fail("%s %d: the flags of a read are 16 bits, the mask must lie in [0, 0xFFFF]" % (name, v))
    if (ex or 0) & (rq or 0):
        fail("--exclude-flags 0x%x and --require-flags 0x%x share the bits 0x%x: no read could pass" % (ex, rq, ex & rq))
    f = ReadFilter(ex or 0, rq or 0, q or 0)
    return f.as_tuple() if f.on else None


def parse(p: argparse.ArgumentParser, args, reads_bam: bool = True, what: str = "a BAM") -> Optional[Tuple[int, int, int]]:
    """``check`` with ``p.error`` as the refusal."""
    return check(args, p.error, reads_bam, what)


def cli_flags(read_filter, read_stats: bool = False) -> list:
    """The flags that hand the filter on to a child process."""
    f = ReadFilter.of(read_filter)
    ex, rq, q = f.as_tuple() if f is not None else (0, 0, 0)
    return (["--exclude-flags", "0x%x" % ex] if ex else []) + (["--require-flags", "0x%x" % rq] if rq else []) + \
           (["--min-mapq", str(q)] if q else []) + (["--read-stats"] if read_stats else [])


def report_line(stats: Dict[str, int], read_filter) -> str:
    """The one line a tool prints when a filter is on."""
    f = ReadFilter.of(read_filter)
    c = census_of(stats)
    return "read filter: %d records seen, %d dropped by flags, %d dropped by MAPQ, %d kept; %s" % (
        c["seen"], c["dropped_flags"], c["dropped_mapq"], c["kept"],
        "exclude 0x%x, require 0x%x, min MAPQ %d" % f.as_tuple() if f is not None else "no filter")


def census_text(stats: Dict[str, int]) -> str:
    """What ``--read-stats`` prints."""
    c = census_of(stats)
    lines = ["read census: %d records seen, %d dropped by flags, %d dropped by MAPQ, %d kept" % tuple(c[n] for n in TOTALS)]
    lines += ["  flag 0x%-4x %-13s %d" % (1 << k, FLAG_NAMES[k], v) for k, v in enumerate(c["flag_bits"]) if v]
    lines += ["  MAPQ %-3d %d" % (q, v) for q, v in enumerate(c["mapq_hist"]) if v]
    return "\n".join(lines)
