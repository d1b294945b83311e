"""The command-line face of read subsampling by name hash (``bamio.SampleRule``; the flags are named as samtools names them):
``--subsample F [--subsample-seed S]`` on every tool that reads a BAM, the refusals they share and the one line they print.
"""
from __future__ import annotations

import argparse
from typing import Optional, Tuple

from .bamio import SampleRule


def add_flags(p: argparse.ArgumentParser) -> None:
    p.add_argument("--subsample", type=float, default=None, metavar="F",
                   help="Keep the fraction F in (0, 1] of the BAM's reads, chosen by a hash of the read name as `samtools view "
                   "--subsample F` chooses them: mates stay together, and every stage given the same F and seed sees the same reads")
    p.add_argument("--subsample-seed", dest="subsample_seed", type=int, default=None, metavar="S",
                   help="Seed of --subsample in [0, 2^32) (default 0): another seed keeps another subset")


def parse(p: argparse.ArgumentParser, args, reads_bam: bool = True, what: str = "a BAM") -> Optional[Tuple[float, int]]:
    """``(fraction, seed)`` of the parsed flags, or None without them; every refusal ends in ``p.error`` with its reason."""
    f, s = args.subsample, args.subsample_seed
    if f is None:
        if s is not None:
            p.error("--subsample-seed %d without --subsample: the seed chooses among subsets of a fraction" % s)
        return None
    if not reads_bam:
        p.error("--subsample thins the reads of %s, and this run reads none" % what)
    if not (0.0 < f <= 1.0):
        p.error("--subsample %r: the fraction must lie in (0, 1]" % (f,))
    s = 0 if s is None else s
    if not (0 <= s < 1 << 32):
        p.error("--subsample-seed %d: the seed must lie in [0, 2^32)" % s)
    return (f, s)


def report_line(seen: int, kept: int, subsample) -> str:
    """The one line a tool prints when the flag is given."""
    rule = SampleRule.of(subsample)
    return "subsample: %d records seen, %d kept (%.4f); asked %g, seed %d" % (seen, kept, kept / seen if seen else 0.0, rule.fraction,
                                                                             rule.seed)
