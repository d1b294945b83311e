"""Site sharding across GPUs: contiguous index ranges, no collective.

Candidate sites are independent, so the record range ``[0, N)`` is cut into G contiguous slices
``[g*N//G, (g+1)*N//G)``; each rank (one process per GPU) scores its slice into a part file and the
parts are concatenated in rank order, which reproduces the single-process file byte for byte because
the reference iterates in record order (``shuffle=False``, main.py:94).
"""
from __future__ import annotations

import os
import shutil
import time
import zlib
from typing import List, Optional, Tuple

import numpy as np


def shard_range(n: int, index: int, count: int) -> Tuple[int, int]:
    if count < 1 or not (0 <= index < count):
        raise ValueError("shard %d of %d" % (index, count))
    return (index * n) // count, ((index + 1) * n) // count


def parse_shard(text: str) -> Tuple[int, int]:
    """``"i/n"`` -> (i, n); empty -> (0, 1)."""
    if not text:
        return 0, 1
    i, n = text.split("/")
    i, n = int(i), int(n)
    if n < 1 or not (0 <= i < n):
        raise ValueError("bad --shard %r" % text)
    return i, n


def part_path(path: str, index: int) -> str:
    return "%s.part%d" % (path, index)


def concat_parts(path: str, count: int, header_from: str = None, keep_parts: bool = False) -> str:
    """``path`` = header (the '#' lines of ``header_from`` if given) + part0 + part1 + ...  Parts hold records
    only.  Returns ``path``."""
    with open(path, "wb") as out:
        if header_from:
            with open(header_from, "rb") as f:
                for line in f:
                    if not line.startswith(b"#"):
                        break
                    out.write(line)
        for g in range(count):
            with open(part_path(path, g), "rb") as f:
                shutil.copyfileobj(f, out, 1 << 20)
    if not keep_parts:
        for g in range(count):
            os.remove(part_path(path, g))
    return path


# ------------------------------------------------------------------------------------------
# --test_bam on several GPUs: the record census (one flag per location: 1 = the location gives a record)
# ------------------------------------------------------------------------------------------
def plan_bam_shard(flags, held_out=None, site_limit: int = 0, shard_index: int = 0, shard_count: int = 1) -> List[Tuple[int, int, int]]:
    """The locations shard ``shard_index`` of ``shard_count`` scores, as runs ``(location_lo, location_hi, first_record)``:
    scoring ``locations[lo:hi]`` with the first record seeded as record ``first_record`` gives exactly the shard's records.

    ``flags``: the census of ALL locations.  A location's record index is the exclusive prefix sum of the flags -- the index
    the record has in the candidate file the converter would write.  Selected records are all records, or those whose
    location is ``held_out`` (one bool per location: ``--test_holdout_chromosomes``), cut to the first ``site_limit`` (> 0);
    the selection is split with ``shard_range``: the selection and the split ``inference.run_shard`` makes on a candidate file.

    A run holds no record outside the shard's.  Locations without a record ride along so that scoring checks their flag too:
    each goes with the selected record before it, or, where none is in front of it, with the one after it."""
    flags = np.asarray(flags).astype(bool)
    n = len(flags)
    if held_out is not None and len(held_out) != n:
        raise ValueError("held_out has %d entries for %d locations" % (len(held_out), n))
    rec_index = np.cumsum(flags, dtype=np.int64) - flags
    sel = np.flatnonzero(flags & np.asarray(held_out, bool)) if held_out is not None else np.flatnonzero(flags)
    if site_limit > 0:
        sel = sel[:site_limit]
    a, b = shard_range(len(sel), shard_index, shard_count)
    mine = sel[a:b]
    if len(mine) == 0:
        return []
    flagged = np.flatnonzero(flags)
    chosen = np.zeros(n, bool)
    chosen[sel] = True
    r = rec_index[mine]                                    # (flagged[r] == mine)
    nxt = np.where(r + 1 < len(flagged), flagged[np.minimum(r + 1, len(flagged) - 1)], n)
    prv = np.where(r > 0, flagged[np.maximum(r - 1, 0)], -1)
    hi = nxt                                               # the empty locations behind the record
    lo = np.where((prv >= 0) & chosen[np.maximum(prv, 0)], mine, prv + 1)   # and those in front that no selected record precedes
    cut = np.flatnonzero(hi[:-1] != lo[1:]) + 1
    starts, ends = np.concatenate(([0], cut)), np.concatenate((cut, [len(mine)]))
    return [(int(lo[i]), int(hi[j - 1]), int(r[i])) for i, j in zip(starts, ends)]


def census_path(path: str, index: int) -> str:
    """The side file of shard ``index``'s census flags, next to its part file."""
    return part_path(path, index) + ".census"


def write_census(path: str, flags) -> None:
    """One uint8 per location at ``path``, atomically: a reader sees the whole file or none of it."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(np.ascontiguousarray(flags, np.uint8).tobytes())
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def wait_census(path: str, shard_count: int, sizes, timeout_s: float = 600.0, poll_s: float = 0.05) -> np.ndarray:
    """The census of every shard (``census_path(path, g)``, ``sizes[g]`` flags each), concatenated.  Waits for files that are
    not there yet; after ``timeout_s`` seconds a missing one is a ``RuntimeError`` naming its shard."""
    deadline = time.monotonic() + timeout_s
    parts = []
    for g in range(shard_count):
        p = census_path(path, g)
        while not os.path.exists(p):
            if time.monotonic() >= deadline:
                raise RuntimeError("the record census of shard %d/%d did not arrive within %g s (%s is missing): that shard "
                                   "failed or has not started" % (g, shard_count, timeout_s, p))
            time.sleep(poll_s)
        a = np.fromfile(p, np.uint8)
        if len(a) != sizes[g]:
            raise RuntimeError("the record census of shard %d/%d holds %d flags for %d locations (%s)" % (g, shard_count, len(a), sizes[g], p))
        parts.append(a)
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def remove_census(path: str, shard_count: int) -> None:
    for g in range(shard_count):
        try:
            os.remove(census_path(path, g))
        except OSError:
            pass


# ------------------------------------------------------------------------------------------
# data-parallel replicas: a cheap proof that every rank holds the same parameters
# ------------------------------------------------------------------------------------------
PER_REPLICA_SUFFIXES = ("running_mean", "running_var", "num_batches_tracked")


def replica_checksum(state) -> np.ndarray:
    """Three numbers that are equal on two ranks exactly when their trained parameters are bit-identical (up to a CRC
    collision): CRC-32 of every parameter's bytes chained in key order, split into two 16-bit halves (so that a float64
    all-reduce carries them exactly), and the tensor count.  BatchNorm running statistics are per replica by design
    (nn.DataParallel keeps replica 0's; main.py:117) and do not take part."""
    crc, n = 0, 0
    for key in sorted(state):
        if key.rsplit(".", 1)[-1] in PER_REPLICA_SUFFIXES:
            continue
        crc = zlib.crc32(np.ascontiguousarray(state[key]).tobytes(), crc)
        n += 1
    return np.array([crc >> 16, crc & 0xFFFF, n], np.float64)


def check_replicas_agree(state, all_reduce_max, what: str = "evaluation") -> None:
    """Raises when any rank's parameters differ from another's.  ``all_reduce_max(vec)`` -> element-wise maximum over ranks of a
    float64 vector.  The sharded evaluation scores each rank's share with that rank's parameters: identical by construction
    (every rank applies the same averaged gradient), and this is the check that the construction held -- a rank that
    diverged (a skipped step, a non-deterministic reduction) would otherwise score with other weights without any error."""
    mine = replica_checksum(state)
    both = np.asarray(all_reduce_max(np.concatenate([mine, -mine])), np.float64)
    hi, lo = both[:3], -both[3:]
    if not np.array_equal(hi, lo):
        raise RuntimeError("%s: the ranks hold different parameters (checksum range %s .. %s, this rank %s); the data-parallel "
                           "replicas have diverged" % (what, lo.astype(np.int64).tolist(), hi.astype(np.int64).tolist(),
                                                        mine.astype(np.int64).tolist()))
