"""Site assembly without candidates.hdf: encoder planes of a list of locations -> the six planes of the forward.

What ``dataset.assemble_batch`` / the native loader do to the records of a candidate file, restated for planes that never
became records: locations without a record (status 0) leave no hole, site i takes R of the S stored rows -- the first R, or
the seeded sorted subset of a pileup deeper than R, drawn by ``dl_select_rows`` with ``seed + (absolute record index)`` --
and gets its allele masks from ``dl_allele_masks`` (both are the native loader's own functions, libdl4vc_loader.so).

``plan_sites`` is the host part (rows, masks, record text); ``assemble_host`` is the numpy statement of the copy that
``pg_assemble_device`` (csrc/assemble_kernels.hip) does on the device, and the definition that kernel is tested against."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

from .hdf5_schema import VCFREC_BYTES


@dataclass
class SitePlan:
    slots: np.ndarray        # (m,) i32   location slot of each output site
    rows: np.ndarray         # (m,R) i16  stored rows of each output site; ``| ZERO_READS``: that row's quality and strand under an
                             #            all-zero reads plane (csrc/plan_entry.h: dynamic read down-sampling's fill rows)
    first_rows: np.ndarray   # (m,) u8    1: rows 0..R-1
    ref: np.ndarray          # (m,L) u8
    ref_mask: np.ndarray     # (m,L) u8
    var_mask: np.ndarray     # (m,L) u8
    vcfrec: List[str]        # record text as the candidate file would hold it (truncated to S128)
    num_reads: np.ndarray    # (m,) i32
    blacklist: np.ndarray = None   # (m,) bool  the allele masks are the blacklist fallback (``NativeLoader``'s ``blacklist``)
    sampled: np.ndarray = None     # (m,) i32   reads dynamic down-sampling kept (``num_reads`` where it did not act)

    def __len__(self):
        return len(self.slots)

    def slice(self, lo: int, hi: int) -> "SitePlan":
        return SitePlan(self.slots[lo:hi], self.rows[lo:hi], self.first_rows[lo:hi], self.ref[lo:hi], self.ref_mask[lo:hi],
                        self.var_mask[lo:hi], self.vcfrec[lo:hi], self.num_reads[lo:hi],
                        None if self.blacklist is None else self.blacklist[lo:hi],
                        None if self.sampled is None else self.sampled[lo:hi])


ZERO_READS = 0x4000          # csrc/plan_entry.h: bit 14 of a plan entry


def plane_set(torch, dev, B, R, L):
    """The six planes of a forward batch of B sites in device memory: reads, qual, strand ``[B][R][L]``, ref, ref_mask, var_mask
    ``[B][L]``."""
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)   # noqa: E731
    return [u8(B, R, L) for _ in range(3)] + [u8(B, L) for _ in range(3)]


def stored_vcfrec(vcf_string: str) -> str:
    """The text ``record_dtype``'s ``vcfrec`` field keeps of a location's record: 128 bytes, read back up to the first NUL."""
    return vcf_string.encode()[:VCFREC_BYTES].split(b"\x00", 1)[0].decode()


def plan_sites(status, num_reads, ref, vcf_strings: Sequence[str], reads: int, stored_rows: int, seed: int,
               first_record: int = 0) -> SitePlan:
    """Rows and masks of the locations with ``status == 1``, in order.  Site i (counting records only) draws with
    ``seed + first_record + i``, as ``score_records`` / ``NativeLoader`` seed record ``first_record + i`` of a file."""
    slots = np.flatnonzero(np.asarray(status) == 1).astype(np.int32)
    return plan_records(slots, first_record + np.arange(len(slots), dtype=np.int64), num_reads, ref, vcf_strings, reads, stored_rows,
                        seed)


def plan_records(slots, record_index, num_reads, ref, vcf_strings: Sequence[str], reads: int, stored_rows: int, seed: int,
                 downsample_rate: float = 0.0, downsample_prob: float = 0.0) -> SitePlan:
    """``plan_sites`` with the sites named one by one: site i is slot ``slots[i]`` (any order, a slot may repeat) and draws the
    subset of a deep pileup with ``seed + record_index[i]`` -- the rule of ``train_data.assemble_training_batch``
    (``RandomState(seed + idx)``) for the shuffled records of a training batch.  ``num_reads``, ``ref`` and ``vcf_strings`` are
    indexed by slot.

    ``downsample_rate`` / ``downsample_prob`` (training only): every site draws dynamic read down-sampling with its seed
    (``dl_select_rows_downsample`` = ``dataset.plan_rows``); a fill row's entry carries ``ZERO_READS``.  A site deeper than the
    stored rows takes its rows from the middle window of ``dataset.assemble_site`` (dataset.py:517-521)."""
    from . import loader
    lib = loader.load_library()
    slots = np.ascontiguousarray(slots, np.int32)
    record_index = np.asarray(record_index, np.int64)
    if record_index.shape != slots.shape:
        raise ValueError("%d record indices for %d slots" % (len(record_index), len(slots)))
    m, R, S = len(slots), int(reads), int(stored_rows)
    L = ref.shape[1] if ref.ndim == 2 else 0
    if R > S:
        raise ValueError("the model reads %d rows per site but the encoder stores only %d" % (R, S))
    if m and L != 201:
        raise ValueError("allele masks are defined on the 201-column window (window size 100), not %d columns" % L)
    rows = np.empty((m, R), np.int16)
    rows[:] = np.arange(R, dtype=np.int16)
    first = np.ones(m, np.uint8)
    out_ref = np.ascontiguousarray(ref[slots], np.uint8)
    rmask, vmask = np.zeros((m, L), np.uint8), np.zeros((m, L), np.uint8)
    nr = np.ascontiguousarray(np.asarray(num_reads)[slots], np.int32)
    recs = []
    black = np.zeros(m, bool)
    draw, zero, kept = np.empty(max(R, S), np.int32), np.zeros(max(R, S), np.uint8), C.c_int32()
    down = downsample_rate > 0 or downsample_prob > 0
    sampled = nr.copy()
    i32, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    base = int(seed) & 0xFFFFFFFF
    for i in range(m):
        n = int(nr[i])
        if n > R or down:
            start = max(0, int(int(max(n, S) / 2) - S / 2))       # the middle window of a site deeper than S (dataset.py:517-518)
            avail = S - start
            site_seed = (base + int(record_index[i])) & 0xFFFFFFFF
            if avail < 1:
                k = 0
            elif down:
                k = lib.dl_select_rows_downsample(site_seed, n, avail, R, float(downsample_rate), float(downsample_prob),
                                                  draw.ctypes.data_as(i32), zero.ctypes.data_as(u8), C.byref(kept))
                sampled[i] = kept.value
            else:
                k = lib.dl_select_rows(site_seed, n, avail, R, draw.ctypes.data_as(i32))
            if k != R:
                raise ValueError("record %d: num_reads %d leaves %d stored rows in the sampling window (< %d reads): the reference "
                                 "cannot batch this site either" % (int(record_index[i]), n, max(k, 0), R))
            rows[i] = start + draw[:R]
            if down:
                rows[i] |= zero[:R].astype(np.int16) * ZERO_READS
            first[i] = int(start == 0 and n <= R and not zero[:R].any()) if down else 0
        text = stored_vcfrec(vcf_strings[int(slots[i])])
        recs.append(text)
        st = lib.dl_allele_masks(text.encode(), p(out_ref[i:i + 1]), p(rmask[i:i + 1]), p(vmask[i:i + 1]))
        if st not in (0, 1):
            raise ValueError("record %d (%s): the allele masks cannot be built" % (int(record_index[i]), text.split("\t", 2)[:2]))
        black[i] = st == 1
    return SitePlan(slots, rows, first, out_ref, rmask, vmask, recs, nr, black, sampled)


def assemble_host(reads, qual, strand, plan: SitePlan, use_q: bool = True, use_strand: bool = True):
    """numpy statement of ``pg_assemble_device``: stored planes ``[n][S][L]`` -> ``(reads, qual, strand [m][R][L], ref, ref_mask,
    var_mask [m][L])``; row gather, compaction over the sites of ``plan``, zero-fill of an unused plane."""
    m, R = plan.rows.shape
    L = reads.shape[2]
    rows = np.where(plan.first_rows[:, None] != 0, np.arange(R)[None, :], plan.rows).astype(np.int64)
    zero = (rows & ZERO_READS) != 0                       # fill rows of dynamic down-sampling: reads plane zero
    rows &= ZERO_READS - 1
    site = plan.slots.astype(np.int64)[:, None]
    rd = np.ascontiguousarray(reads[site, rows]) if m else np.zeros((0, R, L), np.uint8)
    rd[zero] = 0
    ql = np.ascontiguousarray(qual[site, rows]) if (m and use_q) else np.zeros((m, R, L), np.uint8)
    st = np.ascontiguousarray(strand[site, rows]) if (m and use_strand) else np.zeros((m, R, L), np.uint8)
    return rd, ql, st, plan.ref.copy(), plan.ref_mask.copy(), plan.var_mask.copy()
