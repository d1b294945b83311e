"""Hand-built pileup cases for the three pileup encoders (the Python builder, ``pe_encode``, the GPU encoder): named lists of
``BamRecord``s + reference strings + locations + options, each location carrying the status ``pe_encode`` must give it and
what the GPU encoder may do with it.  Plain module (no fixtures; nothing random except the reference letters, which come from
a seeded generator); used by tests/test_pileup_edges.py (CPU), tests/test_pileup_gpu_edges.py and tests/test_pileup_gpu.py.

``expected_decline`` is the list of decline reasons of DESIGN section 9 / include/dl4vc_pileup_gpu.h restated over the
records of a case: the GPU encoder may answer 2 only where it names a reason."""
import os
import re
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from dl4vc_amd import bamio
from dl4vc_amd.bamio import BamRecord, BamWriter, build_bai

FLAG_MASK = 0x704                                   # unmapped, secondary, QC fail, duplicate
MAX_TRACKS, MAX_WINDOW = 1024, 100                   # PG_MAX_TRACKS, PG_MAX_WINDOW
KNOWN = set("AaTtUuGgCc-*NnXx.,e?MmKkRrYySsWwBbVvHhDd")   # the converter's token table
_OPS = {c: i for i, c in enumerate(bamio.CIGAR_OPS)}
_REF_OPS = (0, 2, 3, 7, 8)
_QUERY_OPS = (0, 1, 4, 7, 8)


@dataclass
class Loc:
    contig: str
    pos: int                         # VCF POS (1-based)
    cpu: int                         # the status pe_encode must give
    py: Optional[str] = None         # name of the exception the Python path raises here (None: it returns)
    gpu_encodes: Optional[bool] = None   # None: required exactly where cpu == 1 and gpu_declines is False
    gpu_declines: bool = False       # the GPU must answer 2 (and expected_decline must say why)
    note: str = ""

    def must_encode(self):
        return (self.cpu == 1 and not self.gpu_declines) if self.gpu_encodes is None else self.gpu_encodes


@dataclass
class Case:
    name: str
    refs: List[Tuple[str, str]]                      # BAM contigs (name, sequence)
    reads: List[BamRecord]
    locs: List[Loc]
    w: int = 16
    max_reads: int = 50
    mil: int = 10
    milv: int = 50
    mbq: int = 0
    index: bool = True
    sort: bool = True                                # False: records written in the order given
    fasta: Optional[List[str]] = None                # contig names the FASTA holds (None: all)
    contract_only: bool = False                      # unsorted input: only "no error, status = pe_encode's or 2"

    def options(self):
        return self.w, self.max_reads, self.mil, self.milv, self.mbq


def make_ref(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), n))


def parse_cigar(text):
    return tuple((_OPS[op], int(l)) for l, op in re.findall(r"(\d+)([MIDNSHP=X])", text))


def read(ref, pos, cigar, name, flag=0, qual=30, seq=None, tid=0):
    """One record at 0-based ``pos``; SEQ follows the reference (X: another base; I / S: fixed letters) unless given."""
    ops = parse_cigar(cigar) if isinstance(cigar, str) else tuple(cigar)
    if seq is None:
        out, p, k = [], pos, 0
        for op, l in ops:
            if op in (0, 7, 8):
                assert len(ref[p:p + l]) == l, "read %s runs past the contig" % name
                for c in ref[p:p + l].upper():
                    c = c if c in "ACGT" else "A"
                    out.append({"A": "C", "C": "G", "G": "T", "T": "A"}[c] if op == 8 else c)
            elif op in (1, 4):
                out += ["GATTACAC"[(k + j) % 8] for j in range(l)]
                k += l
            if op in _REF_OPS:
                p += l
        seq = "".join(out)
    q = np.full(len(seq), qual, np.uint8) if np.isscalar(qual) else np.asarray(qual, np.uint8)
    assert len(q) == len(seq)
    return BamRecord(tid, pos, 40, flag, name, ops, seq, q)


def file_order(case: Case):
    return sorted(case.reads, key=lambda r: (r.tid, r.pos)) if case.sort else list(case.reads)


def write_case(tmp, case: Case):
    """-> (bam path, fasta path); FASTA lines of 70, BAI unless ``case.index`` is False."""
    d = os.path.join(str(tmp), case.name)
    os.makedirs(d, exist_ok=True)
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "reads.bam")
    with open(fa, "w") as f:
        for name, seq in case.refs:
            if case.fasta is None or name in case.fasta:
                f.write(">%s\n" % name + "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + "\n")
    with BamWriter(bam, [(n, len(s)) for n, s in case.refs]) as w:
        for r in file_order(case):
            w.write(r.tid, r.pos, r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist())
    if case.index:
        build_bai(bam, bam + ".bai")
    return bam, fa


# ---- why the GPU encoder may decline ------------------------------------------------------------------------------------------
def _spellings(name):
    return (name, name[3:] if name.startswith("chr") else "chr" + name)


class Pileup:
    """The records of a BAM (``BamRecord``s in file order) and the FASTA's sequences, indexed for ``expected_decline``."""

    def __init__(self, contigs: Sequence[str], reads: Sequence[BamRecord], refs: Dict[str, str]):
        self.contigs, self.refs = list(contigs), dict(refs)
        self.by_tid = {}
        for tid in range(len(self.contigs)):
            rs = [r for r in reads if r.tid == tid]
            nref = np.array([sum(l for op, l in r.cigar if op in _REF_OPS) for r in rs], np.int64)
            start = np.array([r.pos for r in rs], np.int64)
            self.by_tid[tid] = dict(
                reads=rs, start=start, end=start + nref,
                ok=np.array([not (r.flag & FLAG_MASK) for r in rs], bool),
                has_ref=np.array([any(op in _REF_OPS for op, _ in r.cigar) for r in rs], bool),
                skip=np.array([any(op == 3 for op, _ in r.cigar) for r in rs], bool),
                eq=np.array(["=" in r.seq for r in rs], bool),
                short=np.array([sum(l for op, l in r.cigar if op in _QUERY_OPS) > len(r.seq) for r in rs], bool),
                unsorted=bool((np.diff(start) < 0).any()))

    @classmethod
    def of_case(cls, case: Case):
        fasta = {n: s for n, s in case.refs if case.fasta is None or n in case.fasta}
        return cls([n for n, _ in case.refs], file_order(case), fasta)

    @classmethod
    def of_files(cls, bam_path, fasta_path):
        with bamio.BamFile(bam_path) as b:
            names, reads = list(b.references), list(b)
        fa = bamio.FastaFile(fasta_path)
        refs = {n: fa.fetch(n, 0, fa.get_reference_length(n)) for n in fa.references}
        fa.close()
        return cls(names, reads, refs)

    def tid(self, contig):
        for name in _spellings(contig):
            if name in self.contigs:
                return self.contigs.index(name)
        return -1

    def ref(self, contig):
        for name in _spellings(contig):
            if name in self.refs:
                return self.refs[name]
        return None


def expected_decline(pile: Pileup, contig: str, pos: int, w: int, mbq: int = 0) -> set:
    """Names of the decline reasons that hold for one location; empty: the GPU encoder must not answer 2."""
    why = set()
    tid = pile.tid(contig)
    if tid < 0:
        return why                                   # no such contig in the BAM: status 0, not a decline
    if w > MAX_WINDOW:
        why.add("window")
    if mbq > 0:
        why.add("min_base_quality")
    ref = pile.ref(contig)
    if ref is None:
        why.add("contig_not_in_fasta")
        return why
    if pos < 1:
        why.add("position")
        return why
    s0, stop = max(pos - (w + 2), 0), pos + w + 3
    t = pile.by_tid[tid]
    if t["unsorted"]:
        why.add("unsorted")
    live = t["ok"] & t["has_ref"]
    if (live & (t["end"] == t["start"]) & (t["start"] >= s0) & (t["start"] < stop)).any():
        why.add("zero_length_alignment")
    sel = live & (t["end"] > t["start"]) & (t["end"] > s0) & (t["start"] < stop)
    idx = np.flatnonzero(sel)
    if len(idx) > MAX_TRACKS:
        why.add("too_many_tracks")
    if t["skip"][idx].any():
        why.add("reference_skip")
    if t["eq"][idx].any():
        why.add("eq_base")
    if t["short"][idx].any():
        why.add("short_seq")
    keys = ["%s:%s" % (t["reads"][i].name, t["reads"][i].seq) for i in idx]
    if len(set(keys)) != len(keys):
        why.add("duplicate_key")
    covered = np.zeros(stop - s0, bool)
    for i in idx:
        covered[max(t["start"][i], s0) - s0:min(t["end"][i], stop) - s0] = True
    if any(s0 + int(p) < len(ref) and ref[s0 + int(p)] not in KNOWN for p in np.flatnonzero(covered)):
        why.add("unknown_reference_base")
    return why


# ---- the grid -----------------------------------------------------------------------------------------------------------------
FREV, FDUP, FSEC = bamio.FREVERSE, bamio.FDUP, bamio.FSECONDARY


def _contig_edges(w):
    n = 3 * w + 60
    ref = make_ref(n, 11 + w)
    reads, p, i = [], 0, 0
    while p + 24 <= n:                               # reads of 24 every 7 bases from position 0 ...
        cigar = ["24M", "10M2I12M", "8M3D13M", "24M"][i % 4]
        reads.append(read(ref, p, cigar, "e%d" % i, FREV if i % 3 == 0 else 0, 20 + i % 17))
        p, i = p + 7, i + 1
    reads.append(read(ref, n - 24, "24M", "last", 0, 33))           # ... and two ending on the contig's last base
    reads.append(read(ref, n - 10, "2S10M", "last_clip", FREV, 12))
    pos = [1, 2, w + 2, w + 3, w + 4, n, n - 1, n - (w + 1), n - (w + 2), n - (w + 3)]
    locs = [Loc("ref", p, 1) for p in pos] + [Loc("ref", n + 1, 0, note="one past the contig: no column at the candidate")]
    return Case("contig_edges_w%d" % w, [("ref", ref)], reads, locs, w=w)


def _window_edges():
    ref = make_ref(1000, 21)
    w, reads = 16, []
    c = 200                                           # POS 200: s0 = 182, stop = 219
    s0, stop = c - 18, c + 19
    reads += [read(ref, s0, "30M", "at_s0"), read(ref, s0 - 1, "30M", "before_s0", FREV), read(ref, s0 + 1, "30M", "after_s0"),
              read(ref, stop - 25, "25M", "to_stop", FREV), read(ref, stop - 26, "25M", "to_stop_m1"),
              read(ref, stop - 24, "25M", "to_stop_p1"), read(ref, s0 - 19, "20M", "last_base_in", 0, 7),
              read(ref, stop - 1, "20M", "first_base_in", FREV, 9)]
    c2 = 600                                          # POS 600 (0-based 599): the crop is reference 583 .. 615
    reads += [read(ref, 570, "60M", "cover", 0, 25),
              read(ref, 584, "20M", "head_on_first_crop_col", FREV, 31), read(ref, 583, "20M", "head_outside", 0, 32),
              read(ref, 595, "20M", "tail_on_last_crop_col", 0, 33), read(ref, 596, "20M", "tail_outside", FREV, 34)]
    return Case("window_edges", [("ref", ref)], reads, [Loc("ref", c, 1), Loc("ref", c2, 1)], w=w)


SHAPES = ["6M2P3I6M", "6M2I1P2I6M", "3H12M2H", "3S2I10M", "6M2D2I6M", "6M2I2D6M", "6M2D3D6M", "1M2I11M", "11M2I1M",
          "5=1X6=", "6M0M6M", "6M2D6M"]


def _cigar_shapes():
    ref = make_ref(100 * len(SHAPES) + 1400, 31)
    reads, locs = [], []
    for i, shape in enumerate(SHAPES):
        c = 100 * i + 60                              # 0-based candidate position; the shaped reads start 5 and 3 before it
        reads += [read(ref, c - 12, "30M", "plain%d" % i, FREV if i % 2 else 0, 22),
                  read(ref, c - 5, shape, "shape%d" % i, 0 if i % 2 else FREV, 35),
                  read(ref, c - 3, shape, "shape%db" % i, FREV if i % 2 else 0, 36)]
        locs.append(Loc("ref", c + 1, 1, note=shape))
    b = 100 * len(SHAPES) + 100
    # all deletion inside the window, aligned bases outside it: the row has no strand of its own, so it comes out forward
    reads += [read(ref, b, "2M300D2M", "del_rev", FREV, 17), read(ref, b + 140, "30M", "cov_rev", FREV, 18),
              read(ref, b + 150, "30M", "cov_fwd", 0, 19)]
    locs.append(Loc("ref", b + 160, 1, note="2M300D2M on the reverse strand"))
    reads += [read(ref, b + 400, "30M40D30M", "del_fwd", 0, 27), read(ref, b + 401, "30M40D30M", "del_rev2", FREV, 28),
              read(ref, b + 440, "20M", "cov2", FREV, 29)]
    locs.append(Loc("ref", b + 451, 1, note="all deleted inside a 16-window, aligned bases outside"))
    return Case("cigar_shapes", [("ref", ref)], reads, locs, w=16)


def _insertion_caps(mil, milv, w):
    cap, cap_ci = mil, max(milv, mil)
    ref = make_ref(400 * 12 + 400, 41 + mil)
    reads, locs, k = [], [], 0

    def site(lengths, at, note):
        """One location: a plain read, and for each length a read with that insertion behind candidate + ``at``."""
        nonlocal k
        c = 400 * k + 200
        k += 1
        reads.append(read(ref, c - 20, "45M", "p%d" % k, FREV, 21))
        for j, l in enumerate(lengths):
            reads.append(read(ref, c - 10 + j, "%dM%dI20M" % (11 - j + at, l), "i%d_%d" % (k, j), FREV if j % 2 else 0, 30 + j))
        locs.append(Loc("ref", c + 1, 1, note=note))

    for l in (cap - 1, cap, cap + 1):
        if l >= 1:
            site([l], -1, "insertion of %d beside the candidate (cap %d)" % (l, cap))
    for l in (cap_ci - 1, cap_ci, cap_ci + 1):
        if l >= 1:
            site([l], 0, "insertion of %d on the candidate (cap %d)" % (l, cap_ci))
    site([2, 5], 0, "two insertion lengths at one position")
    site([1, cap_ci + 3], -1, "two insertion lengths beside the candidate")
    # many insertions left of the candidate: the crop's left edge moves right (clo > 0, off = 0)
    c = 400 * k + 200
    k += 1
    reads += [read(ref, c - 20, "45M", "many_p", 0, 21), read(ref, c - 18, "4M4I4M4I4M4I20M", "many_i", FREV, 23)]
    locs.append(Loc("ref", c + 1, 1, note="insertions left of the candidate"))
    # few columns: off > 0 on the left, the crop ends before W on the right
    c = 400 * k + 200
    k += 1
    reads += [read(ref, c - 4, "9M", "few_a", 0, 24), read(ref, c - 2, "3M1I4M", "few_b", FREV, 26)]
    locs.append(Loc("ref", c + 1, 1, note="few columns"))
    return Case("insertion_caps_%d_%d" % (mil, milv), [("ref", ref)], reads, locs, w=w, mil=mil, milv=milv)


def _qualities():
    ref = make_ref(2000, 51)
    reads, locs = [], []
    reads += [read(ref, 190, "30M", "q0_lead", 0, 0), read(ref, 192, "30M", "q_a", FREV, 30), read(ref, 194, "30M", "q_b", 0, 31)]
    locs.append(Loc("ref", 201, 0, note="leading row of quality 0: the quality plane trims one row more than the others"))
    reads += [read(ref, 590, "30M", "z_a", 0, 0), read(ref, 592, "30M", "z_b", FREV, 0), read(ref, 594, "12M3I15M", "z_c", 0, 0)]
    locs.append(Loc("ref", 601, 1, note="every quality 0: nothing is trimmed"))
    q = np.full(30, 30, np.uint8)
    q[[8, 9, 10]] = [0, 1, 255]
    reads += [read(ref, 990, "30M", "m_a", 0, 28), read(ref, 992, "30M", "m_zero", FREV, 0), read(ref, 991, "30M", "m_mix", 0, q),
              read(ref, 994, "30M", "m_b", FREV, 255)]
    locs.append(Loc("ref", 1001, 1, note="a middle row of quality 0; single bases of quality 0, 1, 255"))
    # the leading row has quality 0 only INSIDE the crop (its head column, outside, has not)
    q2 = np.zeros(40, np.uint8)
    q2[0] = 9
    reads += [read(ref, 1370, "40M", "c_lead", 0, q2), read(ref, 1390, "30M", "c_a", FREV, 30)]
    locs.append(Loc("ref", 1401, 0, note="leading row: quality 0 inside the crop only"))
    return Case("qualities", [("ref", ref)], reads, locs, w=16)


DEPTHS = [255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500]


def _depth():
    ref = make_ref(300 * len(DEPTHS) + 300, 61)
    reads, locs = [], []
    for k, n in enumerate(DEPTHS):
        c = 300 * k + 150
        for i in range(n):
            reads.append(read(ref, c - 14 + i % 5, "24M" if i % 7 else "10M1I13M", "d%d_%d" % (n, i), FREV if i % 3 == 0 else 0, 1 + i % 60))
            if n == 1024 and i % 5 == 0:             # flag-masked reads between the tracks: they do not count
                reads.append(read(ref, c - 14 + i % 5, "24M", "masked%d" % i, [FDUP, FSEC, bamio.FUNMAP, bamio.FQCFAIL][i % 4], 40))
        locs.append(Loc("ref", c + 1, 1, gpu_declines=n > MAX_TRACKS, note="%d tracks" % n))
    return Case("depth", [("ref", ref)], reads, locs, w=16, max_reads=200)


def _max_reads(mr):
    ref = make_ref(1200, 71)
    reads, locs = [], []
    for k, n in enumerate((1, 2, 6, 7, 8, 9)):
        c = 150 * k + 100
        for i in range(n):
            reads.append(read(ref, c - 12 + i, "24M" if i % 3 else "9M2I13M", "m%d_%d" % (n, i), FREV if i % 2 else 0, 10 + 3 * i))
        locs.append(Loc("ref", c + 1, 1, note="%d tracks, max_reads %d" % (n, mr)))
    return Case("max_reads_%d" % mr, [("ref", ref)], reads, locs, w=16, max_reads=mr)


def _reference_tokens():
    ref = list(make_ref(1000, 81))
    for i, ch in enumerate("NnRYMKSWBVHDryUuacgt"):
        ref[190 + i] = ch
    ref[500] = "Z"                                    # under coverage
    ref[815] = "Z"                                    # inside the window of POS 801, not covered
    ref = "".join(ref)
    reads = [read(ref, 180, "45M", "t_a", 0, 30), read(ref, 185, "20M2I20M", "t_b", FREV, 31),
             read(ref, 485, "30M", "z_a", 0, 30), read(ref, 490, "30M", "z_b", FREV, 31),
             read(ref, 785, "25M", "u_a", 0, 30), read(ref, 790, "20M", "u_b", FREV, 31)]
    locs = [Loc("ref", 201, 1, note="N, IUPAC, U and lower case in the reference"),
            Loc("ref", 501, 2, py="KeyError", gpu_declines=True, note="a character outside the table under coverage"),
            Loc("ref", 801, 1, note="the same character inside the window, outside coverage")]
    return Case("reference_tokens", [("ref", ref)], reads, locs, w=16)


def _decline_sites(name, sites, extra=False):
    """Each decline reason alone at c (two ordinary reads + the offending ones), a clean neighbour 100 bases on."""
    ref, other = make_ref(300 * len(sites) + 300, 91), make_ref(600, 92)
    reads, locs = [], []
    for k, (bad_reads, cpu, py, note, declines, encodes) in enumerate(sites):
        c = 300 * k + 150
        reads.extend([read(ref, c - 12, "30M", "c%d" % k, 0, 30), read(ref, c - 8, "30M", "r%d" % k, FREV, 31)])
        reads.extend(f(ref, c) for f in bad_reads)
        locs.append(Loc("ref", c + 1, cpu, py=py, gpu_declines=declines, gpu_encodes=encodes, note=note))
        reads.extend([read(ref, c + 90, "30M", "n%d" % k, 0, 30), read(ref, c + 94, "30M", "nr%d" % k, FREV, 31)])
        locs.append(Loc("ref", c + 101, 1, note="clean neighbour of: " + note))
    if extra:                                         # a contig the BAM has and the FASTA lacks
        reads.extend([read(other, 180, "40M", "o_a", 0, 30, tid=1), read(other, 190, "40M", "o_b", FREV, 31, tid=1)])
        locs.append(Loc("other", 201, 2, py="KeyError", gpu_declines=True, note="contig missing from the FASTA"))
        locs.append(Loc("nowhere", 201, 0, note="contig in neither file"))
    return Case(name, [("ref", ref), ("other", other)], reads, locs, w=16, fasta=["ref"])


def _declines():
    return _decline_sites("declines", [
        ([lambda ref, c: read(ref, c - 10, "8M6N8M", "skip", 0, 32)], 2, "KeyError", "N operation", True, None),
        ([lambda ref, c: read(ref, c - 10, "20M", "eq", 0, 32, seq=ref[c - 10:c] + "=" + ref[c + 1:c + 10])], 2, "KeyError",
         "= in SEQ", True, None),
        ([lambda ref, c: read(ref, c - 3, "5I", "ins_only", 0, 32)], 1, None, "a read without a reference operation is ignored",
         False, None),
        ([lambda ref, c: read(ref, c - 9, "30M", "twin", 0, 32, seq=ref[c - 9:c + 21]),
          lambda ref, c: read(ref, c - 5, "30M", "twin", 0, 32, seq=ref[c - 9:c + 21])], 2, None, "duplicate name:sequence", True, None),
    ], extra=True)


def _zero_length():
    """Reads with a reference-consuming operation of length 0 and no other: ``has_ref``, end == start."""
    return _decline_sites("zero_length", [
        ([lambda ref, c: read(ref, c - 3, "0M5I", "zero_0m5i", 0, 32)], 2, "ValueError", "zero-length alignment 0M5I", True, None),
        ([lambda ref, c: read(ref, c - 3, "5S0D", "zero_5s0d", FREV, 32)], 2, "ValueError", "zero-length alignment 5S0D", True, None),
        ([lambda ref, c: read(ref, c - 17, "0M5I", "zero_at_s0", 0, 32)], 1, None,
         "zero-length alignment exactly at s0: no track on the CPU", False, False),
        ([lambda ref, c: read(ref, c - 3, "0M5I", "zero_masked", FDUP, 32)], 1, None, "zero-length alignment on a duplicate-flagged read",
         False, None),
    ])


def _seq_star():
    """SEQ ``*`` (l_seq = 0) and a SEQ shorter than the CIGAR's query length on a mapped primary read."""
    return _decline_sites("seq_star", [
        ([lambda ref, c: read(ref, c - 10, "20M", "star", 0, 32, seq="")], 2, "ValueError", "SEQ *", True, None),
        ([lambda ref, c: read(ref, c - 10, "5S20M", "short", FREV, 32, seq=ref[c - 10:c + 2])], 2, "ValueError",
         "SEQ shorter than the CIGAR", True, None),
        ([lambda ref, c: read(ref, c - 10, "20M", "star_masked", FDUP, 32, seq="")], 1, None, "SEQ * on a duplicate-flagged read",
         False, None),
    ])


def _window(w):
    ref = make_ref(900, 101)
    reads = [read(ref, 300 + 11 * i, "60M" if i % 2 else "30M2I28M", "w%d" % i, FREV if i % 3 else 0, 20 + i) for i in range(25)]
    locs = [Loc("ref", p, 1, gpu_declines=w > MAX_WINDOW) for p in (420, 450, 500)]
    return Case("window_%d" % w, [("ref", ref)], reads, locs, w=w, max_reads=40)


def _min_base_quality():
    c = _window(16)
    c.name, c.mbq = "min_base_quality_1", 1
    c.locs = [Loc("ref", l.pos, 2, gpu_declines=True) for l in c.locs]
    return c


def _unsorted():
    ref = make_ref(800, 111)
    reads = [read(ref, p, "40M", "u%d" % i, FREV if i % 2 else 0, 20 + i) for i, p in enumerate((300, 280, 320, 290, 310, 100, 330))]
    return Case("unsorted_no_bai", [("ref", ref)], reads, [Loc("ref", 321, 1, gpu_encodes=False), Loc("ref", 121, 0, note="its read lies behind later ones: the forward-moving reader never meets it")],
                w=16, index=False, sort=False, contract_only=True)


_BUILDERS = {}
for _name, _f in ([("contig_edges_w%d" % _w, (lambda _w=_w: _contig_edges(_w))) for _w in (100, 30, 16)] +
                  [("window_edges", _window_edges), ("cigar_shapes", _cigar_shapes)] +
                  [("insertion_caps_%d_%d" % (_a, _b), (lambda _a=_a, _b=_b, _w=_w: _insertion_caps(_a, _b, _w)))
                   for _a, _b, _w in ((10, 50, 100), (3, 5, 16), (0, 0, 16), (10, 4, 30))] +
                  [("qualities", _qualities)] +
                  [("max_reads_%d" % _m, (lambda _m=_m: _max_reads(_m))) for _m in (1, 2, 7, 8)] +
                  [("reference_tokens", _reference_tokens), ("declines", _declines), ("zero_length", _zero_length),
                   ("seq_star", _seq_star), ("window_100", lambda: _window(100)),
                   ("window_101", lambda: _window(101)), ("min_base_quality_1", _min_base_quality),
                   ("unsorted_no_bai", _unsorted), ("depth", _depth)]):
    _BUILDERS[_name] = _f
CASE_NAMES = list(_BUILDERS)


def get_case(name) -> Case:
    case = _BUILDERS[name]()
    assert case.name == name
    return case


# ---- the many-location call (batches of 512, runs cut by gap and span) --------------------------------------------------------
def big_call():
    """-> (Case, contigs, positions): 1 301 locations over two contigs.  "long" (1.3 Mb): 301 locations, ~4 000 bases
    apart (one run until it spans 2^20 bases) with a stretch ~6 000 apart (a run each); "dense" (45 kb): 1 000 locations 41
    apart in ~10x reads.  Reads lie only near locations."""
    long_ref, dense_ref = make_ref(1_300_000, 121), make_ref(45_000, 122)
    reads, pos_long, p = [], [], 500
    for i in range(301):
        pos_long.append(p)
        for j in range(3):
            cigar = ["40M", "18M3I20M", "15M4D21M"][(i + j) % 3]
            reads.append(read(long_ref, p - 30 + 9 * j, cigar, "L%d_%d" % (i, j), FREV if (i + j) % 2 else 0, 5 + (i + 7 * j) % 50))
        p += 6000 + i if 40 <= i < 70 else 3990 + i % 17
    assert p < len(long_ref) and pos_long[-1] - pos_long[0] > (1 << 20)
    for i in range(0, 44_000, 6):
        cigar = ["60M", "25M2I33M", "30M5D25M", "60M", "2S58M"][(i // 6) % 5]
        reads.append(read(dense_ref, i, cigar, "D%d" % i, FREV if (i // 6) % 3 == 0 else (FDUP if i % 100 == 0 else 0), 2 + (i // 6) % 40, tid=1))
    pos_dense = [300 + 41 * i for i in range(1000)]
    case = Case("big_call", [("long", long_ref), ("dense", dense_ref)], reads, [], w=16, max_reads=12)
    return case, ["long"] * 301 + ["dense"] * 1000, pos_long + pos_dense
