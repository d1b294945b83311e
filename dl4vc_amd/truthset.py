"""Comparison against a truth VCF, host side: the record reader, ``bcftools isec``'s default pairing, and the variant-type
counts, precision-recall curve and best-F1 search of the reference's evaluation tools (``tools/called_variant_metrics.py``,
``tools/threshold.py``).  Used by ``tools/vcf_isec.py``, ``tools/called_variant_metrics.py``, ``tools/threshold.py`` and
``tools/make_training_data.sh``.

The pairing rule is ``bcftools isec``'s default collapse mode (``-c none``: "only records with identical REF and ALT alleles
are compatible"), restated from the manual:

* two records pair when CHROM, POS, REF and the set of ALT alleles are equal.  A candidate ``A>G`` therefore does NOT pair
  with a truth record ``A>G,T`` (a 1/2 truth site): both stay private.  For training data this means such a truth site gives
  no true-positive candidate; the candidate is labelled a false positive;
* within one file, records with the same key pair one-for-one in file order; the rest are private;
* FILTER is ignored;
* every output keeps its own input's record order and its input's header lines;
* both inputs must be position-sorted (contig order from ``##contig`` lines, else from first appearance); an unsorted input
  is refused, never paired.

With ``left_align`` (``--left-align REF.fa`` of the tools) the simple indels of BOTH inputs are left-aligned on the FASTA before
their keys are made (``left_align_record``: the rule of ``csrc/cand_left_align.h`` with floor 0, restated here in Python), so a
record placed to the right inside a repeat pairs with its left-aligned twin.  Only the keys move: every output line is still its
input's line, byte for byte.  MNPs, complex alleles and multi-allelic records are compared as they are; this is no
haplotype-aware comparison.

UNPINNED: there is no bcftools here, so the pairing rule is checked against hand-written cases only.
The counting, the curve, the F1 search and the printing are pinned to the reference's own code by
``tools/gen_golden_evaluation.py``.
"""
from __future__ import annotations

import bisect
import gzip
import os
from typing import Callable, Dict, Iterator, List, Optional, Tuple

import numpy as np

# (line, chrom, pos, ref, alts): line is the input's text unchanged, its line ending included; alts is () for ALT '.'
Record = Tuple[str, str, int, str, Tuple[str, ...]]


class VcfError(ValueError):
    pass


def open_text_lines(path: str) -> Iterator[str]:
    """The lines of a plain, gzip or BGZF text file, each with its line ending, split on '\\n' only.  BCF is refused."""
    with open(path, "rb") as raw:
        magic = raw.read(2)
    fh = gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")
    with fh:
        head = fh.peek(3)[:3] if hasattr(fh, "peek") else b""
        if head == b"BCF":
            raise VcfError("%s is BCF (binary VCF), which is not read here: convert it to VCF text (.vcf or .vcf.gz) first"
                           % path)
        for b in fh:
            yield b.decode("utf-8")


class VcfReader:
    """A VCF's header lines (verbatim, in order) and its records, checked for position order.

    ``header`` is read on construction.  Iterate once: each record is ``(line, chrom, pos, ref, alts)``.  Records out of
    order raise ``VcfError`` naming the file and the line."""

    def __init__(self, path: str):
        self.path = path
        self.header: List[str] = []
        self._lines = open_text_lines(path)
        self._contigs: Dict[str, int] = {}
        self._first: Optional[str] = None
        for line in self._lines:
            if line.startswith("#"):
                self.header.append(line)
                if line.startswith("##contig=<"):
                    cid = _contig_id(line)
                    if cid is not None and cid not in self._contigs:
                        self._contigs[cid] = len(self._contigs)
            else:
                self._first = line
                break

    def __iter__(self) -> Iterator[Record]:
        contigs = self._contigs
        cur_chrom, cur_idx, cur_pos = None, -1, 0
        n = len(self.header)

        def body():
            if self._first is not None:
                yield self._first
            yield from self._lines

        for line in body():
            n += 1
            if not line.strip():
                continue
            f = line.rstrip("\r\n").split("\t", 5)
            if len(f) < 5:
                raise VcfError("%s:%d: a VCF record needs at least 5 tab-separated columns" % (self.path, n))
            chrom = f[0]
            try:
                pos = int(f[1])
            except ValueError:
                raise VcfError("%s:%d: POS %r is not an integer" % (self.path, n, f[1])) from None
            if chrom != cur_chrom:
                idx = contigs.get(chrom)
                if idx is None:
                    idx = contigs[chrom] = len(contigs)
                if idx < cur_idx:
                    raise VcfError("%s:%d: not sorted: contig %s comes after %s (contig order %s); sort the file first"
                                   % (self.path, n, chrom, cur_chrom,
                                      "of the ##contig lines" if self._header_contigs() else "of first appearance"))
                cur_chrom, cur_idx, cur_pos = chrom, idx, pos
            elif pos < cur_pos:
                raise VcfError("%s:%d: not sorted: %s:%d comes after %s:%d; sort the file first"
                               % (self.path, n, chrom, pos, chrom, cur_pos))
            cur_pos = pos
            alt = f[4]
            yield line, chrom, pos, f[3], (() if alt == "." else tuple(alt.split(",")))

    def _header_contigs(self) -> bool:
        return any(h.startswith("##contig=<") for h in self.header)


def _contig_id(line: str) -> Optional[str]:
    body = line[len("##contig=<"):].rstrip("\r\n").rstrip(">")
    for kv in body.split(","):
        if kv.startswith("ID="):
            return kv[3:]
    return None


def _key(rec: Record):
    alts = rec[4]
    return rec[1], rec[2], rec[3], alts if len(alts) < 2 else tuple(sorted(set(alts)))


# --- left-alignment ------------------------------------------------------------------------------------------------------------
LA_INS, LA_DEL = 1, 2


def left_align_letters(ref_at: Callable[[int], str], length: int, kind: int, a: int, anchor: str, bases: str, floor: int = 0,
                       anchor_aligned: bool = True) -> Tuple[int, str, str, bool, bool]:
    """The left-alignment rule for one indel observation, on letters: ``ref_at(p)`` is the contig's letter at 0-based ``p`` as
    the allele walk sees it (upper case, N for a byte outside the alphabet) for ``0 <= p < length``; ``a`` / ``anchor`` the anchor
    position and base; ``bases`` the inserted read bases (``LA_INS``) or the deleted reference bases (``LA_DEL``); ``floor`` the
    read's POS.  Returns ``(pos, anchor, bases, eligible, clamped)``: the left-most placement, whether the observation was
    eligible at all (else it comes back as it went in), and whether the shift stopped at ``floor`` where floor 0 would have let it
    go on.  The restatement the C++ rule (``csrc/cand_left_align.h``) is held to; it rotates the string where that indexes."""
    L = len(bases)
    acgt = set("ACGT")
    same = (a, anchor, bases, False, False)
    if not anchor_aligned or L < 1 or kind not in (LA_INS, LA_DEL) or not 0 <= a < length:
        return same
    if anchor not in acgt or any(c not in acgt for c in bases) or ref_at(a) != anchor:
        return same
    if kind == LA_DEL and (a + L >= length or any(ref_at(a + 1 + j) != bases[j] for j in range(L))):
        return same
    floor = max(0, floor)
    k, s, clamped = 0, bases, False
    while True:
        p = a - k
        if p - 1 < 0 or ref_at(p - 1) not in acgt:
            break
        if ref_at(p) != (ref_at(p + L) if kind == LA_DEL else s[-1]):
            break
        if p - 1 < floor:
            clamped = True
            break
        k += 1
        s = s[-1] + s[:-1]
    p = a - k
    if kind == LA_DEL:
        s = "".join(ref_at(p + 1 + j) for j in range(L))
    return p, ref_at(p), s, True, clamped


class _ContigLetters:
    """``ref_at`` over one contig of a ``bamio.FastaFile``, fetched in blocks."""
    BLOCK = 1024

    def __init__(self, fasta, chrom: str):
        self.fasta, self.chrom, self.blocks = fasta, chrom, {}
        self.length = fasta.get_reference_length(chrom)

    def __call__(self, p: int) -> str:
        b = p // self.BLOCK
        if b not in self.blocks:
            if len(self.blocks) > 64:
                self.blocks.clear()
            raw = self.fasta.fetch(self.chrom, b * self.BLOCK, (b + 1) * self.BLOCK).upper()
            self.blocks[b] = "".join(c if c in "=ACMGRSVTWYHKDBN" else "N" for c in raw)
        return self.blocks[b][p - b * self.BLOCK]


def left_align_record(fasta, chrom: str, pos: int, ref: str, alt):
    """``(pos, ref, alt)`` of a VCF record (1-based ``pos``) with a simple indel moved to its left-most placement on ``fasta`` (a
    ``bamio.FastaFile``): the rule of ``left_align_letters`` with floor 0.  Simple means one ALT allele, one of REF / ALT of
    length 1, and both starting with the same base.  Everything else passes through untouched: SNPs, MNPs, complex alleles,
    multi-allelic records (``alt`` a tuple of several, or a string with a comma), a contig the FASTA lacks, and an indel whose
    bases are not ACGT or whose REF differs from the FASTA.  ``alt`` comes back in the form it came in."""
    one = alt[0] if isinstance(alt, (tuple, list)) and len(alt) == 1 else alt
    if not isinstance(one, str) or "," in one or not ref or not one or ref[0].upper() != one[0].upper():
        return pos, ref, alt
    if not ((len(ref) == 1) != (len(one) == 1)):
        return pos, ref, alt
    cache = fasta.__dict__.setdefault("_left_align_contigs", {})
    if chrom not in cache:
        try:
            cache[chrom] = _ContigLetters(fasta, chrom)
        except KeyError:
            cache[chrom] = None
    letters = cache[chrom]
    if letters is None:
        return pos, ref, alt
    kind = LA_INS if len(ref) == 1 else LA_DEL
    bases = (one if kind == LA_INS else ref)[1:].upper()
    p, anchor, s, eligible, _ = left_align_letters(letters, letters.length, kind, pos - 1, ref[0].upper(), bases, 0)
    if not eligible or p == pos - 1:
        return pos, ref, alt
    new_ref, new_alt = (anchor, anchor + s) if kind == LA_INS else (anchor + s, anchor)
    return p + 1, new_ref, (type(alt)([new_alt]) if isinstance(alt, (tuple, list)) else new_alt)


def record_left_aligner(fasta_path: str) -> Callable[[Record], Record]:
    """``normalise`` for ``isec_stream``: a record with its key fields left-aligned on the FASTA, its line unchanged."""
    from .bamio import FastaFile
    fasta = FastaFile(fasta_path)

    def normalise(rec: Record) -> Record:
        pos, ref, alts = left_align_record(fasta, rec[1], rec[2], rec[3], rec[4])
        return rec[0], rec[1], pos, ref, alts
    return normalise


# output numbers, as bcftools isec -p names them
PRIVATE_A, PRIVATE_B, SHARED_A, SHARED_B = 0, 1, 2, 3


def isec_stream(a: str, b: str, emit: Callable[[int, Record], None],
                headers: Optional[Callable[[List[str], List[str]], None]] = None,
                normalise: Optional[Callable[[Record], Record]] = None) -> Tuple[int, int, int, int]:
    """Pairs the records of VCF ``a`` with those of VCF ``b`` (module docstring) and hands each record to
    ``emit(output, record)``, ``output`` one of PRIVATE_A / PRIVATE_B / SHARED_A / SHARED_B.  Every output receives its
    records in its input's order; all of B's records come before A's.  ``headers(header_a, header_b)`` is called once, before
    the first ``emit``.  Memory holds A's keys only; A is read twice, B once.  Returns the four record counts.
    ``normalise(record)``: the record whose fields make the key (``record_left_aligner``); ``emit`` still gets the input's own."""
    key = _key if normalise is None else (lambda r: _key(normalise(r)))
    ra = VcfReader(a)
    count_a: Dict[tuple, int] = {}
    for rec in ra:
        k = key(rec)
        count_a[k] = count_a.get(k, 0) + 1
    rb = VcfReader(b)
    seen_b: Dict[tuple, int] = {}
    counts = [0, 0, 0, 0]
    started = False
    for rec in rb:
        if not started:
            if headers is not None:
                headers(ra.header, rb.header)
            started = True
        k = key(rec)
        avail = count_a.get(k, 0)
        out = PRIVATE_B
        if avail:
            used = seen_b.get(k, 0)
            if used < avail:
                out = SHARED_B
                seen_b[k] = used + 1
        counts[out] += 1
        emit(out, rec)
    if not started and headers is not None:
        headers(ra.header, rb.header)
    seen_a: Dict[tuple, int] = {}
    for rec in VcfReader(a):
        k = key(rec)
        shared = seen_b.get(k, 0)
        out = PRIVATE_A
        if shared:
            used = seen_a.get(k, 0)
            if used < shared:
                out = SHARED_A
                seen_a[k] = used + 1
        counts[out] += 1
        emit(out, rec)
    return tuple(counts)


def isec(a: str, b: str, left_align: Optional[str] = None) -> Tuple[List[Record], List[Record], List[Record], List[Record]]:
    """``(private_a, private_b, shared_a, shared_b)``: bcftools isec -p's 0000 / 0001 / 0002 / 0003 as record lists.
    ``left_align="ref.fa"``: the simple indels of both inputs are left-aligned on it before pairing."""
    outs: Tuple[List[Record], ...] = ([], [], [], [])
    isec_stream(a, b, lambda o, r: outs[o].append(r), normalise=record_left_aligner(left_align) if left_align else None)
    return outs


def isec_to_dir(a: str, b: str, outdir: str, left_align: Optional[str] = None) -> Tuple[int, int, int, int]:
    """Writes ``outdir/0000.vcf`` .. ``0003.vcf`` (each with its input's header, record lines copied byte for byte) and
    ``outdir/README.txt``.  On a refused input the four files are removed again.  ``left_align="ref.fa"``: the simple indels of
    both inputs are left-aligned on it before pairing (the lines written are still the inputs' own)."""
    normalise = record_left_aligner(left_align) if left_align else None
    os.makedirs(outdir, exist_ok=True)
    paths = [os.path.join(outdir, "%04d.vcf" % i) for i in range(4)]
    files = [open(p, "w", encoding="utf-8", newline="") for p in paths]
    try:
        def headers(ha, hb):
            for i, h in enumerate((ha, hb, ha, hb)):
                files[i].writelines(h)

        counts = isec_stream(a, b, lambda o, r: files[o].write(r[0]), headers, normalise)
    except BaseException:
        for f in files:
            f.close()
        for p in paths:
            os.remove(p)
        raise
    for f in files:
        f.close()
    with open(os.path.join(outdir, "README.txt"), "w") as f:
        f.write("This file was produced by vcf_isec.py, the bcftools isec -p restatement of this repository.\n"
                "The command line was:\tvcf_isec.py -p %s %s%s %s\n\n"
                "Using the following file names:\n"
                "%s\tfor records private to\t%s\n"
                "%s\tfor records private to\t%s\n"
                "%s\tfor records from %s shared by both\t%s %s\n"
                "%s\tfor records from %s shared by both\t%s %s\n"
                % (outdir, "--left-align %s " % left_align if left_align else "", a, b, paths[0], a, paths[1], b, paths[2], a, a, b, paths[3], b, a, b))
    return counts


# --- called_variant_metrics.py -----------------------------------------------------------------------------------------

def count_variant_types(records, chrom: Optional[str], start: Optional[int], end: Optional[int],
                        out: Callable[[str], None] = print) -> Tuple[int, int, int]:
    """(substitutions, insertions, deletions) of ``records`` ((chrom, pos, ref, alts) tuples), classified by
    REF and ``alts[0]`` only; anything else is printed as the reference prints it (``Unknown alelle: ...``) and not counted.
    With ``chrom`` set, records with ``contig != chrom or pos < start or pos > end`` (1-based POS) are skipped."""
    snp = ins = dele = 0
    for contig, pos, ref, alts in records:
        if chrom is not None and (contig != chrom or pos < start or pos > end):
            continue
        if not alts:
            raise VcfError("%s:%d has no ALT allele ('.'): the reference tool cannot classify it either" % (contig, pos))
        if len(ref) == 1 and len(alts[0]) == 1:
            snp += 1
        elif len(ref) == 1 and len(alts[0]) > 1:
            ins += 1
        elif len(ref) > 1 and len(alts[0]) == 1:
            dele += 1
        else:
            out("Unknown alelle: {} -> {}".format(ref, alts))
    return snp, ins, dele


class BedRegions:
    """A BED file's intervals, 0-based half-open, merged per contig.  ``contains(chrom, pos)`` tests the 1-based VCF POS,
    i.e. 0-based ``pos - 1``."""

    def __init__(self, path: str):
        iv: Dict[str, List[Tuple[int, int]]] = {}
        for line in open_text_lines(path):
            if not line.strip() or line.startswith(("#", "track", "browser")):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 3:
                raise VcfError("%s: a BED line needs chrom, start and end: %r" % (path, line.rstrip()))
            iv.setdefault(f[0], []).append((int(f[1]), int(f[2])))
        self._starts: Dict[str, List[int]] = {}
        self._ends: Dict[str, List[int]] = {}
        for c, lst in iv.items():
            lst.sort()
            s_out, e_out = [], []
            for s, e in lst:
                if e <= s:
                    continue
                if s_out and s <= e_out[-1]:
                    e_out[-1] = max(e_out[-1], e)
                else:
                    s_out.append(s)
                    e_out.append(e)
            self._starts[c], self._ends[c] = s_out, e_out

    def contains(self, chrom: str, pos: int) -> bool:
        starts = self._starts.get(chrom)
        if not starts:
            return False
        p = pos - 1
        i = bisect.bisect_right(starts, p) - 1
        return i >= 0 and p < self._ends[chrom][i]


def ratio(num: int, den: int) -> float:
    """``num / den``; ``nan`` where the reference divides by zero (and stops with ZeroDivisionError)."""
    return num / den if den else float("nan")


# --- threshold.py --------------------------------------------------------------------------------------------------------

def _binary_clf_curve(labels, scores):
    """sklearn's ``_binary_clf_curve`` without weights: descending stable order (``argsort(kind="mergesort")[::-1]``),
    one point per distinct score."""
    y_true = np.asarray(labels).ravel()
    y_score = np.asarray(scores).ravel()
    if y_true.shape != y_score.shape:
        raise ValueError("Found input variables with inconsistent numbers of samples: [%d, %d]" % (y_true.size, y_score.size))
    if not np.all(np.isfinite(y_score)):
        raise ValueError("Input contains NaN, infinity or a value too large for dtype('float64').")
    classes = np.unique(y_true)
    if not any(np.array_equal(classes, c) for c in ([0, 1], [-1, 1], [0], [-1], [1])):
        raise ValueError("Data is not binary and pos_label is not specified")
    y_true = y_true == 1
    order = np.argsort(y_score, kind="mergesort")[::-1]
    y_score = y_score[order]
    y_true = y_true[order]
    distinct = np.where(np.diff(y_score))[0]
    idx = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true * 1.0, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    return fps, tps, y_score[idx]


def precision_recall_curve(labels, scores, truncate_at_full_recall: bool = True):
    """``sklearn.metrics.precision_recall_curve(labels, scores)`` restated in numpy; thresholds ascending.

    ``truncate_at_full_recall=True`` is scikit-learn 0.22-0.24, the version the reference's ``sklearn==0.0`` pin resolved to:
    the curve stops at the first threshold that reaches full recall, and with no positive label recall is ``nan``.
    ``False`` is scikit-learn >= 1.1 (1.7.2 checked): every distinct score is a threshold, and with no positive label recall is
    1 everywhere."""
    fps, tps, thresholds = _binary_clf_curve(labels, scores)
    with np.errstate(divide="ignore", invalid="ignore"):
        if truncate_at_full_recall:
            precision = tps / (tps + fps)
            precision[np.isnan(precision)] = 0
            recall = tps / tps[-1]
            sl = slice(int(tps.searchsorted(tps[-1])), None, -1)
        else:
            ps = tps + fps
            precision = np.zeros_like(tps)
            np.divide(tps, ps, out=precision, where=(ps != 0))
            recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
            sl = slice(None, None, -1)
    return np.r_[precision[sl], 1], np.r_[recall[sl], 0], thresholds[sl]


def optimal_threshold(labels, scores, truncate_at_full_recall: bool = True, out: Callable[[str], None] = print):
    """The reference's ``get_optimal_threshold``: prints the sizes, the first point at or above each of 0.3 / 0.5 / 0.7 and
    the best-F1 point (first of equal maxima; ``nan`` F1 never wins, and with none left the last threshold is reported with
    F1 -1), and returns the best threshold."""
    out("optimal thresholds for %d labels %d scores" % (len(labels), len(scores)))
    precision, recall, thresholds = precision_recall_curve(labels, scores, truncate_at_full_recall)
    n = len(thresholds)
    p, r = precision[:n], recall[:n]
    with np.errstate(divide="ignore", invalid="ignore"):
        f1 = 2 * (p * r) / (p + r)
    for level in (0.3, 0.5, 0.7):
        hit = np.flatnonzero(thresholds >= level)
        if hit.size:
            i = hit[0]
            out("\tthreshold %f: F1 %f (prec: %f; recall: %f)" % (thresholds[i], f1[i], precision[i], recall[i]))
    valid = ~np.isnan(f1)
    if valid.any():
        best_i = int(np.flatnonzero(valid)[np.argmax(f1[valid])])
        best_f1 = f1[best_i]
    else:
        best_i, best_f1 = -1, -1
    best = thresholds[best_i]
    out("Best threshold %f: F1 %f (prec: %f; recall: %f)" % (best, best_f1, precision[best_i], recall[best_i]))
    return best


def canonicalize_bases(ref: str, var: str) -> Tuple[str, str]:
    """Drops the common suffix of length ``min(len) - 1`` from a REF / ALT pair (both longer than 1); a suffix that is not
    common fails the assertion, as in the reference."""
    trim = min(len(ref), len(var)) - 1
    if trim == 0:
        return ref, var
    assert ref[-trim:] == var[-trim:]
    return ref[:-trim], var[:-trim]
