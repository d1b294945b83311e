"""Pileup encoder: BAM + candidate VCF -> the candidate records main.py scores.

Restates ``tools/convert_bam_single_reads.py``: the per-location image builder ``process_location`` (:846-1118) with its
helpers ``decode_base_detail`` (:84-147), ``decode_query_sequences`` (:198-224), ``resize_alignment_image`` (:226-254),
``add_bases_to_alignment_image`` (:256-345), ``handle_ended_sequences`` (:347-398), the crop / centre / pad step of
``process_locations_chunk`` (:676-845: ``center_image_on_column`` :400-429, ``trim_empty_rows`` :431-461,
``center_image_on_row_window`` :463-478) and the record layout it saves (:703-708), plus ``get_locations_from_vcf``
(:160-196) on a plain-text VCF.

How a location becomes a record, as the reference does it:

* pileup columns of ``[POS - w - 2, POS + w + 3)`` (0-based, ``w`` = ``--window-size``), one image column per reference
  position plus, behind it, as many columns as the longest insertion any read carries there (capped at
  ``--max-insert-length``, ``--max-insert-length-variant`` on the candidate's own column); reads without that insertion
  get ``noinsert`` (8) in those columns;
* one image row per read, keyed ``name:sequence``, rows in order of first appearance and never re-used; ``start`` (6) in the
  column before a read's first base, ``end`` (7) in the column after its last one (after that column's insertion block);
* three planes: base tokens, base qualities, strand (1 lower / reverse, 2 upper / forward; deletions take the read's strand);
* crop to ``w`` columns either side of the candidate's column, drop leading all-zero rows, keep the middle ``--max-reads``
  rows, pad into ``(max_reads, 2w + 1)``.

Parity: the image logic above is PINNED -- tests/golden/pileup_encoder.json.gz holds outputs of the reference's own helper
functions (executed from its source by oracle/gen_golden_pileup.py on synthetic pileup columns) and of this module's
``process_columns`` glue is compared against a transcription of the reference's loop driven by those helpers.  The BAM side
(dl4vc_amd/bamio.py, dl4vc_amd/pileup.py) is UNPINNED: no htslib / pysam in the image.
Differences kept on purpose: records come out in input order (the reference's ``imap_unordered`` order is arbitrary);
IUPAC ambiguity codes in a read take their strand from their case instead of raising ``KeyError`` (the reference's strand
table has no entry for them, :47-56).
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from .bamio import _CONSUMES_QUERY
from .hdf5_schema import blob_dtype, record_dtype

# token tables (tools/convert_bam_single_reads.py:38-56)
BASE_ENUM = {"A": 1, "a": 1, "T": 2, "t": 2, "U": 2, "u": 2, "G": 3, "g": 3, "C": 4, "c": 4,
             "": 5, "-": 5, "*": 5, "N": 5, "n": 5, "X": 5, "x": 5, ".": 5, ",": 5,
             "start": 6, "e": 7, "end": 7, "noinsert": 8, "pad": 0,
             "unk": 9, "?": 9, "M": 9, "m": 9, "K": 9, "k": 9, "R": 9, "r": 9, "Y": 9, "y": 9,
             "S": 9, "s": 9, "W": 9, "w": 9, "B": 9, "b": 9, "V": 9, "v": 9, "H": 9, "h": 9, "D": 9, "d": 9}
PAD, START, END, NOINSERT = 0, 6, 7, 8
STRAND_PAD, STRAND_LOWER, STRAND_UPPER = 200, 1, 2
_STRAND = {"A": 2, "a": 1, "T": 2, "t": 1, "G": 2, "g": 1, "C": 2, "c": 1, "": 200, "-": 200, "*": 200, "N": 2, "n": 1,
           "M": 2, "m": 1, "?": 200}
_INDEL = re.compile(r"(\d+)(\D+)")


@dataclass
class EncoderOptions:
    """The converter's flags that shape a record (argparse defaults at :481-527; call_variants.sh:87-98 passes
    ``--max-reads 200 --max-insert-length 10 --max-insert-length-variant 50 --save-q-scores --save-strand``)."""
    window_size: int = 100
    max_reads: int = 1000
    max_insert_length: int = 10
    max_insert_length_variant: int = 50
    min_base_quality: int = 0
    # (fraction, seed): read subsampling by name hash (``bamio.SampleRule``), applied by every encoder where a read outside
    # the window is dropped; None = every read
    subsample: Optional[Tuple[float, int]] = None
    # (exclude, require, min_mapq): read filter by flags and mapping quality (``bamio.ReadFilter``), applied by every encoder at
    # the same place in front of the sample rule; None = every read.  read_stats: the native encoders collect the read census
    # without a filter too
    read_filter: Optional[Tuple[int, int, int]] = None
    read_stats: bool = False


def decode_base(base_str: str):
    """(start, base token, deletion length, end, strand, insert tokens) of one read string (:84-147)."""
    start = end = base = deletion = 0
    strand = STRAND_PAD
    insert: List[int] = []
    if base_str[0] == "^":
        if len(base_str) > 1:
            start = ord(base_str[1]) - 10
        else:
            return 1, base, deletion, end, strand, insert
        if len(base_str) > 2:
            base_str = base_str[2:]
        else:
            return start, base, deletion, end, strand, insert
    if base_str[-1] == "$":
        end = 1
        base_str = base_str[:-1]
    c = base_str[0]
    base = BASE_ENUM[c]
    strand = _STRAND[c] if c in _STRAND else (STRAND_UPPER if c.isupper() else STRAND_LOWER if c.islower() else STRAND_PAD)
    if len(base_str) > 1:
        m = _INDEL.match(base_str[2:])
        if base_str[1] == "+":
            insert = [BASE_ENUM[b] for b in m.group(2)]
            assert int(m.group(1)) == len(insert)
        elif base_str[1] == "-":
            deletion = int(m.group(1))
        else:
            raise AssertionError("unparsable indel in |%s|" % base_str)
    return start, base, deletion, end, strand, insert


def _grow(img: np.ndarray, rows: int, cols: int) -> np.ndarray:
    """:226-254: double (at least to the size asked) whichever dimension is too small; new cells are ``pad``."""
    if rows > img.shape[0]:
        new = np.zeros((max(img.shape[0] * 2, rows), img.shape[1]), np.uint8)
        new[:img.shape[0]] = img
        img = new
    if cols > img.shape[1]:
        new = np.zeros((img.shape[0], max(img.shape[1] * 2, cols)), np.uint8)
        new[:, :img.shape[1]] = img
        img = new
    return img


@dataclass
class ColumnInput:
    """What the image builder takes from one pileup column."""
    reference_pos: int
    sequences: Sequence[str]
    qualities: Sequence[int]
    ids: Sequence[str]
    ref_base: str


def process_columns(columns: Iterable[ColumnInput], center_position: int, opt: EncoderOptions):
    """The loop of ``process_location`` (:906-1118) over the columns of one location.  ``center_position`` is the VCF POS
    (1-based).  Returns (bases, centre column, {i: (column, reference position, reference base)}, qualities, strands) or
    None when the candidate's own position has no column (the reference returns ``([], -1, [])``)."""
    window = opt.window_size + 2
    max_var = max(opt.max_insert_length_variant, opt.max_insert_length)
    img = np.zeros((1200, 3 * window), np.uint8)
    qimg = np.zeros_like(img)
    simg = np.zeros_like(img)
    rows: Dict[str, int] = {}
    finished = 0
    idx, prev_col, col = 0, 0, 1
    colmap: Dict[int, Tuple[int, int, str]] = {}
    for c in columns:
        if idx > 1000:
            break
        details = [decode_base(s) for s in c.sequences]
        keep = [i for i, d in enumerate(details) if d[1] != 0]               # (:212-214)
        assert len(keep) == len(c.ids), "mismatch between pileups & sequences"
        details = [details[i] for i in keep]
        quals, ids = c.qualities, c.ids
        need_rows = len(rows) + finished + len(ids) + 1
        need_cols = col + max_var + max(10, max_var)
        img, qimg, simg = _grow(img, need_rows, need_cols), _grow(qimg, need_rows, need_cols), _grow(simg, need_rows, need_cols)
        for name in ids:
            if name not in rows:
                rows[name] = len(rows) + finished
        cap = max_var if c.reference_pos == center_position - 1 else opt.max_insert_length
        # ---- add_bases_to_alignment_image (:256-345)
        r = [rows[name] for name in ids]
        for i, d in enumerate(details):
            img[r[i], col], qimg[r[i], col], simg[r[i], col] = d[1], quals[i], d[4]
        for i, d in enumerate(details):
            if d[0]:
                img[r[i], prev_col], qimg[r[i], prev_col], simg[r[i], prev_col] = START, quals[i], d[4]
        longest = 0
        if cap > 0:
            for i, d in enumerate(details):
                ins = d[5][:cap]
                if ins:
                    img[r[i], col + 1:col + 1 + len(ins)] = ins
                    qimg[r[i], col + 1:col + 1 + len(ins)] = quals[i]
                    simg[r[i], col + 1:col + 1 + len(ins)] = d[4]
                    longest = max(longest, len(ins))
        if longest:
            for ri in r:
                blk = img[ri, col + 1:col + 1 + longest]
                blk[blk == PAD] = NOINSERT
        # ---- handle_ended_sequences (:347-398)
        done = [i for i, d in enumerate(details) if d[3]]
        for i in done:
            e = col + longest + 1
            img[r[i], e], qimg[r[i], e], simg[r[i], e] = END, quals[i], details[i][4]
        for i in set(done):
            rows.pop(ids[i], None)
            finished += 1
        colmap[idx] = (col, c.reference_pos, c.ref_base)
        idx += 1
        prev_col = col
        col = col + 1 + longest
    # deletions ('*') carry no strand: every row takes its own strand, forward when it has none (:1063-1078)
    for k in range(simg.shape[0]):
        row = simg[k]
        pads = row == STRAND_PAD
        if pads.any():
            v = int(row[~pads].max()) if (~pads).any() else 0
            row[pads] = v if v else STRAND_UPPER
    n_rows = len(rows) + finished
    center = -1
    for i in colmap:
        if colmap[i][1] == center_position - 1:
            center = colmap[i][0]
            break
    if center == -1:
        return None
    return img[:n_rows, :col + 1], center, colmap, qimg[:n_rows, :col + 1], simg[:n_rows, :col + 1]


# ---- the same images built read by read (numpy per row instead of Python per pileup entry) --------------------------------
_TOKEN = np.zeros(256, np.uint8)
_KNOWN = np.zeros(256, bool)
for _c, _v in BASE_ENUM.items():
    if len(_c) == 1:
        _TOKEN[ord(_c)], _KNOWN[ord(_c)] = _v, True


def process_tracks(tracks, s0: int, stop: int, center_position: int, opt: EncoderOptions, ref: str, ref_start: int):
    """``process_columns`` for the common case, one read at a time: same result, ~10x faster.  Returns ``NotImplemented`` when
    the location needs the column-by-column path -- two reads sharing a ``name:sequence`` key (they share and swap image
    rows in the reference), a reference skip, a base outside the token table, more than 1000 columns, a depth beyond
    pysam's cap or ``--min-base-quality`` -- so those keep the reference's exact column order of operations.  Raises
    ``ValueError`` (naming the read) for a track the specification has no answer for: a zero-length alignment inside the
    window (``0M 5I``) or a SEQ shorter than the CIGAR's query length (SEQ ``*``)."""
    if opt.min_base_quality > 0 or len(tracks) > 8000:
        return NotImplemented
    tracks = [t for t in tracks if t.end > s0 and t.start < stop]
    for t in tracks:
        # neither has an answer in the specification (pe_encode and the GPU encoder decline them, status 2)
        if t.end <= t.start:
            raise ValueError("read %r at %d: zero-length alignment (CIGAR %s) inside the window of position %d"
                             % (t.rec.name, t.start + 1, t.rec.cigar_string(), center_position))
        n_query = sum(l for op, l in t.rec.cigar if _CONSUMES_QUERY[op])
        if n_query > len(t.rec.seq):
            raise ValueError("read %r at %d: SEQ holds %d bases, its CIGAR %s needs %d (SEQ '*'?)"
                             % (t.rec.name, t.start + 1, len(t.rec.seq), t.rec.cigar_string(), n_query))
    keys = {t.key for t in tracks}
    if len(keys) != len(tracks):
        return NotImplemented
    n_pos = stop - s0
    cover = np.zeros(n_pos + 1, np.int32)
    longest = np.zeros(n_pos, np.int32)
    cap = np.full(n_pos, opt.max_insert_length, np.int32)
    ci = center_position - 1 - s0
    if 0 <= ci < n_pos:
        cap[ci] = max(opt.max_insert_length_variant, opt.max_insert_length)
    spans = []
    for t in tracks:
        lo, hi = max(t.start, s0), min(t.end, stop)
        if t.is_refskip[lo - t.start:hi - t.start].any():
            return NotImplemented
        cover[lo - s0] += 1
        cover[hi - s0] -= 1
        ins = t.indel[lo - t.start:hi - t.start]
        if (ins > 0).any():
            np.maximum(longest[lo - s0:hi - s0], np.minimum(np.maximum(ins, 0), cap[lo - s0:hi - s0]), out=longest[lo - s0:hi - s0])
        spans.append((lo, hi))
    covered = np.cumsum(cover[:-1]) > 0
    pos_idx = np.nonzero(covered)[0]
    if len(pos_idx) == 0 or not (0 <= ci < n_pos and covered[ci]):
        return None
    if len(pos_idx) > 1001:
        return NotImplemented
    width = 1 + longest[pos_idx]
    col_of = np.zeros(n_pos, np.int64)
    col_of[pos_idx] = 1 + np.concatenate(([0], np.cumsum(width)[:-1]))
    prev_col = np.zeros(n_pos, np.int64)
    prev_col[pos_idx] = np.concatenate(([0], col_of[pos_idx][:-1]))
    end_col = int(col_of[pos_idx[-1]] + width[-1])                  # the column the loop would give the next position
    order = sorted(range(len(tracks)), key=lambda i: (spans[i][0], i))
    n_rows = len(tracks)
    n_cols = end_col + 1
    img = np.zeros((n_rows, n_cols), np.uint8)
    qimg = np.zeros_like(img)
    simg = np.zeros_like(img)
    for row, i in enumerate(order):
        t = tracks[i]
        rec = t.rec
        lo, hi = spans[i]
        a, b = lo - t.start, hi - t.start
        cols = col_of[lo - s0:hi - s0]
        qpos, dele = t.qpos[a:b], t.is_del[a:b]
        seq = np.frombuffer(rec.seq.encode("ascii"), np.uint8)
        inside = qpos < len(seq)
        chars = np.where(inside, seq[np.minimum(qpos, len(seq) - 1)], ord("N"))
        if not _KNOWN[chars].all():
            return NotImplemented
        strand = STRAND_LOWER if rec.is_reverse else STRAND_UPPER
        img[row, cols] = np.where(dele, BASE_ENUM["*"], _TOKEN[chars])
        quals = np.where(qpos < len(rec.qual), rec.qual[np.minimum(qpos, len(rec.qual) - 1)], 0).astype(np.uint8)
        qimg[row, cols] = quals
        simg[row, cols] = np.where(dele, STRAND_PAD, strand)
        if t.start >= s0:                                            # head column inside the window
            pc = prev_col[lo - s0]
            img[row, pc], qimg[row, pc], simg[row, pc] = START, quals[0], STRAND_PAD if dele[0] else strand
        ins = t.indel[a:b]
        lg = longest[lo - s0:hi - s0]
        for k in np.nonzero(lg > 0)[0]:
            c0, m = int(cols[k]) + 1, int(lg[k])
            st = STRAND_PAD if dele[k] else strand
            if ins[k] > 0:
                n_ins = min(int(ins[k]), int(cap[lo - s0 + k]))
                if n_ins > 0:
                    q0 = int(qpos[k])
                    letters = [rec.seq[q0 + j] if q0 + j < len(rec.seq) else "N" for j in range(1, n_ins + 1)]
                    toks = _TOKEN[np.frombuffer("".join(letters).encode("ascii"), np.uint8)]
                    if not _KNOWN[np.frombuffer("".join(letters).encode("ascii"), np.uint8)].all():
                        return NotImplemented
                    img[row, c0:c0 + n_ins] = toks
                    qimg[row, c0:c0 + n_ins] = quals[k]
                    simg[row, c0:c0 + n_ins] = st
            blk = img[row, c0:c0 + m]
            blk[blk == PAD] = NOINSERT
        if t.end <= stop:                                            # tail column inside the window
            k = b - a - 1
            e = int(cols[k]) + int(lg[k]) + 1
            img[row, e], qimg[row, e], simg[row, e] = END, quals[k], STRAND_PAD if dele[k] else strand
        pads = simg[row] == STRAND_PAD
        if pads.any():
            rest = simg[row][~pads]
            v = int(rest.max()) if len(rest) else 0
            simg[row][pads] = v if v else STRAND_UPPER
    colmap = {}
    for i, p in enumerate(pos_idx):
        o = s0 + int(p) - ref_start
        colmap[i] = (int(col_of[p]), s0 + int(p), ref[o:o + 1])
    return img, int(col_of[ci]), colmap, qimg, simg


def _trim_top(image: np.ndarray) -> np.ndarray:
    """``trim_empty_rows(image, "top")`` (:431-461): rows before the first one with a non-zero sum go (none when all are zero)."""
    sums = image.sum(axis=1)
    nz = np.nonzero(sums > 0)[0]
    return image[int(nz[0]):] if len(nz) else image


def finish_record(result, location, opt: EncoderOptions, dtype: np.dtype):
    """The per-image part of ``process_locations_chunk`` (:720-838): one structured record, or None where the reference counts
    an error (its planes disagree in shape after trimming, or no read row is left)."""
    bases, center, colmap, quals, strands = result
    w, cols = opt.window_size, 2 * opt.window_size + 1
    ref_line = np.full(bases.shape[1], BASE_ENUM[""], np.uint8)
    for off, _pos, base in colmap.values():
        ref_line[off] = BASE_ENUM[base]
    lo = max(0, center - w)
    hi = min(center + w + 1, bases.shape[1])
    bases, quals, strands = _trim_top(bases[:, lo:hi]), _trim_top(quals[:, lo:hi]), _trim_top(strands[:, lo:hi])
    n = bases.shape[0]
    first = max(0, int((n - opt.max_reads) / 2))
    last = min(first + opt.max_reads, n)
    bases, quals, strands = bases[first:last], quals[first:last], strands[first:last]
    if quals.shape != bases.shape or strands.shape != bases.shape or bases.shape[0] == 0:
        return None
    rec = np.zeros((), dtype)
    off = w - (center - lo)
    k = min(opt.max_reads, bases.shape[0])
    rec["single_reads"][:k, off:off + bases.shape[1]] = bases
    rec["q-scores"][:k, off:off + bases.shape[1]] = quals
    rec["strand"][:k, off:off + bases.shape[1]] = strands
    rec["ref_bases"][off:off + bases.shape[1]] = ref_line[lo:hi]
    rec["num_reads"] = k
    rec["name"] = location.name.encode()[:dtype["name"].itemsize]
    rec["label"] = location.label
    rec["vcfrec"] = location.vcf_string.encode()[:dtype["vcfrec"].itemsize]
    # 'ref' / 'reads' summary planes: NaN for VCF-derived locations in the reference (:195), i.e. zeros once cast
    return rec


@dataclass
class Location:
    contig: str
    pos: int                       # VCF POS (1-based)
    name: str
    label: int
    vcf_string: str


def locations_from_vcf(path: str, label: int, full_vcf: Optional[str] = None) -> List[Location]:
    """``get_locations_from_vcf`` (:160-196) on a plain-text (optionally gzip / BGZF) VCF: one location per record, named
    ``contig:pos``, carrying the record's text (+ ``\\tGT:<genotype>`` when ``full_vcf`` has a genotype for that position)."""
    def lines(p):
        import gzip
        opener = gzip.open if open(p, "rb").read(2) == b"\x1f\x8b" else open
        with opener(p, "rt") as f:
            for line in f:
                if line.strip() and not line.startswith("#"):
                    yield line.rstrip("\r\n")

    genotypes = {}
    if full_vcf:
        for line in lines(full_vcf):
            p = line.split("\t")
            if len(p) >= 10 and p[-2].split(":")[0] == "GT":
                genotypes["%s:%s" % (p[0], p[1])] = "GT:%s" % p[-1].split(":")[0]
    out = []
    for line in lines(path):
        p = line.split("\t")
        name = "%s:%s" % (p[0], p[1])
        text = line.strip()
        if name in genotypes:
            text += "\t%s" % genotypes[name]
        out.append(Location(p[0], int(p[1]), name, label, text))
    return out


def encode_location(bam, fasta, loc: Location, opt: EncoderOptions, reader=None):
    """``process_location`` (:846-1118) for one candidate against an open ``BamFile`` / ``FastaFile``.  ``reader``: a
    ``bamio.WindowReader`` on ``bam`` shared by a run of locations (each alignment is then parsed once, not once per
    location)."""
    from .pileup import pileup_columns, resolve_reads
    window = opt.window_size + 2
    start, stop = loc.pos - window, loc.pos + window + 1
    tid = bam.get_tid(loc.contig)
    if tid < 0:
        return None
    s0 = max(start, 0)
    ref = fasta.fetch(loc.contig, s0, stop + 64)

    tracks = resolve_reads(reader.reads(tid, s0, stop) if reader is not None else bam.fetch(tid, s0, stop))
    fast = process_tracks(tracks, s0, stop, loc.pos, opt, ref, s0)
    if fast is not NotImplemented:
        return fast

    def cols():
        for c in pileup_columns((), s0, stop, tracks=tracks):
            seqs = c.query_sequences(opt.min_base_quality)
            o = c.reference_pos - s0
            yield ColumnInput(c.reference_pos, seqs, c.query_qualities(opt.min_base_quality), c.query_ids(opt.min_base_quality),
                              ref[o:o + 1])
    return process_columns(cols(), loc.pos, opt)


def _add_counts(total: dict, part: dict) -> None:
    for k, v in part.items():
        total[k] = total.get(k, 0) + v


def encode_locations(bam_path: str, fasta_path: str, locations: Sequence[Location], opt: EncoderOptions,
                     native: Optional[bool] = None, threads: int = 1, device: Optional[str] = None,
                     device_id: int = 0, inflate_device: Optional[str] = None, compress_device: Optional[str] = None,
                     pending: int = 0, records_per_chunk: int = 8, compress_codes: str = "fixed", subsample=None,
                     read_stats: Optional[dict] = None):
    """Records for ``locations`` in input order and the number of locations that produced none.

    ``read_stats`` (a dict, with ``opt.read_filter`` or ``opt.read_stats``): the read census of this call is added to it
    (``read_*`` entries, ``read_filter.census_of``) -- the GPU encoder's over all locations with ``device="gpu"``, else
    ``pe_encode``'s; the Python builder keeps none.

    ``subsample=(fraction, seed)``: ``opt.subsample`` for this call -- every encoder below drops the reads the rule drops
    (``bamio.SampleRule``), so the records are those of the BAM ``tools/subsample_bam.py`` writes (tests/test_subsample_*.py).

    ``native`` (default: when libdl4vc_loader.so is built): the image planes come from the C++ encoder (``pe_encode``:
    BGZF / BAM / CIGAR / image builder in ``threads`` worker threads); a location it declines (status 2: the cases
    ``process_tracks`` hands to the column-by-column builder) is encoded here, so the records are the same bytes either
    way (tests/test_pileup_native.py).

    ``device="gpu"`` (default None: the host encoders above): the planes come from the GPU encoder (libdl4vc_pileup.so on HIP device ``device_id``) first; what it
    declines goes to ``pe_encode``, and what that declines to the Python encoder -- the same bytes and error count as
    ``native=True`` (tests/test_pileup_gpu.py).  A missing libdl4vc_pileup.so is an error, not a fall-back.
    ``inflate_device="gpu"`` (with ``device="gpu"`` only): the GPU encoder inflates the BAM's BGZF blocks and frames its records on
    the device as well (needs the ``.bai``; same bytes, tests/test_pileup_inflate_gpu.py).

    ``compress_device="gpu"`` (with ``device="gpu"`` only): instead of the record array, a generator of ``EncodedBatch`` -- one
    per ``COMPRESS_BATCH`` locations -- whose records were packed into the HDF5 compound layout and compressed into the
    dataset's chunks on the device (``pg_compress_records_device``); only the compressed bytes come to the host, and no record
    array of the whole step is ever held.  ``pending``: the records a ``hdf5io.ChunkWriter`` already carries; each batch hands
    the few records in front of and behind its whole chunks over as ordinary records (``head`` / ``tail``), so every compressed
    chunk starts at a multiple of ``records_per_chunk`` (tests/test_compress_gpu.py).  ``compress_codes``: ``"fixed"`` or
    ``"dynamic"`` (with ``compress_device="gpu"`` only), the Huffman codes of those chunks (tests/test_compress_dynamic_gpu.py).

    Raises ``ValueError`` naming the read where a location's window holds a read the specification has no answer for (a
    zero-length alignment such as ``0M 5I``, a SEQ shorter than the CIGAR's query length such as SEQ ``*``): the native and
    GPU encoders decline such a location, so all three paths end here (tests/test_pileup_edges.py)."""
    from . import loader
    if subsample is not None:
        from dataclasses import replace
        from .bamio import SampleRule
        rule = SampleRule.of(subsample)
        opt = replace(opt, subsample=(rule.fraction, rule.seed))
    if device not in (None, "gpu"):
        raise ValueError("device must be None (host encoders) or 'gpu', not %r" % (device,))
    if inflate_device not in (None, "gpu"):
        raise ValueError("inflate_device must be None or 'gpu', not %r" % (inflate_device,))
    if inflate_device == "gpu" and device != "gpu":
        raise ValueError("inflate_device='gpu' is the GPU pileup encoder's option: it needs device='gpu'")
    if compress_device not in (None, "gpu"):
        raise ValueError("compress_device must be None or 'gpu', not %r" % (compress_device,))
    if compress_codes not in ("fixed", "dynamic"):
        raise ValueError("compress_codes must be 'fixed' or 'dynamic', not %r" % (compress_codes,))
    if compress_codes != "fixed" and compress_device != "gpu":
        raise ValueError("compress_codes=%r is the device compressor's option: it needs compress_device='gpu'" % (compress_codes,))
    if compress_device == "gpu":
        if device != "gpu":
            raise ValueError("compress_device='gpu' compresses the GPU pileup encoder's planes where they lie: it needs device='gpu'")
        return _encode_compressed(bam_path, fasta_path, locations, opt, threads, device_id, inflate_device, pending, records_per_chunk,
                                  compress_codes)
    from .location_round import HostEncoders, declined, record_members
    W = 2 * opt.window_size + 1
    dtype, bdt = record_dtype(opt.max_reads, W), blob_dtype(W)
    n = len(locations)
    use_native = loader.available() if native is None else native
    # the planes of the locations the GPU encoder takes (flag 1), then of those the host encoders take of the rest, in location order
    gpu = np.zeros(n, bool)
    ref, num = np.zeros((n, W), np.uint8), np.zeros(n, np.int32)
    rest = np.arange(n)
    if device == "gpu" and n:
        from . import pileup_gpu
        with pileup_gpu.GpuPileupEncoder.from_options(bam_path, fasta_path, opt, device_id, inflate_device) as enc:
            reads, qual, strand, ref, num, status = enc.encode([l.contig for l in locations], [l.pos for l in locations])
            if read_stats is not None:
                _add_counts(read_stats, enc.read_stats())
        gpu, rest = status == 1, declined(status)
    host = {}
    if len(rest):
        encoders = HostEncoders(bam_path, fasta_path, opt, threads, native=use_native or device == "gpu")
        try:
            host = encoders.encode(locations, rest)
            if read_stats is not None and device != "gpu" and encoders.cpu is not None:
                _add_counts(read_stats, encoders.cpu.read_stats())
        finally:
            encoders.close()
    keep = np.array([i for i in range(n) if gpu[i] or i in host], np.int64)
    out = np.zeros(len(keep), dtype)
    for k, i in enumerate(keep):
        if gpu[i]:
            out["single_reads"][k], out["q-scores"][k], out["strand"][k] = reads[i], qual[i], strand[i]
        else:               # (popped: a record of the Python builder is held only until it is copied)
            out["single_reads"][k], out["q-scores"][k], out["strand"][k], ref[i], num[i] = host.pop(int(i))
    blob = record_members(locations, keep, ref, num, bdt)
    for name in bdt.names:
        out[name] = blob[name]
    return out, n - len(keep)


COMPRESS_BATCH = 4096          # locations per device batch of encode_locations(compress_device="gpu")


@dataclass
class EncodedBatch:
    """One batch of ``encode_locations(compress_device="gpu")``, in the order it goes to a ``hdf5io.ChunkWriter``:
    ``append_records(head)``, ``write_chunks(chunks)`` (None where the batch holds no whole chunk), ``append_records(tail)``."""
    head: np.ndarray
    chunks: object
    tail: np.ndarray
    records: int
    errors: int
    stats: dict


def _encode_compressed(bam_path, fasta_path, locations, opt, threads, device_id, inflate_device, pending, chunk, codes):
    import torch
    from .location_round import LocationRounds, record_members
    W = 2 * opt.window_size + 1
    dtype, bdt = record_dtype(opt.max_reads, W), blob_dtype(W)
    if not len(locations):
        return
    dev = torch.device("cuda", device_id)
    B = min(COMPRESS_BATCH, len(locations))
    rounds = LocationRounds(bam_path, fasta_path, opt, B, device_id, inflate_device=inflate_device, compress_codes=codes, threads=threads)
    try:
        for l0 in range(0, len(locations), B):
            locs = locations[l0:l0 + B]
            ref, num, status = rounds.encode(locs)
            reads, qual, strand = (p[:len(locs)] for p in rounds.stored)
            stats = rounds.last_stats()
            keep = np.flatnonzero(status == 1)
            m = len(keep)
            blob = record_members(locs, keep, ref, num, bdt)

            def records(lo, hi):
                out = np.zeros(hi - lo, dtype)
                if hi > lo:
                    idx = torch.from_numpy(keep[lo:hi]).to(dev)
                    for name, plane in zip(("single_reads", "q-scores", "strand"), (reads, qual, strand)):
                        out[name] = plane[idx].cpu().numpy()
                    for name in bdt.names:
                        out[name] = blob[name][lo:hi]
                return out

            n_head = min((chunk - pending) % chunk, m)
            n_tail = (m - n_head) % chunk
            head, tail = records(0, n_head), records(m - n_tail, m)
            chunks = None
            if m - n_tail > n_head:
                chunks = rounds.enc.compress_records((reads, qual, strand), keep[n_head:m - n_tail], blob[n_head:m - n_tail], chunk)
                stats = rounds.last_stats()
            pending = (pending + m) % chunk
            yield EncodedBatch(head, chunks, tail, m, int((status == 0).sum()), stats)
    finally:
        rounds.close()
