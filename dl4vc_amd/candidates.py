"""Candidate generation, host side: BAM -> ``candidates.vcf`` (the first stage of ``call_variants.sh``; reference
``tools/candidate_generator.py`` and ``tools/bedutils.py``).

The per-read work and the per-locus counts run in ``libdl4vc_cand.so`` (``dl4vc_amd/candgen.py``); this module holds what
stays on the host: the regions (whole BAM, ``--contigs``, BED intersection with its ``chr`` handling), their split into
subregions and groups, the multi-allele rule, and the VCF text and order.

Semantics restated from the reference (DESIGN.md section 9 lists them with the deliberate divergences):

* alleles are counted per subregion: reads are fetched over ``[start, end)`` but an allele counts at ``start <= pos <= end``,
  so an allele on a boundary can be written twice, once per subregion, with different DP / AF;
* ``af = min(count, depth) / depth`` (double), kept when ``af > min_freq`` (strictly); depth 0 is skipped;
* without ``keep_multialleles`` each subregion keeps, per position, the first allele (in tuple order) with the highest AF;
* records are ``chrom POS+1 . REF ALT 50 . DP=d;AF=af GT:GQ 1:50`` with AF a float32 printed like C ``%g``; the merged file is
  ordered as ``sort -k1,1 -k2,2n`` orders it in the C locale (chrom bytes, POS as a number, then the whole line).

UNPINNED: the header and the float text are written from the VCF specification and htslib's conventions; there is no
pysam / htslib here to compare them with.
"""
from __future__ import annotations

import json
import logging
import os
from collections import OrderedDict, namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

BedInterval = namedtuple("BedInterval", ["chrom", "start", "stop"])
Region = Tuple[str, int, int]

VCF_HEADER_FIXED = (
    "##fileformat=VCFv4.2",
    '##FILTER=<ID=PASS,Description="All filters passed">',
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Genotype Quality">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    '##INFO=<ID=DP,Number=1,Type=Integer,Description="Total Depth">',
    '##INFO=<ID=AF,Number=A,Type=Float,Description="Allele Frequency">',
)
VCF_COLUMNS = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED"


# ---- regions ----------------------------------------------------------------------------------------------------------------
def read_bed(path: str) -> Dict[str, List[BedInterval]]:
    """Tab-separated chrom, start, stop per line, grouped by chrom in file order (blank lines skipped)."""
    out: Dict[str, List[BedInterval]] = OrderedDict()
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            col = line.split("\t")
            out.setdefault(col[0], []).append(BedInterval(col[0], int(col[1]), int(col[2])))
    return out


def intersect_interval(a: BedInterval, b: BedInterval) -> Optional[BedInterval]:
    """The reference's four-case overlap of two intervals (a partial overlap keeps a's chrom; full containment returns
    the contained interval itself; anything else, touching ends included, is no overlap)."""
    if a.chrom != b.chrom:
        return None
    if a.start <= b.start < a.stop < b.stop:
        return BedInterval(a.chrom, b.start, a.stop)
    if b.start <= a.start < b.stop < a.stop:
        return BedInterval(a.chrom, a.start, b.stop)
    if a.start >= b.start and a.stop <= b.stop:
        return a
    if b.start >= a.start and b.stop <= a.stop:
        return b
    return None


def _strip_chr(name: str) -> str:
    return name[3:] if name.startswith("chr") else name


def contig_regions(references: Sequence[str], lengths: Sequence[int], contigs: Optional[str] = None,
                   bedfile: Optional[str] = None, keep_contig_chr: bool = False) -> List[Region]:
    """Whole BAM, ``--contigs c[:s:e],...`` (anything but three fields means the whole contig), then, with a BED file, the
    intersection with its intervals: contig names lose a leading ``chr`` to match the BED's, and regain it with
    ``keep_contig_chr``."""
    length_of = dict(zip(references, lengths))
    regions: List[Region] = []
    if contigs is None:
        regions = [(c, 0, length_of[c]) for c in references]
    else:
        for item in contigs.split(","):
            f = item.split(":")
            regions.append((f[0], int(f[1]), int(f[2])) if len(f) == 3 else (f[0], 0, length_of[f[0]]))
    if not regions:
        raise RuntimeError("No regions! Need to supply either via contig_str or the bamfile")
    if bedfile is None:
        return regions
    bed = read_bed(bedfile)
    by_chrom: Dict[str, List[BedInterval]] = OrderedDict()
    for c, s, e in regions:
        by_chrom.setdefault(_strip_chr(c), []).append(BedInterval(_strip_chr(c), s, e))
    out: List[Region] = []
    for chrom, mine in by_chrom.items():
        for a in mine:
            for b in bed.get(chrom, ()):
                x = intersect_interval(a, b)
                if x is not None:
                    out.append(("chr" + x.chrom if keep_contig_chr else x.chrom, x.start, x.stop))
    return out


def split_subregions(regions: Sequence[Region], size: int) -> List[Region]:
    """Each region cut into pieces of ``size`` from its start (the last may be shorter; a region always yields one)."""
    out: List[Region] = []
    for c, s, e in regions:
        a = s
        while True:
            b = e if a + size > e else a + size
            out.append((c, a, b))
            if b >= e:
                break
            a = b
    return out


def group_subregions(subregions: Sequence[Region], group_size: int) -> List[List[Region]]:
    """Greedy groups whose total length stays within ``group_size`` (groups shape only the reference's temporary files, not
    what is counted or written)."""
    groups: List[List[Region]] = [[]]
    total = 0
    for sub in subregions:
        n = sub[2] - sub[1]
        if n > group_size:
            raise RuntimeError("subregion %s:%d:%d is longer than the group size %d" % (sub[0], sub[1], sub[2], group_size))
        if total + n > group_size:
            groups.append([])
            total = 0
        groups[-1].append(sub)
        total += n
    return groups


# ---- counting rules ---------------------------------------------------------------------------------------------------------
def allele_frequency(count: int, depth: int) -> float:
    return min(count, depth) / depth


def passes(ref: str, alt: str, count: int, depth: int, snp_min_freq: float, indel_min_freq: float) -> bool:
    if depth == 0:
        return False
    snp = len(ref) == 1 and len(alt) == 1
    return allele_frequency(count, depth) > (snp_min_freq if snp else indel_min_freq)


def keep_one_per_position(alleles: Sequence[tuple]) -> List[tuple]:
    """``(chrom, pos, ref, alt, depth, af)`` tuples: per position the first, in sorted order, with the highest AF."""
    best: Dict[Tuple[str, int], tuple] = OrderedDict()
    for a in sorted(alleles):
        k = (a[0], a[1])
        if k not in best or best[k][5] < a[5]:
            best[k] = a
    return list(best.values())


# ---- VCF text -----------------------------------------------------------------------------------------------------------------
def format_af(af: float) -> str:
    return "%g" % float(np.float32(af))


def record_line(chrom: str, pos0: int, ref: str, alt: str, depth: int, af: float) -> str:
    return "%s\t%d\t.\t%s\t%s\t50\t.\tDP=%d;AF=%s\tGT:GQ\t1:50" % (chrom, pos0 + 1, ref, alt, depth, format_af(af))


def header_lines(references: Sequence[str], lengths: Sequence[int]) -> List[str]:
    return list(VCF_HEADER_FIXED) + ["##contig=<ID=%s,length=%d>" % (c, n) for c, n in zip(references, lengths)] + [VCF_COLUMNS]


def sort_lines(lines: Sequence[str]) -> List[str]:
    """``sort -k1,1 -k2,2n`` in the C locale: chrom bytes, POS as a number, then the whole line as the last resort."""
    def key(line: str):
        f = line.split("\t", 2)
        return f[0].encode(), int(f[1]), line.encode()
    return sorted(lines, key=key)


def candidate_tuples(subregions: Sequence[Region], counted: Sequence[tuple], keep_multialleles: bool) -> List[tuple]:
    """Device results ``(region_index, tid, pos0, ref, alt, depth, count)`` -> per subregion ``(chrom, pos0, ref, alt, depth,
    af)`` after the multi-allele rule, subregion by subregion."""
    per: Dict[int, List[tuple]] = {}
    for ri, _tid, pos0, ref, alt, depth, count in counted:
        per.setdefault(ri, []).append((subregions[ri][0], pos0, ref, alt, depth, allele_frequency(count, depth)))
    out: List[tuple] = []
    for ri in range(len(subregions)):
        al = per.get(ri, [])
        out += al if keep_multialleles else keep_one_per_position(al)
    return out


def generate(bam_path: str, output: str, contigs: Optional[str] = None, bedfile: Optional[str] = None,
             keep_contig_chr: bool = False, chunk_size: int = 1000, threads: Optional[int] = None, snp_min_freq: float = 0.01,
             indel_min_freq: float = 0.01, keep_multialleles: bool = False, max_len_indel_allele: int = 60,
             device: int = 0, inflate_device: Optional[str] = None, shard: Optional[Tuple[int, int]] = None,
             reference: Optional[str] = None, subsample=None, read_filter=None, read_stats: bool = False,
             left_align: bool = False) -> dict:
    """Writes ``output`` and returns the run's summary (counts of reads by kind, candidates, times).  ``read_filter=(exclude,
    require, min_mapq)``: reads are dropped by flags and mapping quality in front of every count (``bamio.ReadFilter``); with it or
    with ``read_stats`` the summary carries the read census (``read_*`` entries, ``read_filter.census_of``).  ``subsample=(fraction,
    seed)``: the reads are subsampled by name hash in front of every count (``bamio.SampleRule``; ``subsample_records_seen`` /
    ``subsample_records_kept`` in the summary).  ``inflate_device="gpu"``
    inflates and frames the BAM's records on the device (needs the ``.bai``) and adds the ``inflate_*`` figures to the summary.
    ``reference="ref.fa"`` walks the reads that have no MD tag against the FASTA's bases (``reference_*`` figures in the summary).
    ``left_align=True`` (needs ``reference``): insertions and deletions are moved to their left-most placement on the reference
    bases before they are counted (``left_align_*`` figures in the summary; ``merge_parts`` sums them over shards).
    ``shard=(g, n)``: only the g-th of n contiguous ranges of the groups is counted, and instead of ``output`` the shard's
    unsorted body lines go to ``part_path(output, g)`` with its summary and the header beside them (``merge_parts`` makes
    ``output`` of the n parts)."""
    from .candgen import CandidateCounter, MAX_ALLELE_LEN
    if left_align and reference is None:
        raise ValueError("left_align needs reference: left-alignment is defined by the reference bases")
    if max_len_indel_allele > MAX_ALLELE_LEN:
        raise ValueError("--max_len_indel_allele %d exceeds the allele key's limit of %d bases" % (max_len_indel_allele,
                                                                                                  MAX_ALLELE_LEN))
    with CandidateCounter(bam_path, threads=threads, max_len_indel_allele=max_len_indel_allele, snp_min_freq=snp_min_freq,
                          indel_min_freq=indel_min_freq, device=device, inflate_device=inflate_device, reference=reference,
                          subsample=subsample, read_filter=read_filter, read_stats=read_stats, left_align=left_align) as cc:
        regions = contig_regions(cc.references, cc.lengths, contigs, bedfile, keep_contig_chr)
        logging.info("Examining %d regions in the bamfile", len(regions))
        subregions = split_subregions(regions, chunk_size * 1000)
        groups = group_subregions(subregions, chunk_size * 1000)
        logging.info("Process %d subregions from %d regions in %d groups", len(subregions), len(regions), len(groups))
        tid_of = {c: i for i, c in enumerate(cc.references)}
        missing = sorted({c for c, _, _ in subregions if c not in tid_of})
        if missing:
            raise ValueError("contig(s) %s not in the BAM header" % ", ".join(missing))
        if shard is not None:
            from .shard import shard_range
            a, b = shard_range(len(groups), shard[0], shard[1])
            groups = groups[a:b]
            subregions = [sub for g in groups for sub in g]
            logging.info("Shard %d/%d: %d subregions in %d groups", shard[0], shard[1], len(subregions), len(groups))
        counted, stats = cc.run([(tid_of[c], s, e) for c, s, e in subregions])    # (a shard beyond the last group: no region, zero counts)
        cands = candidate_tuples(subregions, counted, keep_multialleles)
        header = header_lines(cc.references, cc.lengths)
        if shard is None:
            lines = sort_lines([record_line(*c) for c in cands])
            with open(output, "w") as f:
                f.write("\n".join(header + lines) + "\n")
        else:
            lines = [record_line(*c) for c in cands]
    stats.update(regions=len(regions), subregions=len(subregions), groups=len(groups), records=len(lines))
    if shard is not None:
        write_part(output, shard[0], lines, header, stats)
    return stats


# ---- one process per GPU: parts of unsorted body lines, merged by the parent ------------------------------------------------
def write_part(output: str, index: int, lines: Sequence[str], header: Sequence[str], stats: dict) -> None:
    from .shard import part_path
    with open(part_path(output, index), "w") as f:
        f.write("".join(line + "\n" for line in lines))
    with open(part_path(output, index) + ".stats.json", "w") as f:
        json.dump({"header": list(header), "stats": stats}, f)


def merge_parts(output: str, count: int, keep_parts: bool = False) -> dict:
    """``output`` = the header, once, and ``sort_lines`` over the body lines of parts 0..count-1: byte for byte the file one
    process writes, since the sort key is the whole line.  Returns the summed summaries (``regions`` is the job's, not a
    sum; the times are summed over processes that ran side by side) and removes the parts and their side files."""
    from .shard import part_path
    lines: List[str] = []
    total: dict = {}
    header = None
    for g in range(count):
        with open(part_path(output, g)) as f:
            lines += f.read().splitlines()
        with open(part_path(output, g) + ".stats.json") as f:
            side = json.load(f)
        header = side["header"] if header is None else header
        for k, v in side["stats"].items():
            total[k] = v if k == "regions" else total.get(k, 0) + v
    lines = sort_lines(lines)
    with open(output, "w") as f:
        f.write("\n".join(list(header or []) + lines) + "\n")
    if not keep_parts:
        remove_parts(output, count)
    total["records"] = len(lines)
    return total


def remove_parts(output: str, count: int) -> None:
    from .shard import part_path
    for g in range(count):
        for p in (part_path(output, g), part_path(output, g) + ".stats.json"):
            try:
                os.remove(p)
            except OSError:
                pass
