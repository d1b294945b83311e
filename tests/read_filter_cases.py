"""Shared by tests/test_read_filter_host.py and tests/test_read_filter_gpu.py: the oracle of the read filter by flags and mapping
quality.  For a BAM X and a filter (exclude, require, min_mapq), X' = tools/subsample_bam.py X with the filter's flags; every
consumer run on X with the flags must equal the same consumer run on X' without them, byte for byte.  One small BAM with MD tags
in BGZF blocks of 3 000 bytes (so that records straddle block boundaries), its FASTA, and the hand-placed sites the issue names.
Plain module: helpers and fixtures' builders only."""
import os

import numpy as np

from dl4vc_amd import bamio, vcfpost
from dl4vc_amd import pileup_encoder as PE
from tests import pileup_cases as PC
from tests import subsample_cases as SC
from tests.candidates_fixture import md_aux

ROOT = SC.ROOT
FLAGS = (0, 16, 99, 147, 0x100, 0x200, 0x400, 0x800, 0x4)
MAPQS = (0, 1, 19, 20, 21, 59, 60, 255)
FILTERS = [(0, 0, 20), (0x704, 0, 0), (0x900, 0x1, 1)]          # -q 20; -F 0x704; -q 1 -F 0x900 -R 0x1  (exclude, require, min_mapq)
SUBSAMPLE = (0.5, 7)
BLOCK = 3000
ISLAND, DEEP = 2450, 2100                                       # VCF POS on ctgB: MAPQ-0 supplementary reads only; ~1 040 tracks
ISLAND_DROPPED = [(0, 0, 20), (0x900, 0x1, 1)]                  # the filters that drop every read of the island (0x704 spares 0x800)
W, MAX_READS = 16, 60


def flags_of(flt):
    ex, rq, q = flt
    return (["--exclude-flags", "0x%x" % ex] if ex else []) + (["--require-flags", "0x%x" % rq] if rq else []) + \
        (["--min-mapq", str(q)] if q else [])


def predicate(flag, mapq, flt):
    """The three lines the rule is."""
    ex, rq, q = flt
    return (flag & ex) == 0 and (flag & rq) == rq and mapq >= q


def build_case():
    rng = np.random.default_rng(77)
    refs = [("ctgA", PC.make_ref(4000, 301)), ("ctgB", PC.make_ref(3000, 302))]
    reads = []

    def add(tid, pos, cigar, name, flag, mapq, qual=30):
        ref = refs[tid][1]
        if flag & 0x4:
            cigar = "1M"                                        # an unmapped read placed at its mate's position covers one base
        r = PC.read(ref, pos, cigar, name, flag, qual, tid=tid)
        r.mapq = mapq
        reads.append(r)

    k = 0
    for tid, last in ((0, 3880), (1, 1800)):                    # ~25x of 100-base reads with SNP, insertion and deletion reads
        first = len(reads)
        for s in range(20, last, 4):
            cigar = ["100M", "50M1X49M", "40M2I58M", "30M3D67M", "5S95M"][k % 5]
            add(tid, s, cigar, "r%d" % k, int(rng.choice(FLAGS)), int(rng.choice(MAPQS)), 12 + k % 30)
            k += 1
        for r in (reads[first], reads[-1]):                     # the first and the last record of a run: dropped by each filter
            r.flag, r.mapq = 0x400, 0
    # the island: a SNP that exists only through MAPQ-0 supplementary reads (the pileup's own mask 0x704 keeps them)
    for j in range(8):
        add(1, ISLAND - 60 + 3 * j, "%dM1X%dM" % (59 - 3 * j, 40 + 3 * j), "island%d" % j, 0x800, 0)
    # the deep site: 1 060 records, 22 of them duplicates and 22 supplementary.  The encoders' own mask 0x704 drops the duplicates
    # IN FRONT of the GPU encoder's limit of 1 024 tracks (tests/pileup_cases.py::_depth pins that masked reads do not count), so
    # 1 038 tracks are declined with or without -F 0x400, and it is -F 0x800 that brings the site under the limit (1 016 tracks)
    for j in range(1060):
        add(1, DEEP - 50 + j % 7, "100M", "deep%d" % j, 0x400 if j % 50 == 7 else 0x800 if j % 50 == 9 else 0, 60, 20 + j % 20)
    locs = [PC.Loc("ctgA", p, 1) for p in (300, 1171, 2042, 3900)] + [PC.Loc("ctgB", p, 1) for p in (400, 1700, ISLAND, DEEP)]
    return PC.Case("read_filter", refs, reads, locs, w=W, max_reads=MAX_READS)


def write_fixture(tmp):
    """-> {"bam", "bare", "fasta", "case"}: in ``bam`` every read carries NM and MD and the BGZF blocks hold BLOCK inflated
    bytes; ``bare`` holds the same reads without aux tags; the indexes beside them."""
    case = build_case()
    d = os.path.join(str(tmp), case.name)
    os.makedirs(d, exist_ok=True)
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "reads.bam")
    with open(fa, "w") as f:
        for name, seq in case.refs:
            f.write(">%s\n" % name + "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + "\n")
    whole, vcfpost.BGZF_BLOCK = vcfpost.BGZF_BLOCK, BLOCK
    try:
        with bamio.BamWriter(bam, [(n, len(s)) for n, s in case.refs]) as w:
            for r in PC.file_order(case):
                w.write(r.tid, r.pos, r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist(),
                        aux=md_aux(SC.md_of(case.refs[r.tid][1], r)))
    finally:
        vcfpost.BGZF_BLOCK = whole
    bamio.build_bai(bam, bam + ".bai")
    bare = os.path.join(d, "reads_bare.bam")                    # the same reads without aux tags, for the --reference walk
    with bamio.BamWriter(bare, [(n, len(s)) for n, s in case.refs]) as w:
        for r in PC.file_order(case):
            w.write(r.tid, r.pos, r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist())
    bamio.build_bai(bare, bare + ".bai")
    return {"bam": bam, "bare": bare, "fasta": fa, "case": case}


def filtered(bam, flt, subsample=None):
    """X' of ``bam``, written by the tool as a process (once per path) -> its path."""
    out = "%s.f_%x_%x_%d%s.bam" % ((bam[:-4],) + tuple(flt) + ("_s" if subsample else "",))
    if not os.path.isfile(out):
        sub = ["--subsample", subsample[0], "--subsample-seed", subsample[1]] if subsample else []
        r = SC.run_tool("subsample_bam.py", bam, out, *(flags_of(flt) + sub))
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return out


def options(case, flt=None, subsample=None, read_stats=False):
    return PE.EncoderOptions(window_size=case.w, max_reads=case.max_reads, max_insert_length=case.mil,
                             max_insert_length_variant=case.milv, min_base_quality=case.mbq, subsample=subsample, read_filter=flt,
                             read_stats=read_stats)


def parsed(path):
    with bamio.BamFile(path, index="") as b:
        return list(b)


def census_numpy(records_per_region, flt=(0, 0, 0), subsample=None):
    """The census of lists of ``BamRecord``s, one list per region: numpy counts, a record in two regions counting twice."""
    recs = [r for region in records_per_region for r in region]
    flag = np.array([r.flag for r in recs], np.int64)
    mapq = np.array([r.mapq for r in recs], np.int64)
    ex, rq, q = flt
    by_flags = ((flag & ex) != 0) | ((flag & rq) != rq)
    by_mapq = ~by_flags & (mapq < q)
    keep = ~by_flags & ~by_mapq
    if subsample is not None:
        rule = bamio.SampleRule(*subsample)
        keep &= np.array([rule.keeps(r.name.encode()) for r in recs], bool)
    return {"mapq_hist": np.bincount(mapq, minlength=256).tolist(), "flag_bits": [int((flag >> k & 1).sum()) for k in range(16)],
            "seen": len(recs), "dropped_flags": int(by_flags.sum()), "dropped_mapq": int(by_mapq.sum()), "kept": int(keep.sum())}


def window_records(bam, case, locs=None):
    """Per location, the records of its fetch window [pos - (w + 2), pos + w + 3) (clipped at 0): the native encoder's regions."""
    out = []
    with bamio.BamFile(bam) as b:
        for l in (case.locs if locs is None else locs):
            out.append(list(b.fetch(b.get_tid(l.contig), max(l.pos - (case.w + 2), 0), l.pos + case.w + 3)))
    return out


def subregion_records(bam, chunk_kb):
    """Per subregion of candidate generation over the whole BAM, the records overlapping it."""
    from dl4vc_amd.candidates import contig_regions, split_subregions
    out = []
    with bamio.BamFile(bam) as b:
        for c, s, e in split_subregions(contig_regions(b.references, b.lengths), chunk_kb * 1000):
            out.append(list(b.fetch(b.get_tid(c), s, e)))
    return out


def corrupt_bam(tmp):
    """A BAM whose third record is structurally corrupt (its l_seq runs past the record) AND carries the duplicate flag and
    MAPQ 0: a filter would drop it, and it must still be an error.  -> (bam, fasta, location)."""
    ref = PC.make_ref(600, 303)
    d = os.path.join(str(tmp), "read_filter_corrupt")
    os.makedirs(d, exist_ok=True)
    fa, bam = os.path.join(d, "ref.fa"), os.path.join(d, "reads.bam")
    with open(fa, "w") as f:
        f.write(">ref\n" + "\n".join(ref[i:i + 70] for i in range(0, len(ref), 70)) + "\n")
    # the index is that of the same records undamaged: every record lies in the file's one BGZF block, at the same offset
    for path, damage in ((bam + ".clean.bam", False), (bam, True)):
        with bamio.BamWriter(path, [("ref", len(ref))]) as w:
            for i in range(6):
                r = PC.read(ref, 200 + 5 * i, "50M", "c%d" % i, 0x400 if i == 2 else 0, 30)
                body = bytearray(bamio.pack_record(r.tid, r.pos, r.name, r.flag, 0 if i == 2 else 60, list(r.cigar), r.seq,
                                                   r.qual.tolist())[4:])
                if i == 2 and damage:
                    body[16:20] = (5000).to_bytes(4, "little")  # l_seq
                w.write_raw(bytes(body))
    bamio.build_bai(bam + ".clean.bam", bam + ".bai")
    return bam, fa, PC.Loc("ref", 230, 1)
