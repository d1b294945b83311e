"""Shared by tests/test_subsample_host.py and tests/test_subsample_gpu.py: the oracle of read subsampling by name hash.  For a
BAM X, fraction F and seed S, X' = tools/subsample_bam.py X --subsample F --subsample-seed S; every consumer run on X with the
option must equal the same consumer run on X' without it, byte for byte.  Plain module: helpers and fixtures' builders only."""
import os
import subprocess
import sys

import numpy as np

from dl4vc_amd import bamio
from dl4vc_amd import pileup_encoder as PE
from tests import pileup_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
FRACTION = 0.5
SEEDS = (0, 7)
WORKED = [          # name, seed, X31, wang(X31 ^ seed), & 0xffffff (the issue's table)
    (b"r1", 0, 0x00000dff, 0xf0f8c8cd, 16304333),
    (b"read/1", 0, 0xc84551f8, 0xec530e6b, 5443179),
    (b"read/1", 42, 0xc84551f8, 0x1f4e6d53, 5139795),
    (b"HWI-ST1234:7:1101:1234:5678", 0, 0x52e1ffc8, 0x0d408e20, 4230688),
    (b"HWI-ST1234:7:1101:1234:5678", 11, 0x52e1ffc8, 0x4572214f, 7479631),
]
THRESHOLDS = [(0.3, 5033165), (0.5, 8388608), (0.6, 10066330), (1e-9, 1), (1.0, 16777216)]


def run_tool(name, *argv, **kw):
    return subprocess.run([sys.executable, os.path.join(TOOLS, name)] + [str(a) for a in argv], capture_output=True, text=True,
                          timeout=600, **kw)


def subsampled(bam, fraction, seed, out=None):
    """X' of ``bam``, written by the tool as a process (once per path) -> its path."""
    out = out or "%s.sub_%g_%d.bam" % (bam[:-4], fraction, seed)
    if not os.path.isfile(out):
        r = run_tool("subsample_bam.py", bam, out, "--subsample", fraction, "--subsample-seed", seed)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return out


def raw_records(path):
    with bamio.BamFile(path, index="") as b:
        return list(b.raw_records())


def kept_share(path, fraction, seed):
    rule = bamio.SampleRule(fraction, seed)
    recs = raw_records(path)
    return sum(rule.keeps_record(r) for r in recs) / max(1, len(recs))


def options(case, subsample=None):
    return PE.EncoderOptions(window_size=case.w, max_reads=case.max_reads, max_insert_length=case.mil,
                             max_insert_length_variant=case.milv, min_base_quality=case.mbq, subsample=subsample)


def location(l):
    return PE.Location(l.contig, l.pos, "%s:%d" % (l.contig, l.pos), 2, "%s\t%d\t.\tA\tC" % (l.contig, l.pos))


def python_result(bam, fa, loc, opt):
    """The Python builder on one location: ("raises", exception type name) or (record bytes, errors)."""
    try:
        recs, errors = PE.encode_locations(bam, fa, [loc], opt, native=False)
    except (KeyError, ValueError) as e:
        return ("raises", type(e).__name__)
    return (recs.tobytes(), errors)


def same_planes(a, b, what):
    """Two six-tuples of an encoder (reads, qual, strand, ref, num_reads, status) are equal, status first."""
    assert np.array_equal(a[5], b[5]), (what, "status", a[5].tolist(), b[5].tolist())
    assert np.array_equal(a[4], b[4]), (what, "num_reads")
    for k, name in enumerate(("reads", "qual", "strand", "ref")):
        assert np.array_equal(a[k], b[k]), (what, name)


ONE_CHAR = "abcdefgh"
LONG = [c * 253 + d for c, d in zip("LMKQ", "0123")] + [c * 254 for c in "RSTV"]      # 254 characters: l_read_name 255


def named_case():
    """Reads whose names have 1 and 254 characters (l_read_name 2 and 255) among ordinary ones over three locations.  Each such
    name is on two records at different positions (a pair of mates): one answer for both."""
    ref = PC.make_ref(1200, 131)
    reads = []
    for i in range(80):
        cigar = ["50M", "20M2I28M", "25M3D25M", "2S48M"][i % 4]
        reads.append(PC.read(ref, 260 + i, cigar, "n%d/%d" % (i, i % 3), PC.FREV if i % 2 else 0, 12 + i % 30))
    for k, name in enumerate(list(ONE_CHAR) + LONG):
        reads.append(PC.read(ref, 270 + 3 * k, "50M", name, 0, 33))
        reads.append(PC.read(ref, 290 + 3 * k, "40M1X9M", name, PC.FREV, 34))
    locs = [PC.Loc("ref", p, 1) for p in (300, 320, 341)]
    return PC.Case("subsample_names", [("ref", ref)], reads, locs, w=16, max_reads=150)


def block_case():
    """The reads of the device-inflate arms: ~3 200 reads of 100 bases, mismatches, insertions and deletions among them, enough
    for the BAM to span several BGZF blocks with records straddling their boundaries (``block_layout`` says how many)."""
    ref = PC.make_ref(30000, 141)
    reads = []
    for i, s in enumerate(range(100, 29000, 9)):
        cigar = ["100M", "50M1X49M", "40M2I58M", "30M3D67M", "5S95M"][i % 5]
        reads.append(PC.read(ref, s, cigar, "blk%d:%d" % (i // 2, i % 7), PC.FREV if i % 2 else 0, 10 + i % 30))
    locs = [PC.Loc("ref", p, 1) for p in range(400, 28000, 1717)]
    return PC.Case("subsample_blocks", [("ref", ref)], reads, locs, w=16, max_reads=60)


def md_of(ref, r):
    """The MD value of a ``pileup_cases.read`` against ``ref`` (M and = match, X differs, D deletes)."""
    out, run, p = [], 0, r.pos
    for op, l in r.cigar:
        if op in (0, 7):
            run += l
        elif op == 8:
            for j in range(l):
                out.append("%d%s" % (run, ref[p + j]))
                run = 0
        elif op == 2:
            out.append("%d^%s" % (run, ref[p:p + l]))
            run = 0
        if op in (0, 2, 3, 7, 8):
            p += l
    return "".join(out) + str(run)


def write_block_bams(tmp):
    """``block_case`` as two BAMs with their indexes -- ``md`` (every read carries NM and MD) and ``bare`` (no aux) -- and the FASTA."""
    from tests.candidates_fixture import md_aux
    case = block_case()
    bare, fa = PC.write_case(tmp, case)
    ref = case.refs[0][1]
    md = os.path.join(os.path.dirname(bare), "reads_md.bam")
    with bamio.BamWriter(md, [(n, len(s)) for n, s in case.refs]) as w:
        for r in PC.file_order(case):
            w.write(r.tid, r.pos, r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist(), aux=md_aux(md_of(ref, r)))
    bamio.build_bai(md, md + ".bai")
    return {"md": md, "bare": bare, "fasta": fa, "case": case}


def block_layout(path):
    """(number of BGZF blocks holding records, records that straddle a block boundary), read from the virtual offsets."""
    blocks, straddle = set(), 0
    with bamio.BamFile(path, index="") as b:
        b.r.seek(b.first_record)
        while True:
            at = b.r.tell()
            if b._next() is None:
                break
            end = b.r.tell()
            blocks.add(at >> 16)
            if (at >> 16) != (end >> 16) and (end & 0xffff) > 0:
                straddle += 1
    return len(blocks), straddle
