"""Fixtures of the ``--train_bam`` tests (tests/test_train_bam_host.py on the CPU, tests/test_train_bam_gpu.py on the GPU): records
laid out both ways -- as three plane arrays ``[n][S][W]`` (the pileup encoder's output) and as packed records with the planes at
odd offsets (an inflated chunk) -- and a labelled BAM fixture with its tp / fp / full VCFs."""
import os

import numpy as np

from tests import pileup_cases as PC
from tests.test_score_bam import vcf_line

SHAPES = [(5, 7), (3, 16), (200, 201)]           # (S, W): 35-byte slots (every alignment), 48-byte slots, the production planes
N_SLOTS = 14
# slots in the order they are appended: out of order, with gaps (4, 6, 8, 10 and 12 are never taken)
TAKEN = np.array([9, 2, 0, 13, 5, 1, 3, 11, 7], np.int32)


def span(kept, W):
    return (3 * np.asarray(kept, np.int64) * W + 15) & ~np.int64(15)


def planes_and_kept(S, W, seed=0):
    """Three arrays ``[N_SLOTS][S][W]`` and every slot's extent.  Slot 0: all zero (kept 0).  Slot 1: the only non-zero byte is the
    last byte of the strand plane (kept S).  Slot 2: the last non-zero byte is the first byte of a row.  Slot 3: the last byte of a
    row.  The others: 0..S rows of random bytes (zeros among them), the last row non-zero in one plane only."""
    rng = np.random.default_rng(1000 * S + W + seed)
    planes = [np.zeros((N_SLOTS, S, W), np.uint8) for _ in range(3)]
    kept = np.zeros(N_SLOTS, np.int32)
    planes[2][1, S - 1, W - 1] = 7
    kept[1] = S
    for slot in range(2, N_SLOTS):
        k = int(rng.integers(1, S + 1)) if slot not in (2, 3) else max(1, S // 2)
        if slot in (5, 9, 13):
            k = S                                            # (large records: the small slabs fill up)
        for p in planes:
            if k > 1:
                p[slot, :k - 1] = rng.integers(0, 5, (k - 1, W)) * rng.integers(1, 60, (k - 1, W))
        col = 0 if slot == 2 else W - 1 if slot == 3 else int(rng.integers(0, W))
        planes[slot % 3][slot, k - 1, col] = 1 + slot
        kept[slot] = k
    return planes, kept


def as_records(planes):
    """The same slots as packed records: 7 bytes | reads | 5 bytes | qual | strand | 3 or 4 bytes, the filler 0xEE (never zero)
    -> (the bytes, record_bytes, plane offsets).  record_bytes is odd, so the planes start at every alignment."""
    n, S, W = planes[0].shape
    sw = S * W
    off = [7, 7 + sw + 5, 7 + 2 * sw + 5]
    rb = off[2] + sw + 3 + sw % 2
    buf = np.full((n, rb), 0xEE, np.uint8)
    for o, p in zip(off, planes):
        buf[:, o:o + sw] = p.reshape(n, sw)
    return buf.reshape(-1), rb, off


# ---- the labelled BAM --------------------------------------------------------------------------------------------------------
# Records the fixture gives (locations minus those without a read), stated here and asserted by the tests that fill from it.
TRAIN_RECORDS = 40          # of 43 locations: 60, 3800 and 8000 hold no read
TEST_RECORDS = 23           # of 26 locations: 120, 5522 (behind the twin pair) or 8500 hold none -- see the test
CONVERTER_FLAGS = ["--max-reads", "200", "--num-processes", "2", "--max-insert-length", "10", "--max-insert-length-variant", "50",
                   "--save-q-scores", "--save-strand"]


def labelled_fixture(d, contigs=1):
    """The BAM of ``tests/test_score_bam_gpu.py::_fixture`` (24x background, a 170-deep and a 260-deep site, holes, the ``twin`` pair
    only the Python builder takes, a site with 1 100 tracks) with LABELLED locations: training tp / fp VCFs and a full VCF that
    carries GT for the tp sites, and the same for evaluation over other positions.  One training tp record's text is longer than the
    128 stored bytes.  ``contigs=2``: a second contig ``chr21`` with the same reads, and locations on both, for the held-out runs.
    -> dict of paths."""
    ref = PC.make_ref(9000, 77)
    def reads_on(tid):
        reads = []
        for i, s in enumerate(range(200, 5000, 4)):
            if 3600 <= s < 3800:
                continue
            cigar = ["100M", "50M1X49M", "40M2I58M", "30M3D67M", "5S95M"][i % 5]
            reads.append(PC.read(ref, s, cigar, "bg%d" % i, PC.FREV if i % 2 else 0, 10 + i % 30, tid=tid))
        reads += [PC.read(ref, 1950 + i % 45, "100M" if i % 3 else "47M1X52M", "deep%d" % i, PC.FREV if i % 2 else 0, 20 + i % 20, tid=tid)
                  for i in range(150)]
        reads += [PC.read(ref, 2930 + i % 60, "90M", "deeper%d" % i, PC.FREV if i % 3 else 0, 25, tid=tid) for i in range(240)]
        reads += [PC.read(ref, 5500, "40M", "solo", 0, 30, tid=tid), PC.read(ref, 5505, "30M", "twin", 0, 32, seq=ref[5505:5535], tid=tid),
                  PC.read(ref, 5509, "30M", "twin", PC.FREV, 32, seq=ref[5505:5535], tid=tid)]
        reads += [PC.read(ref, 6200 + i % 25, "30M", "many%d" % i, PC.FREV if i % 2 else 0, 30, tid=tid) for i in range(1100)]
        return reads

    names = [("chr20", ref)] + ([("chr21", ref)] if contigs == 2 else [])
    reads = [r for tid in range(len(names)) for r in reads_on(tid)]
    case = PC.Case("train_bam", names, reads, [], w=100, max_reads=200)
    bam, fa = PC.write_case(d, case)
    grid = list(range(330, 4900, 83))                         # 56 positions; 3652 and 3735 lie in the hole but reads reach them
    train_tp = [60] + grid[0:36:2] + [2000, 3800, 5520]       # no read at 60 and 3800; 170 deep; the twin pair
    train_fp = grid[1:36:2] + [2990, 6215, 8000]              # 260 deep; 1 100 tracks; no read at 8000
    test_tp = [120] + grid[36::2] + [2002, 5522]
    test_fp = grid[37::2] + [2992, 6217, 8500]
    head = "##fileformat=VCFv4.2\n##contig=<ID=chr20,length=9000>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n"
    out = {"bam": bam, "fasta": fa, "dir": str(d), "ref": ref}

    def line(p, i, pad, chrom):
        return vcf_line(ref, p, i % 3, pad).replace("chr20", chrom, 1)

    chroms = [c for c, _ in names]
    for name, pos, pad_at in (("train_tp", train_tp, 4), ("train_fp", train_fp, -1), ("test_tp", test_tp, -1), ("test_fp", test_fp, 2)):
        path = os.path.join(str(d), name + ".vcf")
        with open(path, "w") as f:
            f.write(head + "".join(line(p, i, 150 if i == pad_at else 0, c) + "\n" for c in chroms for i, p in enumerate(pos)))
        out[name] = path
    # the full VCFs: the tp sites with a genotype column format_vcf-style (GT in FORMAT, the call in the sample column)
    for name, pos in (("train_full", train_tp), ("test_full", test_tp)):
        path = os.path.join(str(d), name + ".vcf")
        with open(path, "w") as f:
            f.write(head + "".join(line(p, i, 0, c).rsplit("\t", 1)[0] + "\t%s\n" % ("1/1" if i % 2 else "0/1")
                                   for c in chroms for i, p in enumerate(pos)))
        out[name] = path
    # evaluation as inference has it: one VCF of all evaluation locations (label 2)
    path = os.path.join(str(d), "sample.vcf")
    with open(path, "w") as f:
        f.write(head + "".join(open(out[k]).read().split("CALLED\n", 1)[1] for k in ("test_tp", "test_fp")))
    out["sample"] = path
    out["counts"] = {"train": (len(train_tp) + len(train_fp)) * len(chroms), "test": (len(test_tp) + len(test_fp)) * len(chroms)}
    return out


def locations(fx, which):
    """The locations of ``which`` ("train" / "test") in the converter's order: tp with the full VCF's genotypes, then fp."""
    from dl4vc_amd.pileup_encoder import locations_from_vcf
    return locations_from_vcf(fx[which + "_tp"], 0, fx[which + "_full"]) + locations_from_vcf(fx[which + "_fp"], 2)


def convert(fx, which, out, extra=()):
    """``tools/convert_bam_single_reads.py`` on the fixture's ``which`` VCFs -> ``out``."""
    import subprocess
    import sys
    from conftest import ROOT
    cmd = [sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", fx["bam"], "--tp_vcf", fx[which + "_tp"],
           "--tp_full_vcf", fx[which + "_full"], "--fp_vcf", fx[which + "_fp"], "--fasta-input", fx["fasta"], "--output", out] + \
        CONVERTER_FLAGS + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    return out
