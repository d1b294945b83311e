"""Training data from a BAM and a truth VCF on the MI355X (tools/make_training_data.sh): candidate generation (allele counts
on the GPU) -> tools/vcf_isec.py against the truth -> the converter -> train.hdf, then one training step of main.py on it.

The BAM carries planted variants on two haplotypes: SNPs (one homozygous), a deletion, an insertion, a site with a different
ALT on each haplotype (a 1/2 truth record A>X,Y: its two candidates A>X and A>Y pair with nothing), and a SNP the truth does
not hold.  The truth also holds two SNPs no read supports."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import hdf5io
from dl4vc_amd.bamio import BamWriter, build_bai

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, I, D = 0, 1, 2
LENGTH = 3000


def _alt_base(b):
    return [c for c in "ACGT" if c != b][0]


def planted(ref):
    """{hap: {pos0: (kind, data)}} and the truth records (pos1, REF, ALT, GT, supported)."""
    x, y = [c for c in "ACGT" if c != ref[1700]][:2]
    haps = {0: {}, 1: {}}
    truth = []
    for p, hs, gt in ((500, (0,), "0/1"), (800, (0, 1), "1/1"), (2000, (1,), None)):
        for h in hs:
            haps[h][p] = ("snp", _alt_base(ref[p]))
        if gt:
            truth.append((p + 1, ref[p], _alt_base(ref[p]), gt))
    haps[1][1100] = ("del", 2)
    truth.append((1101, ref[1100:1103], ref[1100], "0/1"))
    haps[0][1400] = ("ins", "TT")
    truth.append((1401, ref[1400], ref[1400] + "TT", "0/1"))
    haps[0][1700] = ("snp", x)
    haps[1][1700] = ("snp", y)
    truth.append((1701, ref[1700], "%s,%s" % (x, y), "1/2"))
    for p, gt in ((2300, "0/1"), (2600, "1/1")):                     # no read supports these
        truth.append((p + 1, ref[p], _alt_base(ref[p]), gt))
    return haps, sorted(truth)


def make_read(ref, start, var, length=100):
    """(cigar, seq, md) of a read from ``start`` on the haplotype ``var``."""
    ops, seq, md = [], [], []
    match, r = 0, start

    def add(op, n):
        if ops and ops[-1][0] == op:
            ops[-1][1] += n
        else:
            ops.append([op, n])

    while len(seq) < length or ops[-1][0] != M:
        v = var.get(r)
        if v is None or v[0] == "snp":
            if v is None:
                seq.append(ref[r])
                match += 1
            else:
                seq.append(v[1])
                md.append("%d%s" % (match, ref[r]))
                match = 0
            add(M, 1)
            r += 1
            continue
        seq.append(ref[r])                                  # the anchor base
        add(M, 1)
        match += 1
        r += 1
        if v[0] == "ins":
            seq.extend(v[1])
            add(I, len(v[1]))
        else:
            add(D, v[1])
            md.append("%d^%s" % (match, ref[r:r + v[1]]))
            match = 0
            r += v[1]
    md.append(str(match))
    return [tuple(o) for o in ops], "".join(seq), "".join(md)


def write_inputs(d):
    rng = np.random.default_rng(21)
    ref = "".join(rng.choice(list("ACGT"), LENGTH))
    fa = str(d / "ref.fa")
    with open(fa, "w") as f:
        f.write(">chr20\n%s\n" % "\n".join(ref[i:i + 60] for i in range(0, LENGTH, 60)))
    haps, truth = planted(ref)
    bam = str(d / "reads.bam")
    with BamWriter(bam, [("chr20", LENGTH)]) as w:
        for i, start in enumerate(range(0, LENGTH - 130, 5)):
            cigar, seq, md = make_read(ref, start, haps[i % 2])
            w.write(0, start, "r%d" % i, 16 if (i // 2) % 2 else 0, 60, cigar, seq, qual=[30] * len(seq),
                    aux=b"MDZ" + md.encode() + b"\x00")
    build_bai(bam, bam + ".bai")
    tv = str(d / "truth.vcf")
    with open(tv, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr20,length=%d>\n" % LENGTH)
        f.write("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tHG\n")
        for pos, r, a, gt in truth:
            f.write("chr20\t%d\t.\t%s\t%s\t50\tPASS\t.\tGT\t%s\n" % (pos, r, a, gt))
    return bam, fa, tv, ref, truth


def _body(path):
    return [l.rstrip("\n") for l in open(path) if not l.startswith("#")]


def test_make_training_data_labels_and_trains(tmp_path):
    bam, fa, tv, ref, truth = write_inputs(tmp_path)
    out = tmp_path / "out"
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "make_training_data.sh"), "-i", bam, "-r", fa, "-t", tv,
                        "-o", str(out), "-p", "4"], capture_output=True, text=True, timeout=600)
    logs = {n: (out / n).read_text()[-1500:] for n in ("candidate_generator.log", "isec.log", "training_data.log")
            if (out / n).exists()}
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], logs)

    cands = _body(str(out / "candidates.vcf"))
    by_pos = {}
    for l in cands:
        f = l.split("\t")
        by_pos.setdefault(int(f[1]), []).append((f[3], f[4]))
    # every planted allele is a candidate, and nothing else
    assert sorted(by_pos) == [501, 801, 1101, 1401, 1701, 2001], cands
    tp = [l.split("\t") for l in _body(str(out / "isec" / "0003.vcf"))]
    fp = [l.split("\t") for l in _body(str(out / "isec" / "0001.vcf"))]
    fn = [l.split("\t") for l in _body(str(out / "isec" / "0000.vcf"))]
    shared_truth = [l.split("\t") for l in _body(str(out / "isec" / "0002.vcf"))]
    assert [int(f[1]) for f in tp] == [501, 801, 1101, 1401]
    assert sorted(int(f[1]) for f in fp) == [1701, 1701, 2001]           # the 1/2 site's two alleles pair with nothing
    assert [int(f[1]) for f in fn] == [1701, 2301, 2601]
    assert [f[:5] for f in shared_truth] == [["chr20", str(p), ".", r_, a] for p, r_, a, _ in truth if p in (501, 801, 1101, 1401)]

    with hdf5io.CandidateFile(str(out / "train.hdf")) as h:
        n = len(h)
        labels = h.read_field(0, n, "label").ravel()
        recs = [v.decode().rstrip("\x00") for v in h.read_field(0, n, "vcfrec").ravel()]
    assert n == len(tp) + len(fp)
    gts = {p: gt for p, _, _, gt in truth}
    seen = set()
    for lab, text in zip(labels, recs):
        f = text.split("\t")
        pos, key = int(f[1]), (f[1], f[3], f[4])
        seen.add(key)
        if lab == 0:
            assert pos in (501, 801, 1101, 1401), text
            assert f[-1] == "GT:%s" % gts[pos], text                        # the truth's genotype text
        else:
            assert lab == 2 and pos in (1701, 2001), text
            assert not f[-1].startswith("GT:"), text
    assert seen == {(f[1], f[3], f[4]) for f in tp + fp}

    # one training step on it, evaluated on the same file
    from test_cli_gpu import MODEL_FLAGS, TRAIN_FLAGS
    sample = str(tmp_path / "candidates.vcf")
    open(sample, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n")
    hdf = str(out / "train.hdf")
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--train_file", hdf, "--test_file", hdf, "--max-train-batches", "1",
           "--modelsave", str(tmp_path / "model.pth.tar"), "--sample_vcf", sample, "--save_vcf_records",
           "--save_vcf_records_file", str(tmp_path / "model_test.vcf")] + MODEL_FLAGS + TRAIN_FLAGS
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Test set: Average loss:" in r.stdout
