"""Candidate generation from a BAM without MD tags, walked against the reference FASTA on the MI355X (``reference=``).

The yardstick is the MD path, which tests/test_candidates_gpu.py pins to the reference tool's own output: every equality here
is "the FASTA arm on the BAM without MD tags == the MD arm on the same reads carrying the standard MD tag of
tests/candidates_reference_cases.py::md_for": tuples equal, AF equal as a double, VCF body byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from dl4vc_amd import candidates as C
from dl4vc_amd.candgen import CandidateCounter, reference_codes
from tests import candidates_reference_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = dict(threads=4, snp_min_freq=0.075, indel_min_freq=0.02, keep_multialleles=True)


def _body(path):
    return [l for l in open(path).read().split("\n") if l and not l.startswith("#")]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The genome's FASTA with and without its index, the reads, and the BAMs of the two arms."""
    d = tmp_path_factory.mktemp("refcase")
    genome = K.make_genome()
    reads = K.make_reads(genome)
    (d / "fai").mkdir()
    (d / "scan").mkdir()
    return dict(dir=d, genome=genome, reads=reads,
                fasta={True: K.write_fasta(genome, str(d / "fai" / "ref.fa"), True),
                       False: K.write_fasta(genome, str(d / "scan" / "ref.fa"), False)},
                md=K.write_bam(str(d / "md.bam"), reads, K.with_md), bare=K.write_bam(str(d / "bare.bam"), reads, K.without_md))


def _generate(bam, out, **kw):
    stats = C.generate(bam, out, **{**FLAGS, **kw})
    return _body(out), stats


def _kinds(lines):
    snp = ins = dele = 0
    for l in lines:
        f = l.split("\t")
        snp += len(f[3]) == 1 and len(f[4]) == 1
        ins += len(f[4]) > 1
        dele += len(f[3]) > 1
    return snp, ins, dele


# ---- 1. the edge list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [1, 1000])
@pytest.mark.parametrize("fai", [True, False])
def test_fasta_arm_equals_md_arm(case, chunk_size, fai):
    d = case["dir"]
    want, st_md = _generate(case["md"], str(d / "md.vcf"), chunk_size=chunk_size)
    got, st_fa = _generate(case["bare"], str(d / "fa.vcf"), chunk_size=chunk_size, reference=case["fasta"][fai])
    snp, ins, dele = _kinds(want)
    assert snp >= 20 and ins >= 5 and dele >= 5, (snp, ins, dele)
    for line in K.LITERAL_LINES:
        assert line in want, line
    assert got == want
    # the read that runs past the contig's end is malformed in both arms, the depth it adds the same (DP is in the lines)
    assert st_fa["reads_malformed"] == st_md["reads_malformed"] == 1
    assert st_fa["reads"] == st_md["reads"] and st_fa["reads_no_md"] == 0
    assert st_fa["reads_deletions_dropped"] == st_md["reads_deletions_dropped"] > 0
    assert st_fa["reference_reads"] == st_fa["reads"]
    assert st_fa["reference_contigs"] == 3 and st_fa["reference_bases"] == sum(n for _, n, _ in K.CONTIGS)
    assert st_fa["reference_other_bytes"] == 1                       # the '*'


def test_tuples_equal_as_doubles(case):
    subs = C.split_subregions([(n, 0, l) for n, l, _ in K.CONTIGS], 1000)
    names = [c[0] for c in K.CONTIGS]
    regs = [(names.index(c), s, e) for c, s, e in subs]
    kw = dict(threads=4, snp_min_freq=0.075, indel_min_freq=0.02)
    with CandidateCounter(case["md"], **kw) as cc:
        want, _ = cc.run(regs)
    with CandidateCounter(case["bare"], reference=case["fasta"][True], **kw) as cc:
        got, _ = cc.run(regs)
        again, st = cc.run(regs)                                     # the contigs are resident: loaded once
    assert sorted(C.candidate_tuples(subs, got, True)) == sorted(C.candidate_tuples(subs, want, True))
    assert sorted(got) == sorted(want) == sorted(again) and len(want) > 50
    assert st["reference_contigs"] == 3
    # the leading deletion 900..929 of the S D M reads is anchored on their last pair, inside [1000, 2000): the key holds
    # reference bases 100 below the subregion's start
    ref = K.rule_letters(bytes(case["genome"]["ctgA"]))
    lead = [t for t in got if t[1] == 0 and t[2] == 1029 and len(t[3]) == 31]
    assert [(t[3], t[4], t[6]) for t in lead] == [(ref[1029] + ref[900:930], ref[1029], 3)]
    # REF of 60 bases is kept, of 61 dropped
    assert [t for t in got if len(t[3]) == 60] and not [t for t in got if len(t[3]) > 60]


# ---- 2. precedence ------------------------------------------------------------------------------------------------------------
def test_a_read_with_md_is_walked_by_its_md(case):
    reads, d = case["reads"], case["dir"]
    plain = [i for i, r in enumerate(reads) if i % 3 and r["cigar"] == [(0, 100)]]
    wrong = {i: "100" if reads[i]["md"] != "100" else "40A59" for i in plain[:6]}      # disagrees with the FASTA
    wrong[plain[6]] = "12^"                                                            # malformed
    def mixed(i, r):
        return wrong.get(i, r["md"] if i % 3 == 0 else None)
    def filled(i, r):
        return wrong.get(i, r["md"])
    mixed_bam = K.write_bam(str(d / "mixed.bam"), reads, mixed)
    filled_bam = K.write_bam(str(d / "filled.bam"), reads, filled)
    want, st_md = _generate(filled_bam, str(d / "filled.vcf"), chunk_size=1)
    got, st_fa = _generate(mixed_bam, str(d / "mixed.vcf"), chunk_size=1, reference=case["fasta"][True])
    true_md, _ = _generate(case["md"], str(d / "md1.vcf"), chunk_size=1)
    assert got == want and want != true_md                           # (the wrong tags change the output: they were used)
    subs = C.split_subregions([(n, 0, l) for n, l, _ in K.CONTIGS], 1000)
    assert st_fa["reads_malformed"] == st_md["reads_malformed"] == 1 + K.fetched(reads, subs, lambda i, r: i == plain[6])
    subs = C.split_subregions([(n, 0, l) for n, l, _ in K.CONTIGS], 1000)
    assert st_fa["reference_reads"] == K.fetched(reads, subs, lambda i, r: mixed(i, r) is None) > 100
    assert st_fa["reads_no_md"] == 0


# ---- 3. the option off: today's behaviour ---------------------------------------------------------------------------------------
def test_without_reference_reads_without_md_give_no_alleles(case):
    got, st = _generate(case["bare"], str(case["dir"] / "off.vcf"), chunk_size=1)
    assert st["reads_no_md"] == st["reads"] > 100
    assert _kinds(got) == (0, 0, 0)


# ---- 4. records framed on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_size", [1, 1000])
def test_device_framed_records_give_the_same_bytes(case, chunk_size):
    d = case["dir"]
    host, st_h = _generate(case["bare"], str(d / "h.vcf"), chunk_size=chunk_size, reference=case["fasta"][True])
    dev, st_d = _generate(case["bare"], str(d / "d.vcf"), chunk_size=chunk_size, reference=case["fasta"][True], inflate_device="gpu")
    assert open(str(d / "h.vcf"), "rb").read() == open(str(d / "d.vcf"), "rb").read() and len(host) > 50
    assert st_d["inflate_records"] > 0
    for k in ("reads", "reads_malformed", "reads_unsupported", "reads_no_pairs", "reference_reads", "candidates"):
        assert st_d[k] == st_h[k], k


# ---- 5. the conversion: device == host -----------------------------------------------------------------------------------------
def test_device_conversion_equals_host_conversion(case):
    shapes, bad = K.conversion_shapes()
    at = 0
    raw_file = open(case["fasta"][True], "rb").read()
    for line in open(case["fasta"][True] + ".fai"):
        name, n, off, lb, lw = line.split("\t")
        shapes.append((name, raw_file[int(off):], int(lb), int(lw), int(n)))
    for name, raw, lb, lw, n in shapes:
        host, other_h = reference_codes(raw, lb, lw, n)
        dev, other_d = reference_codes(raw, lb, lw, n, device=0)
        assert np.array_equal(host, dev) and other_h == other_d and len(dev) == n, name
        at += n
    assert at > 8000
    errs = []
    for device in (None, 0):
        with pytest.raises(RuntimeError) as e:
            reference_codes(*bad[1:], device=device)
        errs.append(str(e.value))
    assert errs[0] == errs[1] and "base 99" in errs[0] and "do not describe" in errs[0]


def test_wrong_line_width_is_refused_naming_the_contig(case, tmp_path):
    fa = K.write_fasta(case["genome"], str(tmp_path / "ref.fa"), True)
    lines = open(fa + ".fai").read().split("\n")
    f = lines[1].split("\t")
    f[4] = str(int(f[4]) + 1)                                         # ctgB: lines one byte wider than they are
    lines[1] = "\t".join(f)
    open(fa + ".fai", "w").write("\n".join(lines))
    out = str(tmp_path / "o.vcf")
    with pytest.raises(RuntimeError, match=r"contig ctgB.*does not describe the file"):
        C.generate(case["bare"], out, reference=fa, **FLAGS)
    assert not os.path.exists(out)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(case, tmp_path):
    with pytest.raises(RuntimeError, match="cg_set_reference: .*cannot open"):
        CandidateCounter(case["bare"], reference=str(tmp_path / "absent.fa"))
    genome = case["genome"]
    fa = str(tmp_path / "short.fa")
    with open(fa, "wb") as f:                                         # ctgB is missing, ctgC is 10 bases short
        f.write(b">ctgA\n" + K.wrap(bytes(genome["ctgA"]), 60) + b">ctgC\n" + bytes(genome["ctgC"][:690]) + b"\n")
    with CandidateCounter(case["bare"], reference=fa) as cc:
        _, st = cc.run([(0, 0, 5000)])
        assert st["reference_contigs"] == 1 and st["reference_reads"] > 100
        with pytest.raises(RuntimeError, match=r"contig ctgB of the BAM header is not in .*short\.fa"):
            cc.run([(1, 0, 1000)])
        with pytest.raises(RuntimeError, match=r"contig ctgC has 690 bases in .*short\.fa and 700 in the BAM header"):
            cc.run([(2, 0, 700)])
        _, st = cc.run([(0, 0, 5000)])                                # the handle is still good
        assert st["reference_contigs"] == 1


# ---- 7. call_variants.sh -f -d ---------------------------------------------------------------------------------------------------
def test_call_variants_sh_f_d(tmp_path):
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    genome = K.make_genome(special=False)
    reads = K.make_reads(genome, edges=False)
    fa = K.write_fasta(genome, str(tmp_path / "ref.fa"), True)
    md_bam = K.write_bam(str(tmp_path / "md.bam"), reads, K.with_md)
    bare = K.write_bam(str(tmp_path / "bare.bam"), reads, K.without_md)
    want, _ = _generate(md_bam, str(tmp_path / "md.vcf"), chunk_size=1000)
    assert min(_kinds(want)) >= 5
    sd = random_state_dict(DanConfig(), seed=14)
    ck = str(tmp_path / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {}, "state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    out = tmp_path / "out"
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(out), "-i", bare, "-r", fa, "-p", "4", "-f", "-d"],
                       capture_output=True, text=True, timeout=600)
    logs = "".join((out / n).read_text()[-1500:] for n in ("candidate_generator.log", "training.log") if (out / n).exists())
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], logs)
    assert _body(str(out / "candidates.vcf")) == want
    assert '"reference_reads"' in (out / "candidate_generator.log").read_text()
    assert (out / "called_variants.vcf.gz").exists()
