"""Candidate generation on the MI355X: every fixture of tools/gen_golden_candidates.py (the reference's own functions on a
pysam stand-in) written to a BAM + BAI and run through libdl4vc_cand.so; the tuples equal the reference's exactly (integers
equal, AF equal as a double) and the VCF body equals the fixture's lines.  Then call_variants.sh from a BAM alone."""
import os
import subprocess

import numpy as np
import pytest

from dl4vc_amd import candidates as C
from tests.candidates_fixture import NAMES, load, write_bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _body(path):
    return [l.rstrip("\n") for l in open(path) if not l.startswith("#")]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_generator_matches_reference(name, tmp_path):
    fx = load(name)
    bam = write_bam(fx, str(tmp_path / (name + ".bam")))
    for run in fx["runs"]:
        p = run["params"]
        bed = None
        if run["bed"] is not None:
            bed = str(tmp_path / "r.bed")
            open(bed, "w").write(run["bed"])
        out = str(tmp_path / ("%s.vcf" % run["name"]))
        try:
            stats = C.generate(bam, out, contigs=p["contigs"], bedfile=bed, keep_contig_chr=p["keep_contig_chr"],
                               chunk_size=p["chunk_size"], threads=4, snp_min_freq=p["snp_min_freq"],
                               indel_min_freq=p["indel_min_freq"], keep_multialleles=p["keep_multialleles"],
                               max_len_indel_allele=p["max_len_indel_allele"])
        except ValueError as e:                    # contigs the BAM does not have: the reference's fetch raises too
            assert run["bed"] is not None and not p["keep_contig_chr"], e
            continue
        assert _body(out) == run["lines"], run["name"]
        assert stats["reads_malformed"] == run["malformed_fetched"], (run["name"], stats)


@pytest.mark.gpu
def test_tuples_exact(tmp_path):
    """The counter's raw output, subregion by subregion, against the reference's tuples: depth, count-derived AF as a double."""
    from dl4vc_amd.candgen import CandidateCounter
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    run = [r for r in fx["runs"] if r["name"] == "chunk5"][0]
    p = run["params"]
    subs = [tuple(s) for s in run["subregions"]]
    refs = [r[0] for r in fx["references"]]
    with CandidateCounter(bam, threads=4, max_len_indel_allele=p["max_len_indel_allele"], snp_min_freq=p["snp_min_freq"],
                          indel_min_freq=p["indel_min_freq"]) as cc:
        counted, stats = cc.run([(refs.index(c), s, e) for c, s, e in subs])
    got = sorted(C.candidate_tuples(subs, counted, True))
    want = sorted(tuple(t) for t in run["tuples"])
    assert got == want
    assert stats["reads"] > 3000 and stats["candidates"] == len(want)


@pytest.mark.gpu
def test_call_variants_sh_from_bam_alone(tmp_path):
    """call_variants.sh -i BAM -r REF -m CKPT -o EMPTY_OUT: candidates.vcf is made (= the fixture's lines for the reference's
    call_variants flags) and the run finishes with called_variants.vcf.gz."""
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    rng = np.random.default_rng(3)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, length in fx["references"]:
            s = "".join(rng.choice(list("ACGT"), length))
            f.write(">%s\n%s\n" % (name, "\n".join(s[i:i + 60] for i in range(0, length, 60))))
    sd = random_state_dict(DanConfig(), seed=14)
    ck = str(tmp_path / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {}, "state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    out = tmp_path / "out"
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(out), "-i", bam, "-r", fa, "-p", "4"],
                       capture_output=True, text=True, timeout=600)
    log = (out / "candidate_generator.log").read_text() if (out / "candidate_generator.log").exists() else ""
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], log[-1500:])
    cli = [run for run in fx["runs"] if run["name"] == "cli"][0]
    assert cli["params"]["keep_multialleles"] and cli["params"]["chunk_size"] == 1000
    assert _body(str(out / "candidates.vcf")) == cli["lines"]
    assert (out / "called_variants.vcf.gz").exists()
