"""Fuzzing against the reference's own outputs on random cases.  The cases come from fixed seeds (oracle/fuzz_cases.py);
oracle/gen_golden_fuzz.py ran the reference on them and stored what it returned in tests/golden/fuzz_reference.{npz,json.gz}.
Each test regenerates its cases, checks that they are the ones the fixture was written for, and holds the project's code to the
stored outputs: random structural configurations through the oracle, random allele records through the mask builders, random
scored VCFs through format_vcf and through the acceptance comparison."""
import gzip
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from golden_util import check_against_bf16_fixture


@pytest.fixture(scope="module")
def ref_arrays():
    z = np.load(os.path.join(GOLDEN, "fuzz_reference.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def ref_texts():
    with gzip.open(os.path.join(GOLDEN, "fuzz_reference.json.gz"), "rt") as f:
        return json.load(f)


def stored_outputs(arrays, tag, sd, batch):
    """The reference's outputs of case `tag`, after checking that the regenerated case is the one they were computed from."""
    from oracle.fuzz_cases import digest
    assert bytes(arrays[tag + ":digest"]).decode() == digest(sd, batch), "%s: the seeded case differs from the fixture's" % tag
    return {k[len(tag) + 5:]: v for k, v in arrays.items() if k.startswith(tag + ":out:")}


def test_random_structural_configs_oracle_equals_reference(ref_arrays):
    from oracle.dan_oracle import dan_forward_oracle
    from oracle.fuzz_cases import structural_cases
    cases = structural_cases()
    assert len(cases) == len({k.split(":")[1] for k in ref_arrays if k.startswith("struct:")})
    for trial, spec, sd, batch in cases:
        want = stored_outputs(ref_arrays, "struct:%d" % trial, sd, batch)
        assert want
        got = dan_forward_oracle(sd, spec, *batch.arrays())
        for k, v in want.items():
            np.testing.assert_allclose(got[k], v, atol=2e-5 * max(1.0, float(np.abs(v).max())), err_msg="%s %s" % (spec, k))


def test_bf16_operand_mode_of_the_oracle_equals_the_reference_run_with_bf16_rounded_gemm_operands(ref_arrays):
    """BASELINE config 5 computes in bf16.  The reference has no such mode; what it means is pinned here: the reference's OWN
    forward with the weights of every conv / residual 1x1 / bottleneck module rounded to bf16 and the inputs of those modules
    rounded to bf16 by forward-pre-hooks (fp32 sums, everything else untouched) equals the oracle's bf16 = "operands" mode --
    on random structures and on the production structure at 301 columns.  The "storage" mode (the HIP kernel's bf16 activation
    storage on top) stays within the bf16 bound of it.  Every output and tap is compared, the larger conv taps at a fixed
    sample of 4096 positions (oracle/fuzz_cases.py::tap_sample).  On the machine class the fixture was written on the bar is fp32 roundoff;
    elsewhere the flip-consistent bar of golden_util.check_against_bf16_fixture (a host with another vector ISA sums in
    another order, and a last-bit difference can flip a bf16 rounding)."""
    from oracle.dan_oracle import dan_forward_oracle
    from oracle.fuzz_cases import bf16_operand_cases, tap_sample
    cases = bf16_operand_cases()
    assert len(cases) == len({k.split(":")[1] for k in ref_arrays if k.startswith("bf16:")})
    for i, spec, sd, batch in cases:
        want = stored_outputs(ref_arrays, "bf16:%d" % i, sd, batch)
        assert want
        got = dan_forward_oracle(sd, spec, *batch.arrays(), taps=True, bf16="operands")
        plain = dan_forward_oracle(sd, spec, *batch.arrays(), taps=True)
        stor = dan_forward_oracle(sd, spec, *batch.arrays(), taps=True, bf16="storage")
        moved = 0.0
        for k, v in want.items():
            sc = max(1.0, float(np.abs(v).max()))
            # (the larger conv taps: at the fixture's fixed sample of positions)
            g, pl, st = tap_sample(k, got[k]), tap_sample(k, plain[k]), tap_sample(k, stor[k])
            # the same arithmetic on the same torch kernels: the fp32-vs-fp32 bar (observed: conv taps bit-identical)
            check_against_bf16_fixture(g, v, "%s:%s" % (spec, k), 2e-5)
            moved = max(moved, float(np.abs(pl - v).max()) / sc)
            assert float(np.abs(st - v).max()) <= 4e-2 * sc, (spec, k)
        assert moved > 1e-4, "the hooks rounded nothing: %g" % moved      # the mode IS different from fp32


def test_random_alleles_equal_reference(ref_texts):
    from dl4vc_amd import alleles
    from oracle.fuzz_cases import allele_cases
    cases, stored = allele_cases(), ref_texts["alleles"]
    assert len(cases) == len(stored) == 300
    n_ok = n_err = 0
    for (rec, window), want in zip(cases, stored):
        assert rec == want["rec"] and "".join(str(int(t)) for t in window) == want["window"], "the seeded case differs from the fixture's"
        if "masks" in want:
            got = alleles.allele_mask_vectors(rec, window)
            assert got[0].tolist() == want["masks"][0] and got[1].tolist() == want["masks"][1], rec
            n_ok += 1
        else:
            with pytest.raises(Exception) as ex:
                alleles.allele_mask_vectors(rec, window)
            assert isinstance(ex.value, AssertionError) == (want["error"] == "AssertionError"), (rec, want["error"], ex.value)
            n_err += 1
    assert n_ok > 100 and n_err > 10


def test_random_scored_vcfs_through_format_vcf_equal_reference(ref_texts):
    from dl4vc_amd import vcf
    from oracle.fuzz_cases import scored_vcf_cases
    texts, stored = scored_vcf_cases(), ref_texts["format_vcf"]
    assert len(texts) == len(stored) == 25
    for trial, (text, want) in enumerate(zip(texts, stored)):
        assert text == want["scored"], "trial %d: the seeded case differs from the fixture's" % trial
        got = "".join(vcf.format_vcf_lines(text.splitlines(keepends=True), vcf.FormatOptions(**vcf.PIPELINE_OPTIONS)))
        assert got == want["formatted"], "trial %d" % trial


def test_acceptance_tool_derives_the_genotype_lines_the_reference_program_writes(ref_texts):
    """tools/compare_calls.py judges the real-data run.  Its genotype lines must be what the reference's
    OWN tools/format_vcf.py writes from the same scored file: random pairs of scored VCFs (the second = the first with score noise of
    a few 1e-5, some sites pushed across a threshold) went through the reference program (sorted, as the pipeline does:
    call_variants.sh:151), the two outputs are diffed record by record, and dl4vc_amd.compare must report exactly that set of
    differing records -- split into knife-edge and elsewhere by ITS attribution, which is then checked against the scores."""
    from dl4vc_amd import vcf
    from dl4vc_amd.compare import compare_scored_vcfs
    from oracle.fuzz_cases import scored_vcf_pair_cases

    def genotypes(text):
        out = {}
        for line in text.splitlines():
            if not line.startswith("#"):
                c = line.split("\t")
                out[(c[0], c[1], c[3], c[4])] = c[9].split(":")[0]
        return out

    pairs, stored = scored_vcf_pair_cases(), ref_texts["format_vcf_pairs"]
    assert len(pairs) == len(stored) == 12
    total_diff = 0
    for trial, ((ta, tb), ref) in enumerate(zip(pairs, stored)):
        assert ta == ref["a"] and tb == ref["b"], "trial %d: the seeded case differs from the fixture's" % trial
        ga, gb = genotypes(ref["formatted_a"]), genotypes(ref["formatted_b"])
        want = {k for k in set(ga) | set(gb) if ga.get(k) != gb.get(k)}
        rep = compare_scored_vcfs(ta.splitlines(keepends=True), tb.splitlines(keepends=True), vcf.FormatOptions(**vcf.PIPELINE_OPTIONS), max_listed=1000)
        got = set()
        for kind in ("knife_edge", "elsewhere"):
            for e in rep["genotype_differences"][kind]["first"]:
                m = e["site"]
                chrom_pos, alle = m.split(" ")
                chrom, pos = chrom_pos.split(":")
                r, al = alle.split(">")
                got.add((chrom, pos, r, al))
        assert got == want, (trial, got ^ want)
        # every difference between two files 2e-5 apart is a knife edge by the tool's own attribution
        assert rep["genotype_differences"]["elsewhere"]["count"] == 0 and rep["ok"], rep["genotype_differences"]["elsewhere"]
        total_diff += len(want)
    assert total_diff >= 5, "the trials produced too few threshold crossings to test anything: %d" % total_diff
