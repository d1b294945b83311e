"""The random cases of tests/test_vs_live_reference.py, generated from fixed seeds.

oracle/gen_golden_fuzz.py runs the reference on these cases and stores its outputs in tests/golden/fuzz_reference.*; the
tests regenerate the same cases, check that they are the ones the fixture was written for, and compare against the stored
outputs.  Nothing here calls the reference."""
from __future__ import annotations

import hashlib
import random

import numpy as np

from oracle.dan_oracle import OracleSpec, random_state_dict
from dl4vc_amd import synth

VCF_HEADER = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n"
ALLELES_POOL = [("A", "G"), ("C", "T"), ("AT", "A"), ("A", "AT"), ("ATG", "A"), ("A", "ATGC"), ("G", "C"), ("T", "A")]
# the options format_vcf.py is called with (call_variants.sh's thresholds)
FORMAT_VCF_ARGS = dict(snp_threshold=0.1, indel_threshold=0.2, long_indel_threshold=0.0, delete_threshold=0.0,
                       snp_zygo_threshold=0.75, indel_zygo_threshold=0.8, long_indel_zygo_threshold=0.5, delete_zygo_threshold=0.5,
                       multiallele_second_threshold=0.7, multiallele_homozygous_second_threshold=0.9, debug=False)


TAP_SAMPLE = 4096


def tap_sample(name, a):
    """The elements of an activation tap the fixture keeps: a conv tap larger than TAP_SAMPLE elements is reduced to a fixed
    sample of TAP_SAMPLE positions over all its sites, channels, reads and columns (seeded by its size and layer, sorted);
    everything else (heads, feature row, hidden layer, highway outputs) whole."""
    a = np.asarray(a)
    if not name.startswith("conv") or a.size <= TAP_SAMPLE:
        return a
    idx = np.random.default_rng([a.size, int(name[4:])]).choice(a.size, TAP_SAMPLE, replace=False)
    return a.reshape(-1)[np.sort(idx)]


def digest(sd, batch) -> str:
    """sha256 of a case's weights and inputs: the fixture records it, the tests check it (same seeds, same case)."""
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    for a in batch.arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def structural_cases():
    """[(trial, spec, state dict, batch)]: random structural configurations of the network, fp32."""
    rng = random.Random(5)
    cases = []
    for trial in range(9):
        layers = rng.choice([3, 4, 5, 7])
        pools = tuple(sorted(rng.sample(range(1, layers), rng.choice([0, 1, 2]) if layers > 2 else 0)))
        # a third of the trials above the reference's MAX_READS = 100 (gen_golden.build_reference_model raises the constant in the
        # imported module for those: dl4vc/model.py:12,194,303-304)
        spec = OracleSpec(reads=(rng.choice([101, 117, 128]) if trial % 3 == 1 else rng.choice([3, 5, 8])), c_init=rng.choice([4, 8, 12]), c_final=rng.choice([4, 8, 12]),
                          layers=layers, pool_layers=pools, residual_start=rng.choice([0, 2, 3]),
                          dil_mid=rng.choice([1, 2, 3]), dil_final=rng.choice([1, 2]), use_bn=rng.random() < 0.7,
                          use_q=rng.random() < 0.7, use_strand=rng.random() < 0.7, use_mask=rng.random() < 0.8,
                          bottleneck=rng.choice([0, 2, 4]), fc_sizes=(rng.choice([8, 12]), rng.choice([4, 6])))
        if spec.residual_start > layers:
            continue
        sd = random_state_dict(spec, seed=300 + trial)
        batch = synth.make_sites(3, reads=spec.reads, seed=400 + trial)
        cases.append((trial, spec, sd, batch))
    return cases


def bf16_operand_cases():
    """[(i, spec, state dict, batch)]: the production structure at 301 columns, one above MAX_READS, four random structures."""
    rng = random.Random(11)
    specs = [OracleSpec(reads=6, length=301, c_init=16, c_final=16, bottleneck=4, fc_sizes=(16, 8)),
             OracleSpec(reads=109, length=240, c_init=8, c_final=8, bottleneck=4, fc_sizes=(8, 4), pool_layers=(2, 4))]   # > MAX_READS
    for trial in range(4):
        layers = rng.choice([3, 5, 7])
        pools = tuple(sorted(rng.sample(range(1, layers), rng.choice([0, 1]))))
        specs.append(OracleSpec(reads=rng.choice([3, 5]), c_init=rng.choice([8, 12]), c_final=rng.choice([8, 12]), layers=layers,
                                pool_layers=pools, residual_start=rng.choice([0, 2, 3]), dil_mid=rng.choice([1, 2]),
                                dil_final=2, use_bn=rng.random() < 0.7, bottleneck=rng.choice([0, 4]), fc_sizes=(8, 4)))
    cases = []
    for i, spec in enumerate(specs):
        if spec.residual_start > spec.layers:
            continue
        sd = random_state_dict(spec, seed=700 + i)
        batch = synth.make_sites(3, reads=spec.reads, length=spec.length, seed=800 + i)
        cases.append((i, spec, sd, batch))
    return cases


def allele_cases():
    """[(VCF record, 201-column reference window)]: random SNPs, insertions, deletions and complex alleles around gap columns."""
    rng = np.random.default_rng(9)
    bases = "ACGT"
    cases = []
    for trial in range(300):
        window = rng.integers(1, 5, 201).astype(np.uint8)
        for g in rng.integers(95, 115, rng.integers(0, 4)):
            window[g] = 5                                           # gap columns around the centre
        kind = rng.integers(0, 4)
        c = "ATGC"[window[100] - 1] if window[100] in (1, 2, 3, 4) else "A"
        tok2chr = {1: "A", 2: "T", 3: "G", 4: "C", 5: "N"}
        if kind == 0:
            ref_s, alt_s = c, bases[rng.integers(0, 4)]
        elif kind == 1:
            k = int(rng.integers(1, 6))
            ref_s, alt_s = c, c + "".join(bases[i] for i in rng.integers(0, 4, k))
        elif kind == 2:
            k = int(rng.integers(1, 6))
            tail = [tok2chr[int(t)] for t in window[101:140] if t != 5][:k]      # the deleted reference bases
            ref_s, alt_s = c + "".join(tail), c
        else:
            ref_s = "".join(bases[i] for i in rng.integers(0, 4, rng.integers(1, 4)))
            alt_s = "".join(bases[i] for i in rng.integers(0, 4, rng.integers(1, 4)))
        rec = "\t".join(("chr1", "77", ".", ref_s, alt_s, "50", ".", "DP=10;AF=0.5", "GT:GQ", "1:50"))
        cases.append((rec, window))
    return cases


def scored_vcf_cases():
    """[scored VCF text]: random multi-allelic sites with random scores, as main.py writes them (before format_vcf)."""
    rng = np.random.default_rng(3)
    texts = []
    for trial in range(25):
        lines, pos, used = [], 100, set()
        for _ in range(int(rng.integers(1, 40))):
            if rng.random() < 0.6:
                pos += int(rng.integers(1, 50))
                used = set()
            cands = [a for a in ALLELES_POOL if a not in used]      # identical lines trip an assert in the reference
            if not cands:
                continue
            ref_s, alt_s = cands[int(rng.integers(0, len(cands)))]
            used.add((ref_s, alt_s))
            p = rng.dirichlet((0.6, 0.6, 0.6)) if rng.random() < 0.7 else np.array([rng.random() * 0.2, 0.05, 0.0])
            nv, hv, ov = (float(x) for x in p / max(p.sum(), 1e-9)) if p.sum() > 0 else (1.0, 0.0, 0.0)
            lines.append("\t".join(("chr2", str(pos), "BP=%.8f;NV=%.8f;HV=%.8f;OV=%.8f" % (1 - nv, nv, hv, ov), ref_s, alt_s,
                                    "50", ".", "DP=30;AF=0.5", "GT:GQ", "1:50")))
        texts.append(VCF_HEADER + "\n".join(lines) + "\n")
    return texts


def scored_vcf_pair_cases():
    """[(text a, text b)]: pairs of scored VCFs, b = a with score noise of a few 1e-5 and some call scores planted next to the
    SNP / indel threshold, so that some sites cross it."""
    rng = np.random.default_rng(17)
    pairs = []
    for trial in range(12):
        recs, pos, used = [], 100, set()
        for _ in range(int(rng.integers(20, 60))):
            if rng.random() < 0.7:
                pos += int(rng.integers(1, 50))
                used = set()
            cands = [a for a in ALLELES_POOL if a not in used]
            if not cands:
                continue
            ref_s, alt_s = cands[int(rng.integers(0, len(cands)))]
            used.add((ref_s, alt_s))
            p = rng.dirichlet((0.6, 0.6, 0.6))
            if rng.random() < 0.25:                                  # plant the call score next to the SNP / indel threshold
                thr = 0.1 if (len(ref_s) == 1 and len(alt_s) == 1) else 0.2
                nv = 1.0 - thr + rng.uniform(-3e-5, 3e-5)
                p = np.array([nv, (1 - nv) * 0.7, (1 - nv) * 0.3])
            recs.append((pos, ref_s, alt_s, p))

        def text_of(scores):
            return VCF_HEADER + "".join("\t".join(("chr2", str(pos), "BP=%.8f;NV=%.8f;HV=%.8f;OV=%.8f" % (1 - s[0], s[0], s[1], s[2]), r, al,
                                                   "50", ".", "DP=30;AF=0.5", "GT:GQ", "1:50")) + "\n" for (pos, r, al, _), s in zip(recs, scores))
        sa = [p for _, _, _, p in recs]
        sb = []
        for p in sa:
            d = rng.normal(0, 2e-5, 3)
            q = np.clip(p + d - d.mean(), 0, 1)
            sb.append(q)
        pairs.append((text_of(sa), text_of(sb)))
    return pairs
