#!/usr/bin/env python
"""Scoring straight from a BAM (``main.py --test_bam``) against the two steps it replaces (``tools/convert_bam_single_reads.py``,
then ``main.py --test_file``), on a seeded synthetic BAM: one contig at ~30x (150-base reads, a SNP allele in half of the reads
over every 50th candidate, an indel in 5 % of reads), a candidate every 10 bases -- by default 200 kbp and 19 940 locations, the
shape the GPU pileup encoder's own rate was measured on.  Production network, seeded random weights.

Alternating rounds (A B A B ...), each a fresh process as a user would start it, wall clock around the whole process:
  (i)   sites/s of the new path end to end, and its scoring loop's own clock;
  (ii)  wall time of the converter plus ``main.py --test_file`` on the same input;
  (iii) the rate of the forward alone on the same sites: the scoring loop ``main.py --test_file`` logs (planes already in the
        file; it runs at the device-resident rate of the forward, profiles/r05_e2e.json), and ``bench.py`` at the same size.
Both paths must write the same scored VCF; the tool fails if they do not.  One JSON record.

    python tools/score_bam_rate.py --dir /tmp/sbr [--length 200000 --rounds 3 --precision fp32] [--out profiles/x.json]

``--record-census gpu``: what the record census costs instead -- ``main.py --test_bam --record-census gpu`` (one GPU, one shard)
beside ``main.py --test_bam`` without the flag, alternating rounds of fresh processes on the same input, with ``--inflate-device
gpu`` off and on: each round's ``census_s`` (wall clock around the census) and ``census_ms`` (device time of its resolve and
census kernels), the census's locations/s, and the whole-process time of both arms.  Both arms must write the same scored VCF.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dl4vc_amd.bamio import BamWriter, build_bai, CMATCH, CINS, CDEL, FREVERSE   # noqa: E402

MODEL = ["--model-conv-layers", "7", "--model-residual-layer-start", "5", "--model-batchnorm", "--model-use-q-scores", "--model-use-strands",
         "--model-use-reads-ref-var-mask", "--model-highway-single-reads", "--model_concat_hw_reads", "--model_pool_combine_dimension", "0",
         "--model_middle_layer_dilation", "2", "--model_final_layer_dilation", "2", "--model-hidden-dropout", "0.1"]


def make_inputs(d, length, seed=7):
    """-> (bam, fasta, candidates.vcf, locations)."""
    bam, fa, vcf = os.path.join(d, "reads.bam"), os.path.join(d, "ref.fa"), os.path.join(d, "candidates.vcf")
    positions = list(range(300, length - 300, 10))
    if all(os.path.isfile(p) for p in (bam, bam + ".bai", fa, vcf)):
        return bam, fa, vcf, len(positions)
    rng = np.random.default_rng(seed)
    ref = "".join(rng.choice(list("ACGT"), length))
    with open(fa, "w") as f:
        f.write(">chr20\n" + "\n".join(ref[i:i + 60] for i in range(0, length, 60)) + "\n")
    alts = {p: ("A" if ref[p - 1] != "A" else "C") for p in positions}
    snps = np.array(positions[::50])
    n_reads = length * 30 // 150
    starts = np.sort(rng.integers(0, length - 152, n_reads))
    with BamWriter(bam, [("chr20", length)]) as w:
        for i, s in enumerate(starts.tolist()):
            seq, cigar = list(ref[s:s + 150]), [(CMATCH, 150)]
            if i % 2 == 0:
                for p in snps[np.searchsorted(snps, s + 1):np.searchsorted(snps, s + 150, side="right")]:
                    seq[int(p) - 1 - s] = alts[int(p)]
            if i % 20 == 0:
                if i % 40 == 0:
                    seq, cigar = seq[:70] + list(ref[s + 72:s + 152]), [(CMATCH, 70), (CDEL, 2), (CMATCH, 80)]
                else:
                    seq, cigar = seq[:70] + ["G", "T"] + seq[70:148], [(CMATCH, 70), (CINS, 2), (CMATCH, 78)]
            w.write(0, s, "frag%d" % i, FREVERSE if i % 2 else 0, 60, cigar, "".join(seq), rng.integers(15, 41, len(seq)).tolist())
    build_bai(bam, bam + ".bai")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=chr20,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n" % length)
        f.write("".join("chr20\t%d\t.\t%s\t%s\t50\t.\tDP=30;AF=0.5\tGT\t0/1\n" % (p, ref[p - 1], alts[p]) for p in positions))
    return bam, fa, vcf, len(positions)


def timed(cmd):
    t = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        sys.exit("%s failed:\n%s\n%s" % (" ".join(cmd[:3]), r.stdout[-1500:], r.stderr[-1500:]))
    return dt, r.stdout


def loop_clock(stdout):
    m = re.search(r"scoring loop .*: (\d+) sites in ([0-9.]+) s = (\d+) sites/s", stdout)
    return {"sites": int(m.group(1)), "s": float(m.group(2)), "sites_per_s": int(m.group(3))}


def census_arms(a, bam, fa, n_loc, common):
    """The arm with the record census beside the arm without, with the BAM inflated on the host and on the device."""
    res = {"tool": "score_bam_rate", "arm": "record_census", "locations": n_loc, "precision": a.precision, "same_scored_vcf": True}
    for inflate in (None, "gpu"):
        extra = ["--inflate-device", inflate] if inflate else []
        rounds = []
        for k in range(a.rounds):
            r = {}
            for arm, flag in (("test_bam", []), ("census", ["--record-census", "gpu"])):
                dt, out = timed([sys.executable, os.path.join(ROOT, "main.py"), "--test_bam", bam, "--test_fasta", fa,
                                 "--save_vcf_records_file", os.path.join(a.dir, arm + ".vcf")] + common + extra + flag + a.rf_flags)
                r[arm + "_wall_s"] = round(dt, 3)
                r[arm + "_loop"] = loop_clock(out)
                if flag:
                    m = re.search(r"record census: census_s ([0-9.]+) for (\d+) locations \((\d+) records; census_ms ([0-9.]+) on the device\)", out)
                    if not m:
                        sys.exit("no census line in:\n%s" % out[-1500:])
                    r.update(census_s=float(m.group(1)), census_records=int(m.group(3)), census_ms=float(m.group(4)),
                             census_locations_per_s=round(int(m.group(2)) / max(float(m.group(1)), 1e-9)))
            if open(os.path.join(a.dir, "epoch1_test_bam.vcf"), "rb").read() != open(os.path.join(a.dir, "epoch1_census.vcf"), "rb").read():
                sys.exit("round %d: the two arms wrote different scored VCFs" % k)
            rounds.append(r)
            print("inflate %s round %d: %s" % (inflate, k, json.dumps(r)), file=sys.stderr, flush=True)
        key = "inflate_device_gpu" if inflate else "inflate_host"
        res[key] = {"rounds": rounds, "sites": rounds[0]["census_loop"]["sites"],
                    "test_bam_wall_s": [r["test_bam_wall_s"] for r in rounds], "census_wall_s": [r["census_wall_s"] for r in rounds],
                    "census_s": [r["census_s"] for r in rounds], "census_ms": [r["census_ms"] for r in rounds],
                    "census_locations_per_s": [r["census_locations_per_s"] for r in rounds],
                    "census_arm_slower_by_s_median": round(float(np.median([r["census_wall_s"] - r["test_bam_wall_s"] for r in rounds])), 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", required=True, help="working directory (inputs are made there once and reused)")
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--threads", type=int, default=16, help="--num-processes of the converter")
    ap.add_argument("--no-bench", action="store_true", help="skip the bench.py run of the forward alone")
    ap.add_argument("--inflate-device", default=None, choices=["gpu"], help="passed to main.py --test_bam")
    ap.add_argument("--record-census", dest="record_census", default=None, choices=["gpu"],
                    help="measure main.py --test_bam --record-census gpu beside --test_bam instead (see above)")
    ap.add_argument("--out", default=None)
    from dl4vc_amd import read_filter
    read_filter.add_flags(ap)
    a = ap.parse_args()
    # the read filter goes to the converter and to main.py --test_bam alike (a --test_file run reads no BAM and gets none)
    rf_flags = read_filter.cli_flags(read_filter.parse(ap, a), a.read_stats)
    os.makedirs(a.dir, exist_ok=True)
    t = time.time()
    bam, fa, vcf, n_loc = make_inputs(a.dir, a.length)
    print("inputs: %d locations (%.1f s)" % (n_loc, time.time() - t), file=sys.stderr, flush=True)
    import torch
    from dl4vc_amd.config import DanConfig
    from dl4vc_amd.synth import random_state_dict
    ck = os.path.join(a.dir, "ckpt.pth.tar")
    if not os.path.isfile(ck):
        torch.save({"state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=1).items()}}, ck)
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--sites-per-launch", "4096", "--precision", a.precision] + MODEL
    a.rf_flags = rf_flags
    if a.record_census:
        line = json.dumps(census_arms(a, bam, fa, n_loc, common))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            open(a.out, "w").write(line + "\n")
        return 0
    hdf = os.path.join(a.dir, "candidates.hdf")
    rounds = []
    for k in range(a.rounds):
        if os.path.isfile(hdf):
            os.remove(hdf)
        t_conv, _ = timed([sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf,
                           "--fasta-input", fa, "--output", hdf, "--max-reads", "200", "--num-processes", str(a.threads),
                           "--locations-process-step", "100000", "--max-insert-length", "10", "--max-insert-length-variant", "50",
                           "--save-q-scores", "--save-strand"] + [f for f in rf_flags if f != "--read-stats"])
        t_file, out_file = timed([sys.executable, os.path.join(ROOT, "main.py"), "--test_file", hdf, "--save_vcf_records_file",
                                  os.path.join(a.dir, "two_step.vcf")] + common)
        t_bam, out_bam = timed([sys.executable, os.path.join(ROOT, "main.py"), "--test_bam", bam, "--test_fasta", fa,
                                "--save_vcf_records_file", os.path.join(a.dir, "direct.vcf")] + common +
                               (["--inflate-device", a.inflate_device] if a.inflate_device else []) + rf_flags)
        same = open(os.path.join(a.dir, "epoch1_two_step.vcf"), "rb").read() == open(os.path.join(a.dir, "epoch1_direct.vcf"), "rb").read()
        if not same:
            sys.exit("round %d: the two paths wrote different scored VCFs" % k)
        enc = re.search(r"pileup encoder: (\d+) locations: (\d+) on the GPU, (\d+) by pe_encode, (\d+) by the Python builder, (\d+) without",
                        out_bam)
        r = {"two_step_wall_s": round(t_conv + t_file, 3), "converter_wall_s": round(t_conv, 3), "test_file_wall_s": round(t_file, 3),
             "test_bam_wall_s": round(t_bam, 3), "test_file_loop": loop_clock(out_file), "test_bam_loop": loop_clock(out_bam),
             "encoder_counts": [int(x) for x in enc.groups()] if enc else None, "hdf_mb": round(os.path.getsize(hdf) / 1e6, 1)}
        rounds.append(r)
        print("round %d: %s" % (k, json.dumps(r)), file=sys.stderr, flush=True)
    sites = rounds[0]["test_bam_loop"]["sites"]
    best_bam = min(r["test_bam_wall_s"] for r in rounds)
    fwd = max(r["test_file_loop"]["sites_per_s"] for r in rounds)
    loop = max(r["test_bam_loop"]["sites_per_s"] for r in rounds)
    res = {"tool": "score_bam_rate", "inflate_device": a.inflate_device, "locations": n_loc, "sites": sites, "precision": a.precision, "rounds": rounds,
           "read_filter": rf_flags or None,
           "i_test_bam_sites_per_s_whole_process": round(sites / best_bam), "i_test_bam_sites_per_s_scoring_loop": loop,
           "ii_two_step_wall_s": [r["two_step_wall_s"] for r in rounds], "i_test_bam_wall_s": [r["test_bam_wall_s"] for r in rounds],
           "test_bam_faster_in_every_round": all(r["test_bam_wall_s"] < r["two_step_wall_s"] for r in rounds),
           "iii_forward_sites_per_s_test_file_loop": fwd, "ratio_i_to_iii": round(loop / fwd, 3), "same_scored_vcf": True}
    if not a.no_bench:
        b = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--reads", "100", "--sites", str(sites), "--steps", "2", "--warmup", "1",
                            "--precision", str(("fp32", "bf16x3", "bf16").index(a.precision)), "--skip-empty-rows", "--no-cpu-baseline",
                            "--no-host-path", "--no-oracle-check"], capture_output=True, text=True)
        line = [l for l in b.stdout.splitlines() if l.startswith("{")]
        res["iii_forward_sites_per_s_bench_synthetic"] = json.loads(line[-1])["value"] if line else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0 if res["test_bam_faster_in_every_round"] else 1


if __name__ == "__main__":
    sys.exit(main())
