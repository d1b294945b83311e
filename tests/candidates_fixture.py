"""Shared by tests/test_candidates_host.py and tests/test_candidates_gpu.py: the fixtures of tools/gen_golden_candidates.py
and a BAM (+ BAI) writer for their reads."""
import gzip
import json
import os

from dl4vc_amd.bamio import BamWriter, build_bai

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("edge", "nochr", "random")


def load(name):
    with gzip.open(os.path.join(GOLDEN, "candidates_%s.json.gz" % name), "rt") as f:
        return json.load(f)


def md_aux(md):
    return b"" if md is None else b"NMC\x00MDZ" + md.encode() + b"\x00"


def write_bam(fx, path, index=True):
    with BamWriter(path, [tuple(r) for r in fx["references"]]) as w:
        for r in fx["reads"]:
            w.write(r["tid"], r["pos"], r["name"], r["flag"], 60, [tuple(c) for c in r["cigar"]], r["seq"], aux=md_aux(r["md"]))
    if index:
        build_bai(path, path + ".bai")
    return path
