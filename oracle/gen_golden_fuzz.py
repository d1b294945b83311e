#!/usr/bin/env python3
"""Generate tests/golden/fuzz_reference.{npz,json.gz} by RUNNING THE REFERENCE on the random cases of oracle/fuzz_cases.py.

Runs only where the reference checkout is present (gen_golden.import_reference); nothing of the reference's source travels: the
fixtures hold the reference's outputs (a fixed sample of the larger conv activation taps: fuzz_cases.tap_sample) and a digest of
each case's inputs, which tests/test_vs_live_reference.py regenerates.

Usage:  python oracle/gen_golden_fuzz.py
"""
from __future__ import annotations

import contextlib
import gzip
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import gen_golden as G                                     # noqa: E402
from oracle import fuzz_cases as F                         # noqa: E402
from dl4vc_amd import vcf                                  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def run_format_vcf(fv, text, td):
    pin, pout = os.path.join(td, "in.vcf"), os.path.join(td, "out.vcf")
    with open(pin, "w") as f:
        f.write(text)
    a = types.SimpleNamespace(input_file=pin, output_file=pout, **F.FORMAT_VCF_ARGS)
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        fv.filter_format_vcf(a)
    with open(pout) as f:
        return f.read()


def main():
    m, d, _u = G.import_reference()
    arrays = {}
    for trial, spec, sd, batch in F.structural_cases():
        arrays["struct:%d:digest" % trial] = np.frombuffer(F.digest(sd, batch).encode(), np.uint8)
        for k, v in G.run_reference(m, spec, sd, batch, taps=False).items():
            arrays["struct:%d:out:%s" % (trial, k)] = np.asarray(v, np.float32)
    for i, spec, sd, batch in F.bf16_operand_cases():
        arrays["bf16:%d:digest" % i] = np.frombuffer(F.digest(sd, batch).encode(), np.uint8)
        for k, v in G.run_reference(m, spec, sd, batch, taps=True, bf16_operands=True).items():
            arrays["bf16:%d:out:%s" % (i, k)] = np.asarray(F.tap_sample(k, v), np.float32)
    np.savez_compressed(os.path.join(GOLD, "fuzz_reference.npz"), **arrays)

    alleles = []
    for rec, window in F.allele_cases():
        with contextlib.redirect_stdout(io.StringIO()):
            try:
                want = d.get_read_mask_vectors(rec, reference=window.copy())
                res = {"masks": [np.asarray(want[0]).tolist(), np.asarray(want[1]).tolist()]}
            except Exception as e:          # noqa: BLE001
                res = {"error": "AssertionError" if isinstance(e, AssertionError) else type(e).__name__}
        alleles.append(dict(res, rec=rec, window="".join(str(int(t)) for t in window)))
    with contextlib.redirect_stdout(io.StringIO()):
        fv = importlib.import_module("format_vcf")
    srt = lambda t: "".join(vcf.sort_scored_vcf_lines(t.splitlines(keepends=True)))      # noqa: E731
    with tempfile.TemporaryDirectory() as td:
        formatted = [{"scored": t, "formatted": run_format_vcf(fv, t, td)} for t in F.scored_vcf_cases()]
        # (the pipeline sorts the scored file before format_vcf -- call_variants.sh:151 -- so the reference program gets sorted text)
        pairs = [{"a": a, "b": b, "formatted_a": run_format_vcf(fv, srt(a), td), "formatted_b": run_format_vcf(fv, srt(b), td)}
                 for a, b in F.scored_vcf_pair_cases()]
    with gzip.open(os.path.join(GOLD, "fuzz_reference.json.gz"), "wt") as f:
        json.dump({"alleles": alleles, "format_vcf": formatted, "format_vcf_pairs": pairs}, f)
    print("wrote fuzz_reference.npz (%d arrays), fuzz_reference.json.gz (%d alleles, %d scored VCFs, %d pairs)"
          % (len(arrays), len(alleles), len(formatted), len(pairs)))


if __name__ == "__main__":
    main()
