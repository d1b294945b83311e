"""The reference source of candidate generation, the parts that need no GPU: the byte-to-code conversion's CPU entry against a
Python restatement of its rule, the refusals of the tool and the two scripts before any device work, and the agreement of
include/dl4vc_candgen.h, libdl4vc_cand.so's exports and the binding for the new entries."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import candidates_reference_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cg_set_reference", "cg_get_reference_stats", "cg_reference_codes", "cg_reference_codes_host")


@pytest.fixture(scope="module")
def candgen():
    from dl4vc_amd import candgen
    if not os.path.isfile(candgen.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    candgen.load_library()
    return candgen


def test_host_conversion_against_the_rule_restated(candgen, tmp_path):
    shapes, bad = K.conversion_shapes()
    fa = K.write_fasta(K.make_genome(), str(tmp_path / "ref.fa"), True)
    raw_file = open(fa, "rb").read()
    for line in open(fa + ".fai"):
        name, n, off, lb, lw = line.split("\t")
        shapes.append((name, raw_file[int(off):], int(lb), int(lw), int(n)))
    seen = set()
    for name, raw, lb, lw, n in shapes:
        want, other = K.codes_py(raw, lb, lw, n)
        got, got_other = candgen.reference_codes(raw, lb, lw, n)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and got_other == other, name
        seen |= set(got.tolist())
    assert seen == set(range(16))
    raw = b"acgtnACGTN=*rX"
    got, other = candgen.reference_codes(raw, 14, 15, 14)
    assert got.tolist() == [1, 2, 4, 8, 15, 1, 2, 4, 8, 15, 0, 15, 5, 15] and other == 2
    with pytest.raises(ValueError):
        K.codes_py(*bad[1:])
    with pytest.raises(RuntimeError, match="base 99.*do not describe"):
        candgen.reference_codes(*bad[1:])
    with pytest.raises(RuntimeError, match="base 1"):                  # '>' of the next record where a base should be
        candgen.reference_codes(b"A>x\nCC\n", 2, 3, 2)
    with pytest.raises(RuntimeError, match="no FASTA layout"):
        candgen.reference_codes(b"ACGT", 0, 1, 4)
    with pytest.raises(RuntimeError, match="no FASTA layout"):
        candgen.reference_codes(b"ACGT", 4, 3, 4)


def test_md_for_writes_standard_tags():
    ref = "ACGTACGTNNACGT"
    M, I, D = 0, 1, 2
    assert K.md_for(ref, 0, [(M, 8)], "ACGTACGT") == "8"
    assert K.md_for(ref, 0, [(M, 8)], "ACCAACGT") == "2G0T4"
    assert K.md_for(ref, 1, [(M, 3), (D, 2), (M, 2)], "CGTGT") == "3^AC2"
    assert K.md_for(ref, 1, [(M, 3), (D, 2), (M, 2)], "CGTAT") == "3^AC0G1"
    assert K.md_for(ref, 0, [(M, 2), (I, 2), (M, 2)], "ACTTGT") == "4"
    assert K.md_for(ref, 6, [(M, 4)], "GNNA") == "1T0N0N0"         # N in the read, N in the reference: mismatches (calmd)
    assert K.md_for(ref, 10, [(M, 8)], "ACGTAAAA") == "4"            # past the contig's end: the tag ends short


def _tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "candidate_generator.py")] + list(args), capture_output=True,
                          text=True, timeout=120)


def test_tool_refuses_an_unreadable_reference_before_any_device_work(tmp_path):
    for extra in ([], ["--gpus", "2"]):
        r = _tool("--input", str(tmp_path / "absent.bam"), "--output", str(tmp_path / "o.vcf"), "--reference", "/nonexistent", *extra)
        assert r.returncode != 0 and "--reference /nonexistent is not a readable file" in r.stderr, (r.stdout, r.stderr)
        assert "absent.bam" not in r.stderr and not os.path.exists(str(tmp_path / "o.vcf"))     # (the BAM was not even opened)
    r = _tool("--input", str(tmp_path / "absent.bam"), "--reference", str(tmp_path))             # a directory
    assert r.returncode != 0 and "is not a readable file" in r.stderr


@pytest.mark.parametrize("script,args", [("call_variants.sh", ["-m", "m.pth", "-o", "OUT", "-i", "x.bam", "-f"]),
                                         (os.path.join("tools", "make_training_data.sh"), ["-i", "x.bam", "-t", "t.vcf", "-o", "OUT", "-f"])])
def test_scripts_refuse_f_without_r(script, args, tmp_path):
    args = [str(tmp_path / a) if a == "OUT" else a for a in args]
    r = subprocess.run(["bash", os.path.join(ROOT, script)] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "give -r REFERENCE as well" in r.stdout, (r.stdout, r.stderr)
    assert not os.path.exists(str(tmp_path / "OUT"))


def test_scripts_pass_the_reference_only_with_f():
    for script in ("call_variants.sh", os.path.join("tools", "make_training_data.sh")):
        text = open(os.path.join(ROOT, script)).read()
        assert text.count("--reference") == 2 and '${FROMREF:+--reference "$REFERENCE"}' in text, script


def test_the_flag_is_added_after_the_reference_tools_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import candidate_generator as cli
    assert "--reference" not in [s for a in cli.build_parser()._actions for s in a.option_strings]
    assert "--reference" in open(os.path.join(ROOT, "tools", "candidate_generator.py")).read().split("def main(")[1]


def test_warning_line_names_the_flag(caplog):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import candidate_generator as cli
    with caplog.at_level("WARNING"):
        cli.warn_no_md(dict(reads=10, reads_no_md=6), None)
    assert len(caplog.records) == 1 and "--reference" in caplog.text and "6 of 10" in caplog.text
    caplog.clear()
    with caplog.at_level("WARNING"):
        cli.warn_no_md(dict(reads=10, reads_no_md=5), None)          # half is not more than half
        cli.warn_no_md(dict(reads=10, reads_no_md=0), "ref.fa")
        cli.warn_no_md(dict(reads=0, reads_no_md=0), None)
    assert not caplog.records


def test_header_exports_and_binding_agree(candgen):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dl4vc_candgen.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cg_[a-z_]+)\s*\(", text))
    assert set(NEW) <= declared == {s for s in candgen.SYMBOLS if s.startswith("cg_")}
    lib = candgen.load_library()
    ctype_of = {"cg_handle_t*": ctypes.c_void_p, "const cg_handle_t*": ctypes.c_void_p, "const char*": ctypes.c_char_p,
                "const uint8_t*": ctypes.c_char_p, "uint8_t*": ctypes.c_void_p, "uint64_t": ctypes.c_uint64, "int64_t": ctypes.c_int64,
                "int64_t*": ctypes.POINTER(ctypes.c_int64), "int": ctypes.c_int,
                "cg_reference_stats*": ctypes.POINTER(candgen.ReferenceStats)}
    for name in NEW:
        assert hasattr(lib, name), name
        params = re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
        kinds = [re.sub(r"\s*\w+$", "", " ".join(p.split())).replace(" *", "*") for p in params.split(",")]
        assert [ctype_of[k] for k in kinds] == list(getattr(lib, name).argtypes), (name, kinds)
    body = re.search(r"typedef struct \{([^}]*)\} cg_reference_stats;", text, flags=re.S).group(1)
    fields = re.findall(r"(int64_t|double)\s+([a-z_]+)\s*;", body)
    assert [(n, ctypes.c_int64 if t == "int64_t" else ctypes.c_double) for t, n in fields] == list(candgen.ReferenceStats._fields_)
    # the structures that were there keep their layout
    assert ctypes.sizeof(candgen.Stats) == 10 * 8 + 4 * 8 and ctypes.sizeof(candgen.InflateStats) == 4 * 8 + 3 * 8
