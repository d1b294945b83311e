"""The BAM frame core (dl4vc_amd/csrc/bam_frame.h) on the CPU, no GPU: tools/asan_bam_frame_main.cpp, the stand-alone driver of
tools/asan_bam_frame.sh, built here without sanitizers and run as a child process.  It frames a grid of well-formed and damaged
records, each in a heap buffer of exactly its size, and compares the reason and every field with what the record was built
from: the aux area and MD:Z, the fixed fields, the CIGAR sums against the pileup encoder's span check, bam_endpos and the four
refusals of one step of the record chain."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frame_core_case_grid(tmp_path):
    exe = str(tmp_path / "bam_frame_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tools", "asan_bam_frame_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.startswith("ok: ") and " 0 mismatches" in r.stdout, r.stdout
