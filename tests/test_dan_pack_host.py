"""dan_finalize's host half (dl4vc_amd/csrc/dan_pack.h: tensor checks and the packing of every weight block) on the CPU, no GPU:
tools/dan_pack_main.cpp, a stand-alone driver, built here with g++ and run as a child process.  It packs random tensors of five
small networks (16 / 33 / 128 channels, bottleneck 0 / 8 / 32, windows 8 / 16 / 209, 1 / 3 / 7 layers, with and without q, strand,
mask channels, BatchNorm, residuals and pool layers) at the three precisions and looks every (output, input, tap) of every block
up through the index formula its layout documents: the expected value there, zero wherever no formula reaches, the constants,
res_mask, and the codes and texts of the missing-tensor and wrong-shape refusals."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_every_packed_block_reads_back(tmp_path):
    exe = str(tmp_path / "dan_pack_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE,
                    os.path.join(ROOT, "tools", "dan_pack_main.cpp"), "-o", exe], check=True, capture_output=True, text=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    m = re.match(r"ok: (\d+) checks, 0 mismatches\n$", r.stdout)
    assert m and int(m.group(1)) > 20_000_000, r.stdout[-3000:]
