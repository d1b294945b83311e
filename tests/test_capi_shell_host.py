"""The shell of every extern "C" entry (dl4vc_amd/csrc/capi_shell.h) on the CPU, no GPU: tools/capi_shell_main.cpp, a stand-alone
driver, built here with g++ and run as a child process.  It calls capi::guarded with a body that returns a code, one that
reports through capi::failf and bodies that throw std::bad_alloc, std::runtime_error("x") and an int, and capi::failf with a
message of 2000 characters (cut at 1023, terminated), each with a plain and with a thread_local destination string, and
compares every return value and every text exactly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shell_codes_and_texts(tmp_path):
    exe = str(tmp_path / "capi_shell_driver")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", os.path.join(ROOT, "tools", "capi_shell_main.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.startswith("ok: 29 checks") and " 0 mismatches" in r.stdout, r.stdout
