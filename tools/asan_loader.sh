#!/bin/bash
# CPU sanitizer pass over libdl4vc_loader.so's two sources, the native batched loader (dl4vc_amd/csrc/dan_loader.cpp, dl_*) and the
# native pileup encoder (dl4vc_amd/csrc/dan_pileup.cpp, pe_*): a plain python child writes the input files of
# tests/loader_shell_cases.py into a scratch directory (candidate files whose chunk 1 is damaged, record types whose fields leave
# the record, damaged BAM records), then both sources and the stand-alone driver tools/asan_loader_main.cpp are built into one
# program with -fsanitize=address,undefined and the program is run over that directory: every refusal, dl_close with and without
# pieces in flight, and every allocation of a run failing in turn.  libhdf5 is dlopen'ed by the program as by the library (its
# own allocations are why leaks are not looked for).  CPU only, a program of its own (nothing is loaded into python under a
# sanitizer).
# usage: tools/asan_loader.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
python tests/loader_shell_cases.py "$out"
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/dan_loader.cpp dl4vc_amd/csrc/dan_pileup.cpp tools/asan_loader_main.cpp -o "$out/asan_loader" -lz -ldl -lpthread
ASAN_OPTIONS=detect_leaks=0 "$out/asan_loader" "$out"
