#!/bin/bash
# CPU sanitizer pass over dan_finalize's host half (dl4vc_amd/csrc/dan_pack.h: the tensor checks and the packing of every weight
# block the DAN kernels read): builds the stand-alone driver tools/dan_pack_main.cpp with -fsanitize=address,undefined into a
# scratch directory and runs it: five small networks at the three precisions, every tensor and every packed block a heap vector
# that ends where its data ends, every element read back through its layout's index formula.
# CPU only, a program of its own (nothing is loaded into python).
# usage: tools/asan_dan_pack.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -D__HIP_PLATFORM_AMD__ -I"${ROCM_PATH:-/opt/rocm}/include" -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -fno-omit-frame-pointer tools/dan_pack_main.cpp -o "$out/asan_dan_pack"
"$out/asan_dan_pack"
rm -rf "$out"
