#!/bin/bash
# CPU sanitizer pass over the reference-base conversion of candidate generation (cg_reference_codes_host: the loop over the
# per-base rule of dl4vc_amd/csrc/cand_reference.h, the rule reference_codes_kernel runs on the GPU): builds
# cand_reference_capi.cpp host-only and the stand-alone driver tools/asan_cand_reference_main.cpp with
# -fsanitize=address,undefined into a scratch directory and runs the driver: raw bytes and codes in heap buffers that end where
# they end, lengths around a line's, LF / CRLF / no final line end, every byte value, and indexes that do not describe the bytes.
# CPU only, a program of its own (nothing is loaded into python).
# usage: tools/asan_cand_reference.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -DCG_REFERENCE_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/cand_reference_capi.cpp tools/asan_cand_reference_main.cpp -o "$out/asan_cand_reference"
"$out/asan_cand_reference"
rm -rf "$out"
