#!/bin/bash
# CPU sanitizer pass over the left-alignment rule of candidate generation (dl4vc_amd/csrc/cand_left_align.h, the rule
# Walk::close_run runs on the GPU with cg_set_left_align): builds the stand-alone driver tools/asan_left_align_main.cpp, which
# includes the header itself, and cand_reference_capi.cpp host-only (for cg_left_align_host) with -fsanitize=address,undefined
# into a scratch directory and runs the driver: the enumerated grid (contigs of 1..12 bases over {A, C, N} in heap buffers that
# end where they end, every anchor, L in 1..4, both kinds, every floor) and hostile observations (an anchor at 0 and outside the
# contig, a + L at and past the contig's end, L = 63 and beyond).  CPU only, a program of its own (nothing is loaded into python).
# usage: tools/asan_left_align.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -DCG_REFERENCE_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/cand_reference_capi.cpp tools/asan_left_align_main.cpp -o "$out/asan_left_align"
"$out/asan_left_align"
rm -rf "$out"
