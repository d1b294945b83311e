#!/bin/bash
# CPU sanitizer pass over the BAM frame core (dl4vc_amd/csrc/bam_frame.h, the text the host paths and the GPU kernels run): builds
# the stand-alone driver tools/asan_bam_frame_main.cpp with -fsanitize=address,undefined into a scratch directory and runs it: the
# case grid of well-formed and damaged records, each in a heap buffer of exactly its size.  CPU only, a program of its own (nothing
# is loaded into python); run it before the kernels go near a GPU.
# usage: tools/asan_bam_frame.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    tools/asan_bam_frame_main.cpp -o "$out/asan_bam_frame"
"$out/asan_bam_frame"
rm -rf "$out"
