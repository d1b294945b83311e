#!/bin/bash
# CPU sanitizer pass over the read filter and the host census (dl4vc_amd/csrc/bam_frame.h: passes, verdict, fate, Census -- the text
# the host paths and the GPU frame kernels run): builds the stand-alone driver tools/asan_read_filter_main.cpp with
# -fsanitize=address,undefined into a scratch directory (the argument, or a temporary one) and runs it: records of 33 bytes in heap
# buffers of exactly their size, every flag bit, the MAPQ values around the threshold, the census against counts kept beside it.
# CPU only, a program of its own (nothing is loaded into python).
# usage: tools/asan_read_filter.sh [SCRATCH_DIR]
set -e
cd "$(dirname "$0")/.."
out=${1:-$(mktemp -d)}
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    tools/asan_read_filter_main.cpp -o "$out/asan_read_filter"
"$out/asan_read_filter"
[ -n "$1" ] || rm -rf "$out"
