#!/bin/bash
# CPU sanitizer pass over the read subsampling rule (dl4vc_amd/csrc/bam_frame.h: name_hash, wang, sampled -- the text the host paths
# and the GPU frame kernels run): builds the stand-alone driver tools/asan_subsample_main.cpp with -fsanitize=address,undefined
# into a scratch directory (the argument, or a temporary one) and runs it: records with l_read_name of 1, 2 and 255, a name with
# no NUL, bytes >= 0x80 and a record cut right behind the name, each in a heap buffer of exactly its size.  CPU only, a program of
# its own (nothing is loaded into python).
# usage: tools/asan_subsample.sh [SCRATCH_DIR]
set -e
cd "$(dirname "$0")/.."
out=${1:-$(mktemp -d)}
g++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    tools/asan_subsample_main.cpp -o "$out/asan_subsample"
"$out/asan_subsample"
[ -n "$1" ] || rm -rf "$out"
