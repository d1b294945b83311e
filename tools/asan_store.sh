#!/bin/bash
# CPU sanitizer pass over the record store's CPU definitions (dl4vc_amd/csrc/store_host.h behind the cl_store_*_host entries of
# store_capi.cpp: extent, layout and pack, assembly): builds store_capi.cpp host-only and the stand-alone driver
# tools/asan_store_main.cpp with -fsanitize=address,undefined into a scratch directory and runs the driver: the inflated records,
# the slabs and every output plane in a heap buffer that ends where its data ends, source and destination alignments 0..15.  CPU
# only, a program of its own (nothing is loaded into python).
# usage: tools/asan_store.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -DCL_STORE_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/store_capi.cpp tools/asan_store_main.cpp -o "$out/asan_store"
"$out/asan_store"
rm -rf "$out"
