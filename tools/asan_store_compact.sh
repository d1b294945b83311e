#!/bin/bash
# CPU sanitizer pass over the CPU twins of the record store's compact format (dl4vc_amd/csrc/store_host.h: spans_host,
# pack_compact_host, assemble_compact_plane_host behind the cl_store_* entries of store_capi.cpp): builds store_capi.cpp host-only
# and the stand-alone driver tools/asan_store_compact_main.cpp with -fsanitize=address,undefined into a scratch directory and runs
# the driver: the spans, the pack and the gather over records at the edges of a row's span, every source, slab and output plane
# in a heap buffer that ends where its data ends, source and destination alignments 0..15.  CPU only, a program of its own
# (nothing is loaded into python).
# usage: tools/asan_store_compact.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -DCL_STORE_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/store_capi.cpp tools/asan_store_compact_main.cpp -o "$out/asan_store_compact"
"$out/asan_store_compact"
rm -rf "$out"
