#!/bin/bash
# CPU sanitizer pass over the record store's planar CPU definitions (cl_store_extent_planes_host, cl_store_pack_planes_host: the
# pileup encoder's three plane arrays as the source): builds store_capi.cpp host-only and the stand-alone driver
# tools/asan_store_planes_main.cpp with -fsanitize=address,undefined into a scratch directory and runs the driver: every plane
# array in a heap buffer that ends where it ends, source alignments 0..15, against cl_store_pack_host on the same slots as packed
# records.  CPU only, a program of its own (nothing is loaded into python).
# usage: tools/asan_store_planes.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -Wall -DCL_STORE_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/store_capi.cpp tools/asan_store_planes_main.cpp -o "$out/asan_store_planes"
"$out/asan_store_planes"
rm -rf "$out"
