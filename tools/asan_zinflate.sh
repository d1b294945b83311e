#!/bin/bash
# CPU sanitizer pass over the zlib stream inflate (dl4vc_amd/csrc/zinflate.h over the decode core of bgzf_inflate.h: the text the
# GPU kernel runs, ring included): builds the host entries of zinflate_capi.cpp and zdeflate_capi.cpp (one of the grid's
# compressors) and the stand-alone driver tools/asan_zinflate_main.cpp with -fsanitize=address,undefined into a scratch directory
# and runs the driver: the case grid, the hand-assembled streams and the damaged streams, every stream and every slot in a heap
# buffer that ends where it ends.  CPU only, a program of its own (nothing is loaded into python); run it before the kernel goes
# near a GPU.
# usage: tools/asan_zinflate.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -DZI_HOST_ONLY -DZD_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/zinflate_capi.cpp dl4vc_amd/csrc/zdeflate_capi.cpp tools/asan_zinflate_main.cpp -o "$out/asan_zinflate" -lz
"$out/asan_zinflate"
rm -rf "$out"
