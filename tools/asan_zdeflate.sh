#!/bin/bash
# CPU sanitizer pass over the encode core of the zlib compressor (dl4vc_amd/csrc/zdeflate.h, the text the GPU kernel runs): builds
# the host entries of zdeflate_capi.cpp and the stand-alone driver tools/asan_zdeflate_main.cpp with -fsanitize=address,undefined
# into a scratch directory and runs the driver: the case grid into buffers of exactly zd_bound bytes, every stream inflated by zlib.
# CPU only, a program of its own (nothing is loaded into python); run it before the kernel goes near a GPU.
# usage: tools/asan_zdeflate.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -DZD_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/zdeflate_capi.cpp tools/asan_zdeflate_main.cpp -o "$out/asan_zdeflate" -lz
"$out/asan_zdeflate"
rm -rf "$out"
