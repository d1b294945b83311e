#!/bin/bash
# CPU sanitizer pass over the BGZF decode core (dl4vc_amd/csrc/bgzf_inflate.h, the text the GPU kernel runs): builds the host entry
# of bgzf_capi.cpp with -fsanitize=address,undefined into a scratch directory and runs the case grid of tests/bgzf_cases.py, valid
# and damaged, through it.  CPU only; run it before damaged blocks go near a GPU.  usage: tools/asan_bgzf.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -fPIC -shared -DBZ_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/bgzf_capi.cpp -o "$out/libdl4vc_bgzf_host.so"
asan=$(g++ -print-file-name=libasan.so)
ubsan=$(g++ -print-file-name=libubsan.so)
DL4VC_BGZF_HOST_LIB="$out/libdl4vc_bgzf_host.so" LD_PRELOAD="$asan $ubsan" ASAN_OPTIONS=detect_leaks=0 \
    python -m pytest tests/test_bgzf_inflate_host.py -q -x -k "grid or valid or damaged" "$@"
rm -rf "$out"
