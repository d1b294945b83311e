#!/bin/bash
# CPU sanitizer pass over the framing of the GPU pileup encoder's device inflate path: builds pg_debug_run_records
# (dl4vc_amd/csrc/pileup_debug.cpp: the planning of bgzf_plan.h, the decode core of bgzf_inflate.h and the frame core of
# bam_frame.h with the encoder's own part in pileup_frame.h, the text the kernels run) with -fsanitize=address,undefined into a
# scratch directory and runs the grid and the damaged inputs of tests/pileup_inflate_cases.py through both of its paths.  CPU
# only; run it before damaged files go near a GPU.  usage: tools/asan_pileup_frame.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
g++ -O1 -g -std=c++17 -fPIC -shared -DPG_HOST_ONLY -DBZ_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -fno-omit-frame-pointer dl4vc_amd/csrc/pileup_debug.cpp dl4vc_amd/csrc/bgzf_capi.cpp -o "$out/libdl4vc_pileup_host.so" -lz
asan=$(g++ -print-file-name=libasan.so)
ubsan=$(g++ -print-file-name=libubsan.so)
DL4VC_PILEUP_HOST_LIB="$out/libdl4vc_pileup_host.so" LD_PRELOAD="$asan $ubsan" ASAN_OPTIONS=detect_leaks=0 \
    python -m pytest tests/test_pileup_frame_host.py -q -x "$@"
rm -rf "$out"
