#!/bin/bash
# CPU sanitizer pass over the native side of dynamic read down-sampling: the row plan (dl_select_rows_downsample of
# dl4vc_amd/csrc/dan_loader.cpp) and the CPU twin of the store's gather with flagged plan entries (cl_store_assemble_host of
# store_capi.cpp, built host-only).  A plain python child writes the cases of tests/golden/dataset_downsample.npz as text into a
# scratch directory; the two sources and the stand-alone driver tools/asan_downsample_main.cpp are built into one program with
# -fsanitize=address,undefined and the program is run over that file.  CPU only, a program of its own (nothing is loaded into
# python under a sanitizer).
# usage: tools/asan_downsample.sh
set -e
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
python - "$out/cases.txt" <<'EOF'
import sys
import numpy as np
g = np.load("tests/golden/dataset_downsample.npz")
S, W = g["record_reads"].shape
with open(sys.argv[1], "w") as f:
    f.write("%d %d %d\n" % (S, W, len(g["seed"])))
    for p in ("record_reads", "record_qual", "record_strand"):
        f.write(" ".join(map(str, g[p].reshape(-1).tolist())) + "\n")
    for i in range(len(g["seed"])):
        k = min(int(g["model_reads"][i]), S)
        f.write("%d %d %.17g %.17g %d %d %d\n" % (g["num_reads"][i], g["model_reads"][i], g["rate"][i], g["prob"][i], g["seed"][i],
                                                 g["sampled"][i], k))
        for a in (g["perm"][i, :k], g["zero_reads"][i, :k], g["reads"][i, :k], g["qual"][i, :k], g["strand"][i, :k]):
            f.write(" ".join(map(str, a.reshape(-1).tolist())) + "\n")
EOF
g++ -O1 -g -std=c++17 -Wall -DCL_STORE_HOST_ONLY -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    dl4vc_amd/csrc/dan_loader.cpp dl4vc_amd/csrc/dan_pileup.cpp dl4vc_amd/csrc/store_capi.cpp tools/asan_downsample_main.cpp \
    -o "$out/asan_downsample" -lz -ldl -lpthread
ASAN_OPTIONS=detect_leaks=0 "$out/asan_downsample" "$out/cases.txt"
