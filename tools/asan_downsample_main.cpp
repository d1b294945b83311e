// Stand-alone driver of tools/asan_downsample.sh: dan_loader.cpp (dl_select_rows_downsample) and store_capi.cpp built host-only
// (cl_store_assemble_host, the CPU twin of the store's gather) compiled into this program under the sanitizers, run over the cases
// of tests/golden/dataset_downsample.npz, which the script wrote as text into the file given as argv[1]:
//   * every case's plan into heap buffers of exactly the size the header promises, compared with the fixture's permutation, zero
//     flags and kept reads;
//   * the fixture's record packed into a host store in the rows and in the compact format, and every case's plan -- its entries
//     carrying the zero-reads bit (dl4vc_amd/csrc/plan_entry.h) -- gathered by cl_store_assemble_host into heap buffers that end
//     where their data ends, compared with the fixture's three planes;
//   * the refusals: a rate or a prob outside its range, a flagged entry that names a row past the stored rows.
// Exit status 0 and "asan_downsample: ok" when every call gave what it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "../include/dl4vc_chunks.h"
#include "../include/dl4vc_loader.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; fprintf(stderr, "asan_downsample: FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static long read_int(FILE* f) {
    long v = 0;
    if (fscanf(f, "%ld", &v) != 1) { fprintf(stderr, "asan_downsample: the case file ends early\n"); exit(2); }
    return v;
}
static double read_double(FILE* f) {
    double v = 0;
    if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "asan_downsample: the case file ends early\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: asan_downsample CASES (written by tools/asan_downsample.sh)\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "asan_downsample: cannot open %s\n", argv[1]); return 2; }
    const int S = (int)read_int(f), W = (int)read_int(f), N = (int)read_int(f);
    const size_t plane = (size_t)S * W;
    std::unique_ptr<uint8_t[]> rec[3];
    for (auto& p : rec) {
        p.reset(new uint8_t[plane]);
        for (size_t i = 0; i < plane; ++i) p[i] = (uint8_t)read_int(f);
    }
    cl_store_t* store[2] = {nullptr, nullptr};
    const int32_t slot = 0;
    for (int fmt = 0; fmt < 2; ++fmt) {
        int32_t kept = -1;
        CHECK(cl_store_open(W, S, 1, 1 << 20, 1 << 16, -1, &store[fmt]) == 0 && store[fmt]);
        if (!store[fmt]) return 1;
        CHECK(cl_store_set_format(store[fmt], fmt) == 0);
        CHECK(cl_store_pack_planes_host(store[fmt], rec[0].get(), rec[1].get(), rec[2].get(), 1, &slot, &slot, 1, &kept) == 0 && kept == S);
    }
    cl_store_format_stats fs{};
    CHECK(cl_store_get_format_stats(store[1], &fs) == 0 && fs.compact_records == 1);
    std::vector<uint8_t> line((size_t)W, 7);
    for (int c = 0; c < N; ++c) {
        const int n = (int)read_int(f), R = (int)read_int(f);
        const double rate = read_double(f), prob = read_double(f);
        const uint32_t seed = (uint32_t)read_int(f);
        const int sampled = (int)read_int(f), k = (int)read_int(f);
        std::vector<int> perm(k), zero(k);
        for (int& v : perm) v = (int)read_int(f);
        for (int& v : zero) v = (int)read_int(f);
        std::vector<uint8_t> want[3];
        for (auto& w : want) {
            w.resize((size_t)k * W);
            for (uint8_t& b : w) b = (uint8_t)read_int(f);
        }
        const size_t room = (size_t)std::max(R, S);
        std::unique_ptr<int32_t[]> rows(new int32_t[room]);
        std::unique_ptr<uint8_t[]> flags(new uint8_t[room]);
        int32_t got_sampled = -1;
        const int got = dl_select_rows_downsample(seed, n, S, R, rate, prob, rows.get(), flags.get(), &got_sampled);
        CHECK(got == k && got_sampled == sampled);
        if (got != k) continue;
        bool same = true;
        for (int i = 0; i < k; ++i) same = same && rows[i] == perm[i] && flags[i] == zero[i];
        CHECK(same);
        CHECK(dl_select_rows_downsample(seed, n, S, R, rate, prob, rows.get(), flags.get(), nullptr) == k);
        std::unique_ptr<int16_t[]> plan(new int16_t[(size_t)k]);
        for (int i = 0; i < k; ++i) plan[i] = (int16_t)(perm[i] | (zero[i] ? 0x4000 : 0));
        const uint8_t first = 0;
        for (int fmt = 0; fmt < 2; ++fmt) {
            std::unique_ptr<uint8_t[]> out[6];
            for (int p = 0; p < 6; ++p) {
                const size_t bytes = p < 3 ? (size_t)k * W : (size_t)W;
                out[p].reset(new uint8_t[bytes]);
                memset(out[p].get(), 0xAB, bytes);
            }
            CHECK(cl_store_assemble_host(store[fmt], &slot, plan.get(), &first, 1, k, line.data(), line.data(), line.data(), 1, 1, out[0].get(),
                                         out[1].get(), out[2].get(), out[3].get(), out[4].get(), out[5].get(), nullptr) == 0);
            for (int p = 0; p < 3; ++p) CHECK(memcmp(out[p].get(), want[p].data(), want[p].size()) == 0);
            CHECK(memcmp(out[3].get(), line.data(), (size_t)W) == 0);
        }
    }
    fclose(f);
    // refusals
    int32_t rows[256];
    uint8_t flags[256];
    CHECK(dl_select_rows_downsample(1, 10, 200, 8, 1.0, 0.5, rows, flags, nullptr) == -1);
    CHECK(dl_select_rows_downsample(1, 10, 200, 8, 0.3, 1.5, rows, flags, nullptr) == -1);
    CHECK(dl_select_rows_downsample(1, 10, 200, 8, 0.3, 0.5, nullptr, flags, nullptr) == -1 && dl_last_error(nullptr)[0] != 0);
    {
        const int16_t bad[2] = {(int16_t)(0x4000 | S), 0};
        const uint8_t first = 0;
        std::vector<uint8_t> o((size_t)2 * W, 0xAB), l((size_t)W, 0xAB);
        CHECK(cl_store_assemble_host(store[0], &slot, bad, &first, 1, 2, line.data(), line.data(), line.data(), 1, 1, o.data(), o.data(), o.data(),
                                     l.data(), l.data(), l.data(), nullptr) == -1);
        CHECK(std::all_of(o.begin(), o.end(), [](uint8_t b) { return b == 0xAB; }));
    }
    for (cl_store_t* st : store) cl_store_close(st);
    printf("asan_downsample: %s (%d cases, %d failures)\n", failures ? "FAILED" : "ok", N, failures);
    return failures ? 1 : 0;
}
