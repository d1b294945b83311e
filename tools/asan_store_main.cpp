// Stand-alone driver of tools/asan_store.sh: runs the CPU definitions of the record store (cl_store_extent_host,
// cl_store_pack_host, cl_store_assemble_host of dl4vc_amd/csrc/store_capi.cpp built host-only) on records of the candidate layout
// at 20 stored rows of 201 columns -- an odd record size, so the planes start at every byte alignment -- with extents 0, 1, the
// rows read, all stored rows and random ones between.  The inflated records sit in a heap buffer that ends where the last record
// ends and starts 0..15 bytes into its allocation; the store's one slab is exactly as large as the records need (the capacity is
// their sum), and a second store takes slabs of two records; every output plane sits in a heap buffer that ends where it ends and
// starts 0..15 bytes in.  The sanitizer sees any byte read or written past any of them.  Extents, stored bytes and assembled
// planes are compared with plain loops over the untrimmed records; the refusals must leave the store as it was.  Exit status 0
// when everything agrees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dl4vc_chunks.h"

static const int S = 20, W = 201, R = 12, N = 23, M = 9;
static const int64_t P0 = 16 + 15 * W, P1 = P0 + S * W + W + 133, P2 = P1 + S * W, RB = P2 + S * W;
static const int64_t OFF[3] = {P0, P1, P2};

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

static int failures = 0;
#define CHECK(x)                                                              \
    do {                                                                      \
        if (!(x)) {                                                           \
            if (++failures < 20) printf("line %d: %s\n", __LINE__, #x);      \
        }                                                                     \
    } while (0)

static uint64_t span(int kept) { return ((uint64_t)3 * kept * W + 15) & ~(uint64_t)15; }

// record i: `want` rows, the last of them non-zero in one plane only; everything outside the planes is 0xEE (never zero, never read)
static void make_records(uint8_t* rec, std::vector<int>& want) {
    static const int fixed[6] = {0, 1, R, S, R - 1, R + 1};
    want.resize(N);
    for (int i = 0; i < N; ++i) {
        uint8_t* r = rec + (size_t)i * RB;
        memset(r, 0xEE, (size_t)RB);
        const int k = i < 6 ? fixed[i] : (int)(rnd() % (S + 1));
        want[i] = k;
        for (int p = 0; p < 3; ++p) {
            uint8_t* q = r + OFF[p];
            memset(q, 0, (size_t)S * W);
            for (int row = 0; row + 1 < k; ++row)
                for (int c = 0; c < W; ++c) q[row * W + c] = (uint8_t)(rnd() % 7 == 0 ? 0 : 1 + rnd() % 40);
        }
        if (k) r[OFF[i % 3] + (size_t)(k - 1) * W + (i * 37) % W] = 9;
    }
}

static uint8_t stored(const uint8_t* rec, int record, int plane, int row, int col) { return rec[(size_t)record * RB + OFF[plane] + (size_t)row * W + col]; }

int main() {
    std::vector<int> want;
    std::vector<int32_t> all(N), kept(N);
    for (int i = 0; i < N; ++i) all[i] = i;
    for (int a = 0; a < 16; ++a) {
        uint8_t* heap = (uint8_t*)malloc((size_t)a + (size_t)N * RB);
        uint8_t* rec = heap + a;
        make_records(rec, want);
        CHECK(cl_store_extent_host(rec, (uint64_t)N * RB, RB, OFF, S, W, all.data(), N, kept.data()) == 0);
        uint64_t total = 0, largest = 0;
        for (int i = 0; i < N; ++i) {
            CHECK(kept[i] == want[i]);
            total += span(want[i]);
            if (span(want[i]) > largest) largest = span(want[i]);
        }
        const int32_t bad_slot[1] = {N};
        CHECK(cl_store_extent_host(rec, (uint64_t)N * RB, RB, OFF, S, W, bad_slot, 1, kept.data()) == -1);
        CHECK(cl_store_extent_host(rec, (uint64_t)N * RB - 1, RB, OFF, S, W, all.data(), N, kept.data()) == -1);   // the last record is cut
        for (int form = 0; form < 2; ++form) {
            // form 0: one slab of exactly the records' bytes; form 1: slabs of two of the largest records
            cl_store_t* st = nullptr;
            CHECK(cl_store_open(W, S, N, total, form ? 2 * largest : ((total + 15) & ~(uint64_t)15) + 16, -1, &st) == 0 && st);
            if (!st) return 1;
            // a first append one byte beyond the capacity is refused whole and leaves nothing behind
            if (form == 0) {
                cl_store_t* tight = nullptr;
                CHECK(cl_store_open(W, S, N, total - 1, 1 << 20, -1, &tight) == 0);
                CHECK(cl_store_pack_host(tight, rec, (uint64_t)N * RB, RB, OFF, all.data(), all.data(), N, kept.data()) == -3);
                cl_store_stats s{};
                CHECK(cl_store_get_stats(tight, &s) == 0 && s.records == 0 && s.slabs == 0);
                cl_store_close(tight);
            }
            CHECK(cl_store_pack_host(st, rec, (uint64_t)N * RB, RB, OFF, all.data(), all.data(), 10, kept.data()) == 0);
            CHECK(cl_store_pack_host(st, rec, (uint64_t)N * RB, RB, OFF, all.data() + 10, all.data() + 10, N - 10, kept.data() + 10) == 0);
            CHECK(cl_store_pack_host(st, rec, (uint64_t)N * RB, RB, OFF, all.data(), all.data(), 1, kept.data()) == -1);   // in the store already
            cl_store_stats s{};
            CHECK(cl_store_get_stats(st, &s) == 0 && s.records == N && (uint64_t)s.stored_bytes == total);
            CHECK(form ? s.slabs >= 3 : s.slabs == 1);
            for (int i = 0; i < N; ++i) {
                int32_t slab = -1, k = -1;
                int64_t off = -1, data_off = 0, used = 0, cap = 0;
                CHECK(cl_store_record(st, i, &slab, &off, &k) == 0 && k == want[i] && off % 16 == 0);
                CHECK(cl_store_slab(st, slab, nullptr, 0, &data_off, &used, &cap) == 0 && off + (int64_t)span(k) <= used && used <= cap);
                std::vector<uint8_t> bytes((size_t)cap);
                CHECK(cl_store_slab(st, slab, bytes.data(), (uint64_t)cap, &data_off, &used, &cap) == 0 && data_off == 0);
                bool same = true;
                for (int p = 0; p < 3 && same; ++p)
                    for (int o = 0; o < k * W && same; ++o) same = bytes[(size_t)off + (size_t)p * k * W + o] == stored(rec, i, p, o / W, o % W);
                for (uint64_t o = (uint64_t)3 * k * W; o < span(k) && same; ++o) same = bytes[(size_t)off + o] == 0;
                CHECK(same);
            }
            // sites: row lists over all stored rows (rows >= kept among them) and first-rows sites, every destination alignment
            int32_t sites[M];
            int16_t rows[M * R];
            uint8_t first[M];
            std::vector<uint8_t> line[3];
            for (int c = 0; c < 3; ++c) {
                line[c].resize((size_t)M * W);
                for (auto& x : line[c]) x = (uint8_t)rnd();
            }
            for (int d = 0; d < 16; ++d) {
                for (int i = 0; i < M; ++i) {
                    sites[i] = i < 6 ? i : (int32_t)(rnd() % N);
                    first[i] = (uint8_t)((i + d) % 2);
                    for (int r = 0; r < R; ++r) rows[i * R + r] = (int16_t)(rnd() % S);
                }
                for (int use = 0; use < 4; ++use) {
                    uint8_t* out_heap[6];
                    uint8_t* out[6];
                    for (int c = 0; c < 6; ++c) {
                        const size_t bytes = c < 3 ? (size_t)M * R * W : (size_t)M * W;
                        out_heap[c] = (uint8_t*)malloc((size_t)d + bytes);
                        out[c] = out_heap[c] + d;
                        memset(out_heap[c], 0xAB, (size_t)d + bytes);
                    }
                    CHECK(cl_store_assemble_host(st, sites, rows, first, M, R, line[0].data(), line[1].data(), line[2].data(), use & 1, use >> 1,
                                                 out[0], out[1], out[2], out[3], out[4], out[5], nullptr) == 0);
                    bool same = true;
                    for (int p = 0; p < 3 && same; ++p) {
                        const bool used = p == 0 || (p == 1 && (use & 1)) || (p == 2 && (use >> 1));
                        for (int i = 0; i < M && same; ++i)
                            for (int r = 0; r < R && same; ++r) {
                                const int row = first[i] ? r : rows[i * R + r];
                                for (int c = 0; c < W && same; ++c)
                                    same = out[p][((size_t)i * R + r) * W + c] == (used ? stored(rec, sites[i], p, row, c) : 0);
                            }
                    }
                    for (int c = 0; c < 3 && same; ++c) same = memcmp(out[3 + c], line[c].data(), (size_t)M * W) == 0;
                    for (int c = 0; c < 6 && same; ++c)
                        for (int o = 0; o < d && same; ++o) same = out_heap[c][o] == 0xAB;
                    CHECK(same);
                    for (int c = 0; c < 6; ++c) free(out_heap[c]);
                }
            }
            // refusals: nothing is written, the store goes on
            {
                std::vector<uint8_t> plane((size_t)M * R * W, 0xAB), small((size_t)M * W, 0xAB);
                uint8_t* o[6] = {plane.data(), plane.data(), plane.data(), small.data(), small.data(), small.data()};
                const int32_t keep = sites[3];
                const int16_t keep_row = rows[2 * R + 5];
                sites[3] = N;
                CHECK(cl_store_assemble_host(st, sites, rows, first, M, R, line[0].data(), line[1].data(), line[2].data(), 1, 1, o[0], o[1], o[2], o[3],
                                             o[4], o[5], nullptr) == -1);
                sites[3] = -1;
                CHECK(cl_store_assemble_host(st, sites, rows, first, M, R, line[0].data(), line[1].data(), line[2].data(), 1, 1, o[0], o[1], o[2], o[3],
                                             o[4], o[5], nullptr) == -1);
                sites[3] = keep;
                first[2] = 0;
                rows[2 * R + 5] = S;
                CHECK(cl_store_assemble_host(st, sites, rows, first, M, R, line[0].data(), line[1].data(), line[2].data(), 1, 1, o[0], o[1], o[2], o[3],
                                             o[4], o[5], nullptr) == -1);
                rows[2 * R + 5] = -1;
                CHECK(cl_store_assemble_host(st, sites, rows, first, M, R, line[0].data(), line[1].data(), line[2].data(), 1, 1, o[0], o[1], o[2], o[3],
                                             o[4], o[5], nullptr) == -1);
                CHECK(cl_store_last_error(st)[0] != 0);
                rows[2 * R + 5] = keep_row;
                bool untouched = true;
                for (uint8_t x : plane) untouched = untouched && x == 0xAB;
                CHECK(untouched);
                CHECK(cl_store_assemble_host(st, sites, rows, first, M, R, line[0].data(), line[1].data(), line[2].data(), 1, 1, o[0], o[1], o[2], o[3],
                                             o[4], o[5], nullptr) == 0);
            }
            cl_store_close(st);
        }
        free(heap);
    }
    printf("asan_store: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
