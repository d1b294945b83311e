// Stand-alone driver of tools/asan_store_planes.sh: runs the planar CPU definitions of the record store
// (cl_store_extent_planes_host, cl_store_pack_planes_host of dl4vc_amd/csrc/store_capi.cpp built host-only) on three plane arrays
// [N][S][W] at (S, W) = (5, 7), (3, 16) and (200, 201).  Each array sits in a heap buffer of its own that ends where the array
// ends and starts 0..15 bytes into its allocation, so the sanitizer sees any byte read in front of or behind a plane; the slabs
// are as large as the records need.  Extents and stored bytes are compared with plain loops, and with cl_store_pack_host on the
// same slots laid out as packed records; the refusals (a slot >= n_slots, the budget one byte short) must leave the store as it
// was.  Exit status 0 when everything agrees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dl4vc_chunks.h"

static uint32_t rng_state = 88172645u;
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

static const int N = 11;

static int run(int S, int W, int a) {
    const size_t sw = (size_t)S * W;
    uint8_t* heap[3];
    uint8_t* plane[3];
    for (int p = 0; p < 3; ++p) {
        heap[p] = (uint8_t*)malloc((size_t)((a + 5 * p) % 16) + N * sw);
        plane[p] = heap[p] + (a + 5 * p) % 16;
        memset(plane[p], 0, N * sw);
    }
    // slot 0: nothing; slot 1: the last byte of the strand plane alone; slot 2 / 3: the last byte at the start / end of a row
    std::vector<int> want(N, 0);
    plane[2][1 * sw + sw - 1] = 7;
    want[1] = S;
    for (int i = 2; i < N; ++i) {
        const int k = i < 4 ? (S + 1) / 2 : 1 + (int)(rnd() % S);
        for (int p = 0; p < 3; ++p)
            for (size_t o = 0; o + W < (size_t)k * W + 1 && k > 1; ++o) plane[p][i * sw + o] = (uint8_t)(rnd() % 5 == 0 ? 0 : 1 + rnd() % 40);
        plane[i % 3][i * sw + (size_t)(k - 1) * W + (i == 2 ? 0 : i == 3 ? W - 1 : (int)(rnd() % W))] = 9;
        want[i] = k;
    }
    // the same slots as packed records of an odd size
    const int64_t off[3] = {3, 3 + (int64_t)sw + 6, 3 + 2 * (int64_t)sw + 6};
    const int64_t rb = off[2] + (int64_t)sw + (sw % 2 ? 1 : 2);   // odd: the packed planes start at every alignment
    std::vector<uint8_t> rec((size_t)N * rb, 0xEE);
    for (int i = 0; i < N; ++i)
        for (int p = 0; p < 3; ++p) memcpy(rec.data() + (size_t)i * rb + off[p], plane[p] + i * sw, sw);
    const int32_t slots[8] = {9, 2, 0, 10, 5, 1, 3, 7};        // out of order, with gaps
    int32_t records[8], kept[8], kept2[8];
    uint64_t total = 0, largest = 0;
    for (int i = 0; i < 8; ++i) {
        records[i] = i;
        const uint64_t b = ((uint64_t)3 * want[slots[i]] * W + 15) & ~(uint64_t)15;
        total += b;
        if (b > largest) largest = b;
    }
    CHECK(cl_store_extent_planes_host(plane[0], plane[1], plane[2], N, S, W, slots, 8, kept) == 0);
    for (int i = 0; i < 8; ++i) CHECK(kept[i] == want[slots[i]]);
    const int32_t bad[1] = {N};
    CHECK(cl_store_extent_planes_host(plane[0], plane[1], plane[2], N, S, W, bad, 1, kept) == -1);
    cl_store_t *st = nullptr, *twin = nullptr, *tight = nullptr;
    CHECK(cl_store_open(W, S, 8, total, 2 * largest, -1, &st) == 0 && st);
    CHECK(cl_store_open(W, S, 8, total, 2 * largest, -1, &twin) == 0 && twin);
    CHECK(cl_store_open(W, S, 8, total - 1, 2 * largest, -1, &tight) == 0 && tight);
    if (!st || !twin || !tight) return 1;
    cl_store_stats s{};
    CHECK(cl_store_pack_planes_host(tight, plane[0], plane[1], plane[2], N, slots, records, 8, kept) == -3);
    CHECK(cl_store_get_stats(tight, &s) == 0 && s.records == 0 && s.slabs == 0);
    CHECK(cl_store_pack_planes_host(st, plane[0], plane[1], plane[2], N, bad, records, 1, kept) == -1);
    CHECK(cl_store_get_stats(st, &s) == 0 && s.records == 0 && s.slabs == 0);
    CHECK(cl_store_pack_planes_host(st, plane[0], plane[1], plane[2], N, slots, records, 5, kept) == 0);
    CHECK(cl_store_pack_planes_host(st, plane[0], plane[1], plane[2], N, slots + 5, records + 5, 3, kept + 5) == 0);
    CHECK(cl_store_pack_host(twin, rec.data(), (uint64_t)N * rb, rb, off, slots, records, 8, kept2) == 0);
    CHECK(cl_store_get_stats(st, &s) == 0 && s.records == 8 && (uint64_t)s.stored_bytes == total);
    cl_store_stats s2{};
    CHECK(cl_store_get_stats(twin, &s2) == 0 && s2.slabs == s.slabs && s2.stored_bytes == s.stored_bytes);
    for (int i = 0; i < 8; ++i) {
        int32_t slab = -1, k = -1, slab2 = -1, k2 = -1;
        int64_t o = -1, o2 = -1, data_off = 0, used = 0, cap = 0, used2 = 0, cap2 = 0;
        CHECK(cl_store_record(st, i, &slab, &o, &k) == 0 && k == want[slots[i]] && kept[i] == k);
        CHECK(cl_store_record(twin, i, &slab2, &o2, &k2) == 0 && slab2 == slab && o2 == o && k2 == k);
        CHECK(cl_store_slab(st, slab, nullptr, 0, &data_off, &used, &cap) == 0);
        std::vector<uint8_t> bytes((size_t)cap), bytes2((size_t)cap);
        CHECK(cl_store_slab(st, slab, bytes.data(), (uint64_t)cap, &data_off, &used, &cap) == 0);
        CHECK(cl_store_slab(twin, slab, bytes2.data(), (uint64_t)cap, &data_off, &used2, &cap2) == 0 && used2 == used && cap2 == cap);
        CHECK(memcmp(bytes.data(), bytes2.data(), (size_t)used) == 0);
        bool same = true;
        for (int p = 0; p < 3 && same; ++p)
            for (size_t x = 0; x < (size_t)k * W && same; ++x) same = bytes[(size_t)o + (size_t)p * k * W + x] == plane[p][slots[i] * sw + x];
        CHECK(same);
    }
    cl_store_close(st);
    cl_store_close(twin);
    cl_store_close(tight);
    for (int p = 0; p < 3; ++p) free(heap[p]);
    return 0;
}

int main() {
    const int shapes[3][2] = {{5, 7}, {3, 16}, {200, 201}};
    for (const auto& sh : shapes)
        for (int a = 0; a < 16; ++a)
            if (run(sh[0], sh[1], a)) return 1;
    printf("asan_store_planes: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
