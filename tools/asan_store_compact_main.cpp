// Stand-alone driver of tools/asan_store_compact.sh: runs the CPU twins of the compact record format (cl_store_spans_host /
// cl_store_spans_planes_host, cl_store_pack_host / cl_store_pack_planes_host on a store set to the compact format,
// cl_store_assemble_host of dl4vc_amd/csrc/store_capi.cpp built host-only) over records around the edges of a row's span at
// (S, W) = (5, 7), (3, 16) and (20, 201): no row; the only non-zero byte of a row at column 0, at column W - 1, in the quality
// plane only, in the strand plane only; an all-zero row between two used rows; zero cells inside a span; a row of all W columns;
// token 15 with strand 15; token 16 and strand 16 (both fall back to the rows layout); random spans in every row.  The records
// are read both as packed records (7 bytes | reads | 5 bytes | qual | strand, an odd size) and as three plane arrays, each in a
// heap buffer that ends where its data ends and starts 0..15 bytes into its allocation; the store's capacity is exactly the sum of
// the spans; every output plane ends where it ends.  The sanitizer sees any byte read or written past any of them.  Spans, stored
// bytes and assembled planes are compared with plain loops over the untrimmed planes.  Exit status 0 when everything agrees.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../include/dl4vc_chunks.h"

static const int N = 13;

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

struct Planes {
    int S, W;
    std::vector<uint8_t> p[3];                       // [N][S][W]
    uint8_t& at(int plane, int rec, int row, int col) { return p[plane][((size_t)rec * S + row) * W + col]; }
};

static Planes make_planes(int S, int W) {
    Planes x{S, W, {}};
    for (auto& v : x.p) v.assign((size_t)N * S * W, 0);
    x.at(0, 1, 0, 0) = 3;
    x.at(0, 2, 1, W - 1) = 4;
    x.at(1, 3, 0, W / 2) = 40;
    x.at(2, 4, S / 2, 1) = 2;
    for (int c = 1; c < W - 1; ++c) {
        x.at(0, 5, 0, c) = (uint8_t)(1 + rnd() % 8); x.at(1, 5, 2, c) = (uint8_t)(1 + rnd() % 40);
    }
    x.at(0, 6, 0, 0) = 5; x.at(1, 6, 0, W - 1) = 17;
    for (int c = 0; c < W; ++c)
        for (int p = 0; p < 3; ++p) x.at(p, 7, 1, c) = (uint8_t)(1 + rnd() % 2);
    x.at(0, 8, 0, 1) = 15; x.at(2, 8, 0, 1) = 15; x.at(1, 8, 0, 1) = 255;
    x.at(0, 9, 0, 1) = 16; x.at(0, 9, 1, 0) = 7;
    x.at(2, 10, 1, W - 1) = 16; x.at(0, 10, 0, 0) = 2;
    for (int rec = 11; rec < N; ++rec)
        for (int r = 0; r < S; ++r) {
            const int c0 = (int)(rnd() % (W - 1)), n = 1 + (int)(rnd() % (W - c0));
            for (int c = c0; c < c0 + n; ++c) {
                x.at(0, rec, r, c) = (uint8_t)(rnd() % 16); x.at(2, rec, r, c) = (uint8_t)(rnd() % 16); x.at(1, rec, r, c) = (uint8_t)rnd();
            }
            x.at(0, rec, r, c0) = 1; x.at(1, rec, r, c0 + n - 1) = 9;
            if (rec == 12 && r % 2) for (int c = 0; c < W; ++c) for (int p = 0; p < 3; ++p) x.at(p, rec, r, c) = 0;   // every other row empty
        }
    return x;
}

// the definition by plain loops: spans of record rec -> kept, cells, mergeable
static void define(Planes& x, int rec, std::vector<int>& c0, std::vector<int>& n, int& kept, int& cells, int& mergeable) {
    c0.assign(x.S, 0); n.assign(x.S, 0);
    kept = cells = 0; mergeable = 1;
    for (int r = 0; r < x.S; ++r) {
        int lo = -1, hi = -1;
        for (int c = 0; c < x.W; ++c) {
            if (x.at(0, rec, r, c) | x.at(1, rec, r, c) | x.at(2, rec, r, c)) { if (lo < 0) lo = c; hi = c; }
            if (x.at(0, rec, r, c) >= 16 || x.at(2, rec, r, c) >= 16) mergeable = 0;
        }
        if (lo >= 0) { c0[r] = lo; n[r] = hi - lo + 1; kept = r + 1; cells += n[r]; }
    }
}

static uint64_t pad16(uint64_t b) { return (b + 15) & ~(uint64_t)15; }

static void run(int S, int W, int R, int align, bool as_records) {
    Planes x = make_planes(S, W);
    const int64_t sw = (int64_t)S * W, OFF[3] = {7, 7 + sw + 5, 7 + 2 * sw + 5}, RB = OFF[2] + sw + (sw % 2 ? 0 : 1) + 2;
    uint8_t* heap[3] = {nullptr, nullptr, nullptr};
    const uint8_t* src[3];
    if (as_records) {                               // one buffer of N packed records that ends where the last one ends
        heap[0] = (uint8_t*)malloc((size_t)align + (size_t)N * RB);
        memset(heap[0], 0xEE, (size_t)align + (size_t)N * RB);
        for (int i = 0; i < N; ++i)
            for (int p = 0; p < 3; ++p) memcpy(heap[0] + align + (size_t)i * RB + OFF[p], &x.p[p][(size_t)i * sw], (size_t)sw);
        src[0] = heap[0] + align;
    } else {
        for (int p = 0; p < 3; ++p) {
            heap[p] = (uint8_t*)malloc((size_t)align + (size_t)N * sw);
            memcpy(heap[p] + align, x.p[p].data(), (size_t)N * sw);
            src[p] = heap[p] + align;
        }
    }
    std::vector<int32_t> all(N), kept(N), cells(N), merge(N);
    std::vector<uint16_t> rowspans((size_t)N * S);
    for (int i = 0; i < N; ++i) all[i] = i;
    if (as_records) CHECK(cl_store_spans_host(src[0], (uint64_t)N * RB, RB, OFF, S, W, all.data(), N, kept.data(), cells.data(), merge.data(), rowspans.data()) == 0);
    else CHECK(cl_store_spans_planes_host(src[0], src[1], src[2], N, S, W, all.data(), N, kept.data(), cells.data(), merge.data(), rowspans.data()) == 0);
    std::vector<std::vector<int>> c0(N), n(N);
    std::vector<uint64_t> span(N);
    uint64_t total = 0, largest = 0;
    for (int i = 0; i < N; ++i) {
        int k, c, m;
        define(x, i, c0[i], n[i], k, c, m);
        CHECK(kept[i] == k && cells[i] == c && merge[i] == m);
        CHECK(m == (i != 9 && i != 10));
        for (int r = 0; r < S; ++r) CHECK(rowspans[(size_t)i * S + r] == (uint16_t)(c0[i][r] | n[i][r] << 8));
        span[i] = m ? (k ? pad16(4 * ((uint64_t)k + 1) + 2 * (uint64_t)c) : 0) : pad16((uint64_t)3 * k * W);
        total += span[i];
        if (span[i] > largest) largest = span[i];
    }
    for (int form = 0; form < 2; ++form) {
        // form 0: one slab, the capacity exactly the records' bytes; form 1: slabs of two of the largest records
        cl_store_t* st = nullptr;
        CHECK(cl_store_open(W, S, N, total, form ? 2 * largest : pad16(total) + 16, -1, &st) == 0 && st);
        if (!st) exit(1);
        CHECK(cl_store_set_format(st, 2) == -1 && cl_store_set_format(st, 1) == 0);
        CHECK(cl_store_debug_fill(st, 0xAB) == 0);
        if (form == 0) {                            // one byte short: refused whole, nothing left behind
            cl_store_t* tight = nullptr;
            CHECK(cl_store_open(W, S, N, total - 1, 1 << 20, -1, &tight) == 0 && cl_store_set_format(tight, 1) == 0);
            const int rc = as_records ? cl_store_pack_host(tight, src[0], (uint64_t)N * RB, RB, OFF, all.data(), all.data(), N, kept.data())
                                      : cl_store_pack_planes_host(tight, src[0], src[1], src[2], N, all.data(), all.data(), N, kept.data());
            cl_store_stats s{};
            CHECK(rc == -3 && cl_store_get_stats(tight, &s) == 0 && s.records == 0 && s.slabs == 0);
            cl_store_close(tight);
        }
        for (int part = 0; part < 2; ++part) {      // two appends
            const int a = part ? 6 : 0, m = part ? N - 6 : 6;
            const int rc = as_records ? cl_store_pack_host(st, src[0], (uint64_t)N * RB, RB, OFF, all.data() + a, all.data() + a, m, kept.data() + a)
                                      : cl_store_pack_planes_host(st, src[0], src[1], src[2], N, all.data() + a, all.data() + a, m, kept.data() + a);
            CHECK(rc == 0);
        }
        CHECK(cl_store_set_format(st, 0) == -1);    // after an append
        cl_store_stats s{};
        cl_store_format_stats f{};
        CHECK(cl_store_get_stats(st, &s) == 0 && s.records == N && (uint64_t)s.stored_bytes == total);
        CHECK(cl_store_get_format_stats(st, &f) == 0 && f.format == 1 && f.rows_records == 2 && f.compact_records == N - 2);
        CHECK((uint64_t)(f.rows_bytes + f.compact_bytes) == total);
        for (int i = 0; i < N; ++i) {
            int32_t slab = -1, k = -1, fmt = -1;
            int64_t off = -1, bytes = -1, data_off = 0, used = 0, cap = 0;
            CHECK(cl_store_record(st, i, &slab, &off, &k) == 0 && k == kept[i] && off % 16 == 0);
            CHECK(cl_store_record_span(st, i, &fmt, &bytes) == 0 && fmt == merge[i] && (uint64_t)bytes == span[i]);
            CHECK(cl_store_slab(st, slab, nullptr, 0, &data_off, &used, &cap) == 0 && off + bytes <= used && used <= cap);
            std::vector<uint8_t> b((size_t)cap);
            CHECK(cl_store_slab(st, slab, b.data(), (uint64_t)cap, &data_off, &used, &cap) == 0 && data_off == 0);
            const uint8_t* rec = b.data() + off;
            bool same = true;
            if (!merge[i]) {
                for (int p = 0; p < 3 && same; ++p)
                    for (int o = 0; o < k * W && same; ++o) same = rec[(size_t)p * k * W + o] == x.at(p, i, o / W, o % W);
            } else if (k) {
                uint32_t o = 0;
                const uint8_t* ts = rec + 4 * ((size_t)k + 1);
                const uint8_t* q = ts + cells[i];
                for (int r = 0; r <= k && same; ++r) {
                    const uint32_t e = (uint32_t)rec[4 * r] | (uint32_t)rec[4 * r + 1] << 8 | (uint32_t)rec[4 * r + 2] << 16 | (uint32_t)rec[4 * r + 3] << 24;
                    same = e == (o | (uint32_t)(r < k ? c0[i][r] : 0) << 24);
                    for (int j = 0; r < k && j < n[i][r] && same; ++j, ++o)
                        same = ts[o] == (uint8_t)(x.at(0, i, r, c0[i][r] + j) | x.at(2, i, r, c0[i][r] + j) << 4) && q[o] == x.at(1, i, r, c0[i][r] + j);
                }
                for (uint64_t z = 4 * ((uint64_t)k + 1) + 2 * (uint64_t)cells[i]; z < span[i] && same; ++z) same = rec[z] == 0;
            }
            CHECK(same);
            for (int64_t z = used; z < cap; ++z) CHECK(b[(size_t)z] == 0xAB);
        }
        // sites: row lists over all stored rows (rows >= kept among them) and first-rows sites, every destination alignment
        const int M = 9;
        std::vector<int32_t> sites(M);
        std::vector<int16_t> rows((size_t)M * R);
        std::vector<uint8_t> first(M), line[3];
        for (int c = 0; c < 3; ++c) {
            line[c].resize((size_t)M * W);
            for (auto& v : line[c]) v = (uint8_t)rnd();
        }
        for (int d = 0; d < 16; ++d) {
            for (int i = 0; i < M; ++i) {
                sites[i] = (int32_t)((i * 3 + d) % N);
                first[i] = (uint8_t)((i + d) % 2);
                for (int r = 0; r < R; ++r) rows[(size_t)i * R + r] = (int16_t)(rnd() % S);
            }
            for (int use = 0; use < 4; ++use) {
                uint8_t *out_heap[6], *out[6];
                for (int c = 0; c < 6; ++c) {
                    const size_t bytes = c < 3 ? (size_t)M * R * W : (size_t)M * W;
                    out_heap[c] = (uint8_t*)malloc((size_t)d + bytes);
                    out[c] = out_heap[c] + d;
                    memset(out_heap[c], 0xAB, (size_t)d + bytes);
                }
                CHECK(cl_store_assemble_host(st, sites.data(), rows.data(), first.data(), M, R, line[0].data(), line[1].data(), line[2].data(),
                                             use & 1, use >> 1, out[0], out[1], out[2], out[3], out[4], out[5], nullptr) == 0);
                bool same = true;
                for (int p = 0; p < 3 && same; ++p) {
                    const bool used = p == 0 || (p == 1 && (use & 1)) || (p == 2 && (use >> 1));
                    for (int i = 0; i < M && same; ++i)
                        for (int r = 0; r < R && same; ++r) {
                            const int row = first[i] ? r : rows[(size_t)i * R + r];
                            for (int c = 0; c < W && same; ++c) same = out[p][((size_t)i * R + r) * W + c] == (used ? x.at(p, sites[i], row, c) : 0);
                        }
                }
                for (int c = 0; c < 3 && same; ++c) same = memcmp(out[3 + c], line[c].data(), (size_t)M * W) == 0;
                for (int c = 0; c < 6 && same; ++c)
                    for (int o = 0; o < d && same; ++o) same = out_heap[c][o] == 0xAB;
                CHECK(same);
                for (int c = 0; c < 6; ++c) free(out_heap[c]);
            }
        }
        cl_store_close(st);
    }
    for (int p = 0; p < 3; ++p) free(heap[p]);
}

int main() {
    static const int shapes[3][3] = {{5, 7, 4}, {3, 16, 3}, {20, 201, 12}};     // S, W, rows read
    for (const auto& s : shapes)
        for (int align = 0; align < 16; ++align)
            for (int as_records = 0; as_records < 2; ++as_records) run(s[0], s[1], s[2], align, as_records != 0);
    cl_store_t* wide = nullptr;
    CHECK(cl_store_open(256, 4, 2, 1 << 20, 1 << 16, -1, &wide) == 0 && cl_store_set_format(wide, 1) == -1 && cl_store_last_error(wide)[0] != 0);
    cl_store_close(wide);
    CHECK(cl_store_open(255, 4, 2, 1 << 20, 1 << 16, -1, &wide) == 0 && cl_store_set_format(wide, 1) == 0);
    cl_store_close(wide);
    printf("asan_store_compact: %s (%d failures)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
