// Stand-alone driver of tools/asan_zdeflate.sh: runs zd_deflate_host (dl4vc_amd/csrc/zdeflate_capi.cpp built host-only, the text of
// zdeflate.h the GPU kernel runs) over the case grid of tests/zdeflate_cases.py -- the lengths around the match lengths and the
// segment boundaries, times zeros, one byte, a period of 3, incompressible bytes, pileup-like rows and a run that straddles a
// boundary -- into buffers of exactly zd_bound bytes (so the sanitizer sees any byte past the bound), and inflates every stream
// with zlib; every case in fixed and in dynamic codes (zd_deflate_host_flags), where the dynamic stream may not be the larger one.
// Then the code construction (zd_code_lengths_host): 0, 1, 2 and 286 used symbols, Fibonacci counts that the limit of 15 and of 7
// bits cuts, seeded random histograms -- lengths within the limit, Kraft sum 1.  Exit status 0 when every stream inflates to its
// input and every code is complete.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../include/dl4vc_pileup_gpu.h"

static uint32_t rng_state = 12345;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

static std::vector<uint8_t> content(int kind, size_t n, uint32_t seg) {
    std::vector<uint8_t> v(n, 0);
    switch (kind) {
    case 0: break;
    case 1: v.assign(n, 7); break;
    case 2: for (size_t i = 0; i < n; ++i) v[i] = "abc"[i % 3]; break;
    case 3: for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)(rnd() >> 11); break;
    case 4: {                                                     // rows of 201: tokens that repeat the row above, qualities, strands
        uint8_t ref[201];
        for (int i = 0; i < 201; ++i) ref[i] = 1 + rnd() % 4;
        for (size_t i = 0; i < n; ++i) {
            const size_t row = i / 201, col = i % 201, plane = (row / 16) % 3;
            const bool read = row % 16 < 9 && col >= (row * 7) % 100 && col < (row * 7) % 100 + 100;
            v[i] = !read ? 0 : plane == 0 ? ref[col] : plane == 1 ? 15 + rnd() % 26 : 1 + row % 2;
        }
        break;
    }
    default: {                                                    // random, a run of 5s from 100 before the first boundary to 100 after it
        for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)(rnd() >> 11);
        const size_t first = n < seg ? n : seg, lo = first > 100 ? first - 100 : 0;
        for (size_t i = lo; i < lo + 200 && i < n; ++i) v[i] = 5;
    }
    }
    return v;
}

// lengths within the limit and a Kraft sum of exactly 1 (two codes of length 1 where fewer than two symbols occur)
static bool code_ok(const std::vector<uint32_t>& freq, int limit) {
    std::vector<uint8_t> lens(freq.size() + 1, 0xEE);             // (the guard byte behind the lengths stays)
    if (zd_code_lengths_host(freq.data(), (int32_t)freq.size(), limit, lens.data()) || lens[freq.size()] != 0xEE) return false;
    uint64_t kraft = 0;
    size_t used = 0, coded = 0;
    for (size_t s = 0; s < freq.size(); ++s) {
        if (lens[s] > limit || (freq[s] && !lens[s])) return false;
        used += freq[s] != 0;
        coded += lens[s] != 0;
        if (lens[s]) kraft += 1ull << (limit - lens[s]);
    }
    return kraft == 1ull << limit && coded == (used < 2 ? 2 : used);
}

int main() {
    int bad = 0, cases = 0, codes = 0;
    for (uint32_t seg : {1024u, 4096u, 16384u, 32768u}) {
        const size_t lens[] = {0, 1, 2, 3, 4, 5, 257, 258, 259, seg - 1, seg, seg + 1, 3 * (size_t)seg + 1};
        for (size_t n : lens)
            for (int kind = 0; kind < 6; ++kind) {
                const std::vector<uint8_t> in = content(kind, n, seg);
                uint64_t bound = 0, size = 0;
                uint32_t adler = 0;
                int32_t store = 0;
                if (zd_bound(n, seg, &bound)) { ++bad; continue; }
                std::vector<uint8_t> out(bound);                  // exactly the bound: one byte more is a heap overflow
                uint64_t fixed_size = 0;
                for (int32_t flags : {0, ZD_DYNAMIC}) {
                    if ((flags ? zd_deflate_host_flags(n ? in.data() : nullptr, n, seg, flags, out.data(), bound, &size, &adler, &store)
                               : zd_deflate_host(n ? in.data() : nullptr, n, seg, out.data(), bound, &size, &adler, &store)) ||
                        size > bound || (flags && size > fixed_size)) {
                        fprintf(stderr, "segment %u, %zu bytes, kind %d, flags %d: zd_deflate_host failed or the dynamic stream is larger\n", seg,
                                n, kind, flags);
                        ++bad;
                        continue;
                    }
                    fixed_size = flags ? fixed_size : size;
                    std::vector<uint8_t> back(n + 1);
                    uLongf got = (uLongf)back.size();
                    const int rc = uncompress(back.data(), &got, out.data(), (uLong)size);
                    if (rc != Z_OK || got != n || (n && memcmp(back.data(), in.data(), n) != 0) || adler != (n ? adler32(1, in.data(), (uInt)n) : 1u) ||
                        (store != 0) != (size >= n)) {
                        fprintf(stderr, "segment %u, %zu bytes, kind %d: the stream does not inflate to its input (zlib %d)\n", seg, n, kind, rc);
                        ++bad;
                    }
                    ++cases;
                }
            }
    }
    // the code construction on its own
    for (int limit : {15, 7}) {
        const size_t n = limit == 15 ? 286 : 19;
        std::vector<uint32_t> f(n, 0);
        bad += !code_ok(f, limit); ++codes;                       // no symbol
        f[n - 1] = 9;
        bad += !code_ok(f, limit); ++codes;                       // one
        f[0] = 1;
        bad += !code_ok(f, limit); ++codes;                       // two
        for (size_t s = 0; s < n; ++s) f[s] = 1 + s % 7;
        bad += !code_ok(f, limit); ++codes;                       // all
        std::vector<uint32_t> fib(limit == 15 ? 20 : 12, 1);      // deeper than the limit without it
        for (size_t s = 2; s < fib.size(); ++s) fib[s] = fib[s - 1] + fib[s - 2];
        bad += !code_ok(fib, limit); ++codes;
        for (int k = 0; k < 200; ++k) {
            std::vector<uint32_t> r(2 + rnd() % (n - 1), 0);
            for (auto& x : r) x = rnd() % 4 ? (rnd() % 2 ? rnd() % 200 : 1u << (rnd() % 7)) : 0;
            bad += !code_ok(r, limit); ++codes;
        }
    }
    // refused arguments come back as error codes
    uint64_t b = 0;
    if (zd_bound(10, 100, &b) == 0 || zd_bound(10, 16384, nullptr) == 0) ++bad;
    printf("zd_deflate_host: %d cases, %d codes, %d failed\n", cases, codes, bad);
    return bad ? 1 : 0;
}
