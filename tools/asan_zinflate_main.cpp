// Stand-alone driver of tools/asan_zinflate.sh: runs zi_inflate_host (dl4vc_amd/csrc/zinflate_capi.cpp built host-only: the text of
// zinflate.h the GPU kernel runs, ring included, with one lane) over the grid of tests/zinflate_cases.py -- the lengths around
// the ring's half and whole sizes up to a production chunk of 991 720 bytes, times zeros, one byte, a period of 3, a period of
// 32 768, incompressible bytes and pileup-like rows, compressed by zlib at levels 0 / 1 / 4 / 9 and by zd_deflate_host in fixed
// and dynamic codes, at the slot alignments 0..15 -- then streams assembled by hand (a stored block of 65 535 bytes from 100
// before a half boundary, a 258-byte match across a half boundary and across the ring's wrap, distance-32 768 matches whose
// source begins at ring offset 0) and the damaged streams.  Every stream sits in a heap buffer of exactly its size and every
// slot ends where its heap buffer ends (it starts `alignment` bytes in; those bytes keep their 0xAB), so the sanitizer sees any
// byte read or written past either.  Exit status 0 when every good stream gives its input and every damaged one a status.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include <string>
#include <vector>

#include "../include/dl4vc_chunks.h"
#include "../include/dl4vc_pileup_gpu.h"

typedef std::vector<uint8_t> Bytes;
static const uint32_t HALF = 32768, RING = 65536;

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

static Bytes content(int kind, size_t n) {
    Bytes v(n, 0);
    switch (kind) {
    case 0: break;
    case 1: v.assign(n, 7); break;
    case 2: for (size_t i = 0; i < n; ++i) v[i] = "abc"[i % 3]; break;
    case 3: {
        Bytes p(HALF);
        for (auto& x : p) x = (uint8_t)(rnd() >> 11);
        for (size_t i = 0; i < n; ++i) v[i] = p[i % HALF];
        break;
    }
    case 4: for (size_t i = 0; i < n; ++i) v[i] = (uint8_t)(rnd() >> 11); break;
    default: {                                                    // rows of 201: tokens that repeat the row above, qualities, strands
        uint8_t ref[201];
        for (int i = 0; i < 201; ++i) ref[i] = 1 + rnd() % 4;
        for (size_t i = 0; i < n; ++i) {
            const size_t row = i / 201, col = i % 201, plane = (row / 16) % 3;
            const bool read = row % 16 < 9 && col >= (row * 7) % 100 && col < (row * 7) % 100 + 100;
            v[i] = !read ? 0 : plane == 0 ? ref[col] : plane == 1 ? 15 + rnd() % 26 : 1 + row % 2;
        }
    }
    }
    return v;
}

// compressor 0..3: zlib at level 0 / 1 / 4 / 9; 4 / 5: zd_deflate_host in fixed / dynamic codes
static bool compress_with(int z, const Bytes& in, Bytes& out) {
    if (z < 4) {
        static const int level[4] = {0, 1, 4, 9};
        uLongf got = compressBound((uLong)in.size());
        out.resize(got);
        if (compress2(out.data(), &got, in.data(), (uLong)in.size(), level[z]) != Z_OK) return false;
        out.resize(got);
        return true;
    }
    uint64_t bound = 0, size = 0;
    uint32_t adler = 0;
    int32_t store = 0;
    if (zd_bound(in.size(), 16384, &bound)) return false;
    out.resize(bound);
    if (zd_deflate_host_flags(in.size() ? in.data() : nullptr, in.size(), 16384, z == 5 ? ZD_DYNAMIC : 0, out.data(), bound, &size, &adler, &store))
        return false;
    out.resize(size);
    return true;
}

// One stream through zi_inflate_host: the stream in a heap buffer of exactly its size, the slot at the end of a heap buffer of
// align + out_len bytes.  -> the status; *same: the slot equals want (when given) and the bytes in front of it kept 0xAB.
static int run_one(const Bytes& stream, uint64_t out_len, int align, int raw, const Bytes* want, bool* intact) {
    uint8_t* in = new uint8_t[stream.size()];                     // (operator new of 0 bytes is a valid, zero-sized block)
    if (!stream.empty()) memcpy(in, stream.data(), stream.size());
    uint8_t* out = new uint8_t[align + out_len];
    memset(out, 0xAB, align + out_len);
    const uint64_t off = 0, len = stream.size(), out_off = (uint64_t)align;
    const uint8_t r = (uint8_t)raw;
    int32_t status = -1;
    const int rc = zi_inflate_host(in, len, &off, &len, 1, out, align + out_len, &out_off, &out_len, &r, &status);
    *intact = rc == 0;
    for (int i = 0; i < align; ++i) *intact = *intact && out[i] == 0xAB;
    if (want && status == 0) *intact = *intact && want->size() == out_len && (out_len == 0 || memcmp(out + align, want->data(), out_len) == 0);
    delete[] in;
    delete[] out;
    return rc ? -1 : status;
}

// ---- a DEFLATE body written block by block (RFC 1951): stored blocks, fixed-Huffman literals and matches ------------------
struct Deflate {
    Bytes out;
    uint64_t acc = 0;
    int cnt = 0;
    void bits(uint32_t v, int n) {
        acc |= (uint64_t)v << cnt;
        cnt += n;
        while (cnt >= 8) { out.push_back((uint8_t)acc); acc >>= 8; cnt -= 8; }
    }
    void code(uint32_t v, int n) { for (int i = n - 1; i >= 0; --i) bits((v >> i) & 1, 1); }
    void align() { if (cnt) bits(0, 8 - cnt); }
    void stored(const uint8_t* p, uint32_t n, bool final) {
        bits(final ? 1 : 0, 1); bits(0, 2); align();
        out.push_back((uint8_t)n); out.push_back((uint8_t)(n >> 8)); out.push_back((uint8_t)~n); out.push_back((uint8_t)(~n >> 8));
        out.insert(out.end(), p, p + n);
    }
    void fixed(bool final) { bits(final ? 1 : 0, 1); bits(1, 2); }
    void btype3() { bits(1, 1); bits(3, 2); }
    void symbol(uint32_t s) {
        if (s < 144) code(0x30 + s, 8);
        else if (s < 256) code(0x190 + s - 144, 9);
        else if (s < 280) code(s - 256, 7);
        else code(0xC0 + s - 280, 8);
    }
    void match258(uint32_t dist) {                                // length 258 = symbol 285, no extra bits
        static const uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
        static const uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
        symbol(285);
        int j = 29;
        while (DBASE[j] > dist) --j;
        code((uint32_t)j, 5);
        bits(dist - DBASE[j], DEXT[j]);
    }
    // the zlib stream; *data = what zlib inflates the body to (empty when zlib refuses it)
    Bytes stream(Bytes* data, size_t expect) {
        align();
        data->assign(expect, 0);
        z_stream zs;
        memset(&zs, 0, sizeof zs);
        uLong ad = 1;
        if (inflateInit2(&zs, -15) == Z_OK) {
            zs.next_in = out.data(); zs.avail_in = (uInt)out.size();
            zs.next_out = data->data(); zs.avail_out = (uInt)expect;
            const int rc = inflate(&zs, Z_FINISH);
            if (rc != Z_STREAM_END || zs.total_out != expect) data->clear();
            inflateEnd(&zs);
        }
        if (!data->empty()) ad = adler32(1, data->data(), (uInt)data->size());
        Bytes s = {0x78, 0x01};
        s.insert(s.end(), out.begin(), out.end());
        for (int b = 3; b >= 0; --b) s.push_back((uint8_t)(ad >> (8 * b)));
        return s;
    }
};

static int bad = 0, cases = 0, damaged = 0;

static void good_case(const char* what, const Bytes& stream, const Bytes& data, int align, int raw = 0) {
    bool intact = false;
    const int st = run_one(stream, data.size(), align, raw, &data, &intact);
    if (st != 0 || !intact) {
        fprintf(stderr, "%s (%zu bytes, alignment %d): status %d (%s)%s\n", what, data.size(), align, st, zi_status_text(st),
                intact ? "" : ", wrong bytes");
        ++bad;
    }
    ++cases;
}

static void bad_case(const char* what, const Bytes& stream, uint64_t out_len, int raw = 0) {
    bool intact = false;
    const int st = run_one(stream, out_len, 7, raw, nullptr, &intact);
    if (st <= 0 || !intact) {
        fprintf(stderr, "damaged: %s: status %d%s\n", what, st, intact ? "" : ", bytes in front of the slot changed");
        ++bad;
    }
    ++damaged;
}

int main() {
    const size_t lens[] = {0, 1, HALF - 1, HALF, HALF + 1, RING - 1, RING, RING + 1, 3 * (size_t)RING + 1, 123400, 991720};
    int turn = 0;
    for (size_t n : lens) {
        for (int kind = 0; kind < 6; ++kind, ++turn) {
            const Bytes in = content(kind, n);
            Bytes s;
            if (!compress_with(turn % 6, in, s)) { fprintf(stderr, "compressor %d failed on %zu bytes\n", turn % 6, n); ++bad; continue; }
            good_case("grid", s, in, (turn * 7) % 16);
        }
        ++turn;
    }
    for (int kind = 0; kind < 6; ++kind)                          // every content x every compressor just past one turn of the ring
        for (int z = 0; z < 6; ++z) {
            const Bytes in = content(kind, RING + 1);
            Bytes s;
            if (!compress_with(z, in, s)) { ++bad; continue; }
            good_case("content x compressor", s, in, (3 * kind + z) % 16);
        }
    const Bytes pile = content(5, HALF + 1), rnd_bytes = content(4, 4 * HALF);
    for (int a = 0; a < 16; ++a) {                                // every alignment across the first half boundary
        Bytes s;
        if (!compress_with(a % 6, pile, s)) { ++bad; continue; }
        good_case("alignment", s, pile, a);
    }
    good_case("raw chunk", pile, pile, 9, 1);
    good_case("raw chunk of no bytes", Bytes(), Bytes(), 3, 1);
    // assembled by hand
    Bytes data;
    {
        Deflate d;
        d.stored(rnd_bytes.data(), HALF - 100, false);
        d.stored(rnd_bytes.data() + HALF, 65535, true);
        const Bytes s = d.stream(&data, HALF - 100 + 65535);
        good_case("stored block of 65535 from 100 before a half boundary", s, data, 5);
    }
    for (int wrap = 0; wrap < 2; ++wrap) {
        Deflate d;
        d.stored(rnd_bytes.data(), HALF - 100, false);
        if (wrap) d.stored(rnd_bytes.data() + HALF, HALF, false);
        d.fixed(true);
        d.match258(1000);
        for (const char* p = "tail"; *p; ++p) d.symbol((uint8_t)*p);
        d.match258(3);                                            // (an overlapping match right behind the seam)
        d.symbol(256);
        const Bytes s = d.stream(&data, HALF - 100 + (wrap ? HALF : 0) + 258 + 4 + 258);
        good_case(wrap ? "match of 258 across the ring's wrap" : "match of 258 across the first half boundary", s, data, 11);
    }
    {
        Deflate d;
        d.stored(rnd_bytes.data(), HALF, false);
        d.fixed(false);
        d.match258(HALF);                                         // source [0, 258): ring offset 0 at alignment 0
        d.symbol(256);
        d.stored(rnd_bytes.data() + HALF, 3 * HALF - (HALF + 258), false);
        d.fixed(true);
        d.match258(HALF);                                         // source [65 536, 65 794): ring offset 0 again
        d.match258(HALF);
        d.symbol(256);
        const Bytes s = d.stream(&data, 3 * HALF + 516);
        good_case("distance 32768 from ring offset 0", s, data, 0);
    }
    // damaged
    const Bytes src = content(5, 100000);
    Bytes good;
    if (!compress_with(2, src, good)) ++bad;
    Bytes s = good; s[0] = 0x79; s[1] = (uint8_t)(31 - 0x7900 % 31); bad_case("CM 9", s, src.size());
    s = good; s[0] = 0x88; s[1] = (uint8_t)(31 - 0x8800 % 31); bad_case("CINFO 8", s, src.size());
    s = good; s[1] ^= 1; bad_case("bad FCHECK", s, src.size());
    s = good; s[1] = (uint8_t)(0x20 + 31 - 0x7820 % 31); bad_case("FDICT set", s, src.size());
    s = good; s[s.size() - 2] ^= 0x10; bad_case("flipped Adler byte", s, src.size());
    for (size_t k : {(size_t)0, (size_t)1, (size_t)2, (size_t)5, good.size() / 2}) bad_case("truncated", Bytes(good.begin(), good.begin() + k), src.size());
    s = good; s.push_back(0); bad_case("1 trailing byte", s, src.size());
    bad_case("expected length one more", good, src.size() + 1);
    bad_case("expected length one less", good, src.size() - 1);
    {
        Deflate d;
        d.fixed(true); d.symbol('a'); d.match258(5); d.symbol(256);
        bad_case("distance before the start", d.stream(&data, 259), 259);
    }
    {
        Deflate d;
        d.stored(src.data(), 40000, false);
        d.btype3();
        bad_case("BTYPE 3 after a flushed half", d.stream(&data, 40000), 40000);
    }
    {
        Deflate d;
        d.btype3();
        bad_case("BTYPE 3", d.stream(&data, 0), 0);
    }
    bad_case("raw chunk one byte short", Bytes(src.begin(), src.begin() + 999), 1000, 1);
    bad_case("raw chunk one byte long", Bytes(src.begin(), src.begin() + 1001), 1000, 1);
    // every prefix of a small stream and every single flipped bit of its first 64 bytes: a status or the right bytes, never a fault
    {
        const Bytes small = content(5, 3000);
        Bytes z;
        if (!compress_with(3, small, z)) ++bad;
        bool intact;
        for (size_t k = 0; k < z.size(); ++k) { if (run_one(Bytes(z.begin(), z.begin() + k), small.size(), 1, 0, nullptr, &intact) == 0 || !intact) ++bad; }
        for (size_t bit = 0; bit < 8 * 64 && bit < 8 * z.size(); ++bit) {
            Bytes f = z;
            f[bit / 8] ^= (uint8_t)(1 << (bit % 8));
            const int st = run_one(f, small.size(), 2, 0, &small, &intact);   // (status 0 only with the right bytes)
            if (st < 0 || !intact) ++bad;
        }
    }
    // refused arguments come back as error codes
    const uint64_t zero = 0;
    int32_t st = 0;
    if (zi_inflate_host(nullptr, 0, nullptr, nullptr, 1, nullptr, 0, &zero, &zero, nullptr, &st) == 0 || zi_inflate_host(nullptr, 0, nullptr, nullptr, -1, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0)
        ++bad;
    printf("zi_inflate_host: %d streams, %d damaged, %d failed\n", cases, damaged, bad);
    return bad ? 1 : 0;
}
