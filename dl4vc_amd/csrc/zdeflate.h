// The encode core of the zlib compressor (the twin of bgzf_inflate.h): bytes in, an RFC 1950 stream out -- 2-byte header, DEFLATE
// blocks (RFC 1951), Adler-32.  Plain C++ that compiles for the host and the device, so the text that runs in
// zdeflate_kernels.hip is the text zd_deflate_host runs on the CPU under a sanitizer (tools/asan_zdeflate.sh).
//
// Form (pigz's): the input is cut into segments of `seg` bytes, each compressed on its own -- one lane per segment on the
// device.  A segment is one fixed-Huffman block: greedy LZ77, one candidate per position from a 256-entry hash of 4 bytes
// (entered at every literal, match start and match end) that holds positions of THIS segment only, so no match reaches before
// the segment's start.  A segment that is not the last ends in an empty stored block, which byte-aligns it, so the segments'
// streams concatenate by copying.  A segment whose fixed block would be larger than the segment stored is written as one
// stored block instead: seg_cap(len) = len + 5 bytes hold every segment, and bound(n) every stream.  Each segment's Adler-32
// is combined with zlib's adler32_combine arithmetic.  In dynamic mode (deflate_segment_dynamic, below) a segment is the smaller of
// that fixed block and a dynamic-Huffman block of the same parse, so no segment is larger than in fixed mode.
//   * the bytes depend on the input, `seg` and the mode alone: no atomics, no cross-lane state, no launch geometry;
//   * every output byte goes through Writer::byte, which checks the segment's cap (an overflow only sets a flag, and the
//     segment is then stored);
//   * input is read only at [0, len) of the segment.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZD_HD __host__ __device__
#else
#define ZD_HD
#endif

namespace zd {

constexpr uint32_t MIN_SEG = 1024, MAX_SEG = 32768, DEFAULT_SEG = 16384;   // (MAX_SEG: a position + 1 fits the uint16 hash entry,
                                                                           //  and every distance is <= 32 767)
constexpr uint64_t MAX_STREAM = 1ull << 31;                                 // bytes of one stream
constexpr int HASH_BITS = 8, HASH_SIZE = 1 << HASH_BITS;
constexpr uint32_t MIN_MATCH = 4, MAX_MATCH = 258;
constexpr uint32_t STORED_HEAD = 5;          // BFINAL/BTYPE byte, LEN, NLEN
constexpr uint32_t ADLER_BASE = 65521, ADLER_NMAX = 5552;

ZD_HD inline uint64_t n_segments(uint64_t n, uint32_t seg) { return n ? (n + seg - 1) / seg : 1; }
ZD_HD inline uint32_t seg_cap(uint32_t len) { return len + STORED_HEAD; }
// header (2) + every segment stored + Adler-32 (4)
ZD_HD inline uint64_t bound(uint64_t n, uint32_t seg) { return n + STORED_HEAD * n_segments(n, seg) + 6; }

struct Writer {
    uint8_t* out;
    uint32_t cap, pos;
    uint64_t buf;
    int cnt;
    bool ovf;
    ZD_HD void byte(uint8_t b) {
        if (pos < cap) out[pos++] = b;
        else ovf = true;
    }
    // n <= 32 bits of v, least significant first
    ZD_HD void put(uint32_t v, int n) {
        buf |= (uint64_t)v << cnt;
        cnt += n;
        while (cnt >= 8) {
            byte((uint8_t)buf);
            buf >>= 8;
            cnt -= 8;
        }
    }
    ZD_HD void align() {
        if (cnt) {
            byte((uint8_t)buf);
            buf = 0;
            cnt = 0;
        }
    }
};

// the low n (<= 16) bits of v in reverse order: Huffman codes go most significant bit first
ZD_HD inline uint32_t rev_bits(uint32_t v, int n) {
    v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
    v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
    v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
    v = ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
    return v >> (16 - n);
}

// RFC 1951 section 3.2.6: the fixed code of literal / length symbol s (0..285)
ZD_HD inline void put_symbol(Writer& w, uint32_t s) {
    if (s < 144) w.put(rev_bits(0x30 + s, 8), 8);
    else if (s < 256) w.put(rev_bits(0x190 + (s - 144), 9), 9);
    else if (s < 280) w.put(rev_bits(s - 256, 7), 7);
    else w.put(rev_bits(0xC0 + (s - 280), 8), 8);
}

ZD_HD inline int floor_log2(uint32_t v) { return 31 - __builtin_clz(v); }   // v > 0

// a match of len (MIN_MATCH..MAX_MATCH) at distance dist (1..32 768): section 3.2.5's length and distance codes, computed
ZD_HD inline void put_match(Writer& w, uint32_t len, uint32_t dist) {
    const uint32_t l = len - 3;
    if (len == 258) put_symbol(w, 285);
    else if (l < 8) put_symbol(w, 257 + l);
    else {
        const int e = floor_log2(l) - 2;
        put_symbol(w, 261 + 4 * e + ((l >> e) & 3));
        w.put(l & ((1u << e) - 1), e);
    }
    const uint32_t d = dist - 1;
    if (d < 4) w.put(rev_bits(d, 5), 5);
    else {
        const int e = floor_log2(d) - 1;
        w.put(rev_bits(2 * e + 2 + ((d >> e) & 1), 5), 5);
        w.put(d & ((1u << e) - 1), e);
    }
}

ZD_HD inline uint32_t load32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Adler-32 of in[0, len) from the initial value 1
ZD_HD inline uint32_t adler32(const uint8_t* in, uint32_t len) {
    uint32_t a = 1, b = 0;
    for (uint32_t i = 0; i < len;) {
        const uint32_t stop = len - i < ADLER_NMAX ? len : i + ADLER_NMAX;
        for (; i < stop; ++i) {
            a += in[i];
            b += a;
        }
        a %= ADLER_BASE;
        b %= ADLER_BASE;
    }
    return (b << 16) | a;
}

// zlib's adler32_combine: the checksum of A | B from those of A and B and the length of B
ZD_HD inline uint32_t adler32_combine(uint32_t adler1, uint32_t adler2, uint64_t len2) {
    const uint32_t rem = (uint32_t)(len2 % ADLER_BASE);
    uint32_t sum1 = adler1 & 0xffff;
    uint32_t sum2 = (uint32_t)(((uint64_t)rem * sum1) % ADLER_BASE);
    sum1 += (adler2 & 0xffff) + ADLER_BASE - 1;
    sum2 += ((adler1 >> 16) & 0xffff) + ((adler2 >> 16) & 0xffff) + ADLER_BASE - rem;
    if (sum1 >= ADLER_BASE) sum1 -= ADLER_BASE;
    if (sum1 >= ADLER_BASE) sum1 -= ADLER_BASE;
    if (sum2 >= (ADLER_BASE << 1)) sum2 -= (ADLER_BASE << 1);
    if (sum2 >= ADLER_BASE) sum2 -= ADLER_BASE;
    return sum1 | (sum2 << 16);
}

// The parse of one segment, the same for every pass over it: greedy, one candidate per position.  sink.literal(byte) and
// sink.match(len, dist) take the tokens in order; sink.stop() ends the parse early.  head: HASH_SIZE entries, `stride` apart
// (the device interleaves the lanes' tables in LDS), written before they are read.
template <class Sink>
ZD_HD inline void parse_segment(const uint8_t* in, uint32_t len, uint16_t* head, uint32_t stride, Sink& sink) {
    for (uint32_t i = 0; i < (uint32_t)HASH_SIZE; ++i) head[i * stride] = 0;
    uint32_t i = 0;
    while (i < len && !sink.stop()) {
        uint32_t mlen = 0, dist = 0;
        if (i + MIN_MATCH <= len) {
            const uint32_t h = (load32(in + i) * 2654435761u) >> (32 - HASH_BITS);
            const uint32_t cand = head[h * stride];    // 0: none; else a position of this segment below i, plus 1
            head[h * stride] = (uint16_t)(i + 1);
            if (cand) {
                const uint32_t c = cand - 1;
                const uint32_t maxl = len - i < MAX_MATCH ? len - i : MAX_MATCH;
                uint32_t l = 0;
                while (l < maxl && in[c + l] == in[i + l]) ++l;      // (c + l < i + l < len)
                if (l >= MIN_MATCH) {
                    mlen = l;
                    dist = i - c;
                }
            }
        }
        if (mlen) {
            sink.match(mlen, dist);
            i += mlen;
            // the match's last position as well: inside a run the next position then finds distance 1, the cheapest code
            if (i + MIN_MATCH - 1 <= len) head[((load32(in + i - 1) * 2654435761u) >> (32 - HASH_BITS)) * stride] = (uint16_t)i;
        } else {
            sink.literal(in[i]);
            ++i;
        }
    }
}

struct FixedSink {
    Writer& w;
    ZD_HD bool stop() const { return w.ovf; }
    ZD_HD void literal(uint8_t b) { put_symbol(w, b); }
    ZD_HD void match(uint32_t len, uint32_t dist) { put_match(w, len, dist); }
};

// what follows a segment's end-of-block symbol: nothing but the padding in the last one, else an empty stored block, which
// byte-aligns the next segment
ZD_HD inline void put_join(Writer& w, bool last) {
    if (last) w.align();
    else {
        w.put(0, 3);                                   // an empty stored block: BFINAL 0, BTYPE 00, to the byte boundary,
        w.align();
        w.byte(0); w.byte(0); w.byte(0xff); w.byte(0xff);          // LEN 0, NLEN
    }
}

ZD_HD inline uint32_t store_segment(const uint8_t* in, uint32_t len, bool last, uint8_t* out) {
    Writer s{out, seg_cap(len), 0, 0, 0, false};
    s.byte(last ? 1 : 0);
    s.byte((uint8_t)len); s.byte((uint8_t)(len >> 8));
    s.byte((uint8_t)~len); s.byte((uint8_t)(~len >> 8));
    for (uint32_t k = 0; k < len; ++k) s.byte(in[k]);
    return s.pos;
}

// One segment in fixed codes: in[0, len), len <= MAX_SEG, -> out[0, seg_cap(len)); returns the bytes written.
ZD_HD inline uint32_t deflate_segment(const uint8_t* in, uint32_t len, bool last, uint8_t* out, uint16_t* head, uint32_t stride) {
    Writer w{out, seg_cap(len), 0, 0, 0, false};
    w.put(last ? 1u : 0u, 1);
    w.put(1, 2);                                       // BTYPE 01: fixed codes
    FixedSink sink{w};
    parse_segment(in, len, head, stride, sink);
    put_symbol(w, 256);
    put_join(w, last);
    if (!w.ovf) return w.pos;
    return store_segment(in, len, last, out);          // the fixed block did not fit len + 5 bytes
}

// ---- dynamic codes (RFC 1951 section 3.2.7) -----------------------------------------------------------------------------------
// A segment in dynamic mode is parsed twice: the first pass counts the symbols, the codes are built from the counts and the
// exact sizes of the fixed and the dynamic block are compared before a byte is written; the second pass, the same parse, writes
// the block that is smaller.  The work area of one segment is WORK_SIZE uint32 entries, `stride` apart as `head` is: the
// counts of the literal / length, the distance and the code-length alphabet, each of which becomes that alphabet's
// (code, length) table in place.  The code construction has BUILD_SIZE entries of its own (one lane's, not interleaved: it is
// touched between the parses only).
constexpr uint32_t N_LL = 286, N_D = 30, N_CL = 19;
constexpr int MAX_BITS = 15, CL_BITS = 7;
constexpr uint32_t W_LL = 0, W_D = N_LL, W_CL = N_LL + N_D, WORK_SIZE = W_CL + N_CL;
constexpr uint32_t BUILD_SIZE = N_LL + 16;
constexpr int KIND_FIXED = 0, KIND_DYNAMIC = 1, KIND_STORED = 2;           // what a segment was written as

// section 3.2.5: the symbol of a match length (3..258) or distance (1..32 768) and the number e of extra bits, which are the
// low e bits of len - 3 or dist - 1
ZD_HD inline uint32_t length_symbol(uint32_t len, int& e) {
    const uint32_t l = len - 3;
    e = 0;
    if (len == 258) return 285;
    if (l < 8) return 257 + l;
    e = floor_log2(l) - 2;
    return 261 + 4 * e + ((l >> e) & 3);
}
ZD_HD inline uint32_t dist_symbol(uint32_t dist, int& e) {
    const uint32_t d = dist - 1;
    e = 0;
    if (d < 4) return d;
    e = floor_log2(d) - 1;
    return 2 * e + 2 + ((d >> e) & 1);
}
ZD_HD inline uint32_t fixed_length(uint32_t s) { return s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; }

// Code lengths of at most `limit` bits (<= 15) for the n (<= 286) symbols with counts t[s * stride] (their sum <= 65 535), which
// are replaced by the lengths, 0 for a symbol that does not occur; returns sum(count * length).  a: BUILD_SIZE entries of scratch.
// The used symbols are sorted as (count, symbol) words, Moffat and Katajainen's in-place construction turns the counts into depths
// (an optimal code; on equal weights it joins leaves before trees, which gives the least depth), and depths beyond the limit are
// folded into it and the Kraft sum repaired: a code of the limit leaves, the deepest shorter code is split in two.  Fewer than two
// used symbols give two codes of length 1, the form zlib writes (the used symbol and symbol 0, or symbols 0 and 1).
ZD_HD inline uint32_t code_lengths(uint32_t* t, uint32_t stride, uint32_t n, int limit, uint32_t* a) {
    uint32_t m = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t f = t[s * stride];
        if (f) a[m++] = (f << 16) | s;
    }
    if (m < 2) {
        const uint32_t only = m ? a[0] & 0xffff : 0;
        const uint32_t other = only ? 0 : 1;
        for (uint32_t s = 0; s < n; ++s) t[s * stride] = (s == only || s == other) ? 1 : 0;
        return m ? a[0] >> 16 : 0;
    }
    // ascending; the words are distinct, so every correct sort gives this order
    for (uint32_t gap = 64; gap; gap = gap > 1 ? (gap * 5 + 6) / 13 : 0)      // 64, 25, 10, 4, 2, 1
        for (uint32_t i = gap; i < m; ++i) {
            const uint32_t v = a[i];
            uint32_t j = i;
            for (; j >= gap && a[j - gap] > v; j -= gap) a[j] = a[j - gap];
            a[j] = v;
        }
#define ZD_VAL(i) (a[i] >> 16)
#define ZD_SET(i, v) (a[i] = ((uint32_t)(v) << 16) | (a[i] & 0xffff))
    // first pass: the trees' weights, then their parents, in the places of the counts
    ZD_SET(0, ZD_VAL(0) + ZD_VAL(1));
    uint32_t root = 0, leaf = 2;
    for (uint32_t next = 1; next + 1 < m; ++next) {
        uint32_t w;
        if (leaf >= m || ZD_VAL(root) < ZD_VAL(leaf)) {
            w = ZD_VAL(root);
            ZD_SET(root, next);
            ++root;
        } else w = ZD_VAL(leaf++);
        if (leaf >= m || (root < next && ZD_VAL(root) < ZD_VAL(leaf))) {
            w += ZD_VAL(root);
            ZD_SET(root, next);
            ++root;
        } else w += ZD_VAL(leaf++);
        ZD_SET(next, w);
    }
    // second pass: the depths of the inner nodes; third: of the leaves, the rarest symbol first in the array, so deepest
    ZD_SET(m - 2, 0);
    for (uint32_t next = m - 2; next-- > 0;) ZD_SET(next, ZD_VAL(ZD_VAL(next)) + 1);
    {
        uint32_t avbl = 1, used = 0, depth = 0;
        int32_t r = (int32_t)m - 2, next = (int32_t)m - 1;
        while (avbl > 0) {
            while (r >= 0 && ZD_VAL(r) == depth) {
                ++used;
                --r;
            }
            while (avbl > used) {
                ZD_SET(next, depth);
                --next;
                --avbl;
            }
            avbl = 2 * used;
            ++depth;
            used = 0;
        }
    }
    if (ZD_VAL(0) > (uint32_t)limit) {
        uint32_t* cnt = a + N_LL;                      // codes per length, the over-long ones at the limit
        for (int b = 0; b <= limit; ++b) cnt[b] = 0;
        for (uint32_t i = 0; i < m; ++i) {
            const uint32_t d = ZD_VAL(i);
            ++cnt[d > (uint32_t)limit ? (uint32_t)limit : d];
        }
        uint32_t total = 0;
        for (int b = 1; b <= limit; ++b) total += cnt[b] << (limit - b);
        for (; total != (1u << limit); --total) {
            --cnt[limit];
            for (int b = limit - 1; b > 0; --b)
                if (cnt[b]) {
                    --cnt[b];
                    cnt[b + 1] += 2;
                    break;
                }
        }
        uint32_t i = 0;
        for (int b = limit; b > 0; --b)
            for (uint32_t k = cnt[b]; k; --k, ++i) ZD_SET(i, b);
    }
    uint32_t cost = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint32_t at = (a[i] & 0xffff) * stride;
        cost += t[at] * ZD_VAL(i);
        t[at] = ZD_VAL(i);
    }
#undef ZD_SET
#undef ZD_VAL
    return cost;
}

// lengths -> (code << 4) | length, the code in the order the writer takes it (reversed); section 3.2.2's canonical codes
ZD_HD inline void assign_codes(uint32_t* t, uint32_t stride, uint32_t n, uint32_t* a) {
    for (int b = 0; b < 16; ++b) a[b] = 0;
    for (uint32_t s = 0; s < n; ++s) ++a[t[s * stride]];
    uint32_t code = 0, prev = 0;
    for (int b = 1; b < 16; ++b) {                      // a[b]: the next code of b bits
        code = (code + prev) << 1;
        prev = a[b];
        a[b] = code;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = t[s * stride];
        if (l) t[s * stride] = (rev_bits(a[l]++, (int)l) << 4) | l;
    }
}

// The code lengths of `count` symbols of one alphabet (the low 4 bits of their entries) as code-length symbols:
// sink.cl(symbol, extra bits, their value).  The rule: a run of zeros is cut into 18s of up to 138, then one 17 of 3..10, the rest
// single; a run of another length is the length once, then 16s of up to 6 repeats while 3 or more are left, the rest single.
template <class Sink>
ZD_HD inline void walk_lengths(const uint32_t* t, uint32_t stride, uint32_t count, Sink& sink) {
    uint32_t i = 0;
    while (i < count) {
        const uint32_t v = t[i * stride] & 15;
        uint32_t run = 1;
        while (i + run < count && (t[(i + run) * stride] & 15) == v) ++run;
        i += run;
        if (v == 0) {
            for (; run >= 11; run -= run < 138 ? run : 138) sink.cl(18, 7, (run < 138 ? run : 138) - 11);
            if (run >= 3) {
                sink.cl(17, 3, run - 3);
                run = 0;
            }
        } else {
            sink.cl(v, 0, 0);
            for (--run; run >= 3; run -= run < 6 ? run : 6) sink.cl(16, 2, (run < 6 ? run : 6) - 3);
        }
        for (; run; --run) sink.cl(v, 0, 0);
    }
}

struct ClCount {
    uint32_t* freq;
    uint32_t stride, extra;
    ZD_HD void cl(uint32_t s, int e, uint32_t) {
        ++freq[s * stride];
        extra += (uint32_t)e;
    }
};
struct ClWrite {
    Writer& w;
    const uint32_t* table;
    uint32_t stride;
    ZD_HD void cl(uint32_t s, int e, uint32_t x) {
        const uint32_t c = table[s * stride];
        w.put(c >> 4, (int)(c & 15));
        w.put(x, e);
    }
};

struct CountSink {
    uint32_t* work;
    uint32_t stride, extra;
    ZD_HD bool stop() const { return false; }
    ZD_HD void literal(uint8_t b) { ++work[(W_LL + b) * stride]; }
    ZD_HD void match(uint32_t len, uint32_t dist) {
        int e, f;
        ++work[(W_LL + length_symbol(len, e)) * stride];
        ++work[(W_D + dist_symbol(dist, f)) * stride];
        extra += (uint32_t)(e + f);
    }
};
struct DynamicSink {
    Writer& w;
    const uint32_t* work;
    uint32_t stride;
    ZD_HD bool stop() const { return w.ovf; }
    ZD_HD void code(uint32_t at) {
        const uint32_t c = work[at * stride];
        w.put(c >> 4, (int)(c & 15));
    }
    ZD_HD void literal(uint8_t b) { code(W_LL + b); }
    ZD_HD void match(uint32_t len, uint32_t dist) {
        int e;
        code(W_LL + length_symbol(len, e));
        w.put((len - 3) & ((1u << e) - 1), e);
        code(W_D + dist_symbol(dist, e));
        w.put((dist - 1) & ((1u << e) - 1), e);
    }
};

// bytes of a segment whose block, end-of-block symbol included, has `bits` bits (put_join)
ZD_HD inline uint32_t segment_bytes(uint32_t bits, bool last) { return last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4; }

// the order in which the header carries the code-length code's lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
ZD_HD inline uint32_t cl_order(uint32_t i) { return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - (i - 3) / 2 : 8 + (i - 4) / 2; }

// One segment in dynamic mode: as deflate_segment, with the work area (WORK_SIZE entries, `wstride` apart) and the build area
// above; *kind says what was written.  The fixed block is deflate_segment's own, so its bytes are those of fixed mode.
ZD_HD inline uint32_t deflate_segment_dynamic(const uint8_t* in, uint32_t len, bool last, uint8_t* out, uint16_t* head, uint32_t stride,
                                              uint32_t* work, uint32_t wstride, uint32_t* build, int* kind) {
    for (uint32_t k = 0; k < WORK_SIZE; ++k) work[k * wstride] = 0;
    CountSink count{work, wstride, 0};
    parse_segment(in, len, head, stride, count);
    uint32_t* ll = work + W_LL * wstride;
    uint32_t* dd = work + W_D * wstride;
    uint32_t* cl = work + W_CL * wstride;
    ++ll[256 * wstride];
    uint32_t fixed_bits = 3 + count.extra, dyn_bits = 3 + 5 + 5 + 4 + count.extra;
    for (uint32_t s = 0; s < N_LL; ++s) fixed_bits += ll[s * wstride] * fixed_length(s);
    for (uint32_t s = 0; s < N_D; ++s) fixed_bits += dd[s * wstride] * 5;
    dyn_bits += code_lengths(ll, wstride, N_LL, MAX_BITS, build);
    dyn_bits += code_lengths(dd, wstride, N_D, MAX_BITS, build);
    uint32_t n_ll = N_LL, n_d = N_D, n_cl = N_CL;
    while (n_ll > 257 && !ll[(n_ll - 1) * wstride]) --n_ll;
    while (n_d > 1 && !dd[(n_d - 1) * wstride]) --n_d;
    ClCount cc{cl, wstride, 0};
    walk_lengths(ll, wstride, n_ll, cc);
    walk_lengths(dd, wstride, n_d, cc);
    dyn_bits += cc.extra + code_lengths(cl, wstride, N_CL, CL_BITS, build);
    while (n_cl > 4 && !cl[cl_order(n_cl - 1) * wstride]) --n_cl;
    dyn_bits += 3 * n_cl;
    const uint32_t fixed_bytes = segment_bytes(fixed_bits, last), dyn_bytes = segment_bytes(dyn_bits, last);
    if (!(dyn_bytes < fixed_bytes)) {
        *kind = fixed_bytes > seg_cap(len) ? KIND_STORED : KIND_FIXED;
        return deflate_segment(in, len, last, out, head, stride);
    }
    if (dyn_bytes <= seg_cap(len)) {
        assign_codes(ll, wstride, N_LL, build);
        assign_codes(dd, wstride, N_D, build);
        assign_codes(cl, wstride, N_CL, build);
        Writer w{out, seg_cap(len), 0, 0, 0, false};
        w.put(last ? 1u : 0u, 1);
        w.put(2, 2);                                   // BTYPE 10: dynamic codes
        w.put(n_ll - 257, 5);
        w.put(n_d - 1, 5);
        w.put(n_cl - 4, 4);
        for (uint32_t i = 0; i < n_cl; ++i) w.put(cl[cl_order(i) * wstride] & 15, 3);
        ClWrite cw{w, cl, wstride};
        walk_lengths(ll, wstride, n_ll, cw);
        walk_lengths(dd, wstride, n_d, cw);
        DynamicSink sink{w, work, wstride};
        parse_segment(in, len, head, stride, sink);
        sink.code(W_LL + 256);
        put_join(w, last);
        if (!w.ovf) {                                  // (w.pos == dyn_bytes)
            *kind = KIND_DYNAMIC;
            return w.pos;
        }
    }
    *kind = KIND_STORED;
    return store_segment(in, len, last, out);
}

// What the pieces of one stream add up to: sizes[k], adlers[k] of its n_seg segments (lens: seg, the last one the rest of n)
// -> each segment's offset behind the 2-byte header, the stream's size and Adler-32, and whether it is "store" (not smaller
// than the n raw bytes).
struct StreamInfo {
    uint64_t size;
    uint32_t adler;
    uint32_t store;
};
ZD_HD inline StreamInfo finish_stream(uint64_t n, uint32_t seg, const uint32_t* sizes, const uint32_t* adlers, uint64_t* offs) {
    const uint64_t ns = n_segments(n, seg);
    uint64_t at = 0;
    uint32_t adler = 1;
    for (uint64_t k = 0; k < ns; ++k) {
        const uint64_t len = k + 1 < ns ? seg : n - k * seg;
        offs[k] = at;
        at += sizes[k];
        adler = k ? adler32_combine(adler, adlers[k], len) : adlers[0];
    }
    StreamInfo r;
    r.size = 2 + at + 4;
    r.adler = adler;
    r.store = r.size >= n ? 1u : 0u;
    return r;
}

constexpr uint8_t ZLIB_CMF = 0x78, ZLIB_FLG = 0x01;    // deflate, 32 KiB window, no dictionary, fastest; 0x7801 % 31 == 0

}  // namespace zd
