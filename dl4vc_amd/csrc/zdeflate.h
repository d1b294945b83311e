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
// is combined with zlib's adler32_combine arithmetic.
//   * the bytes depend on the input and `seg` alone: no atomics, no cross-lane state, no launch geometry;
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

// One segment: in[0, len), len <= MAX_SEG, -> out[0, seg_cap(len)); returns the bytes written.  head: HASH_SIZE entries,
// `stride` apart (the device interleaves the lanes' tables in LDS), written before they are read.
ZD_HD inline uint32_t deflate_segment(const uint8_t* in, uint32_t len, bool last, uint8_t* out, uint16_t* head, uint32_t stride) {
    Writer w{out, seg_cap(len), 0, 0, 0, false};
    for (uint32_t i = 0; i < (uint32_t)HASH_SIZE; ++i) head[i * stride] = 0;
    w.put(last ? 1u : 0u, 1);
    w.put(1, 2);                                       // BTYPE 01: fixed codes
    uint32_t i = 0;
    while (i < len && !w.ovf) {
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
            put_match(w, mlen, dist);
            i += mlen;
            // the match's last position as well: inside a run the next position then finds distance 1, the cheapest code
            if (i + MIN_MATCH - 1 <= len) head[((load32(in + i - 1) * 2654435761u) >> (32 - HASH_BITS)) * stride] = (uint16_t)i;
        } else {
            put_symbol(w, in[i]);
            ++i;
        }
    }
    put_symbol(w, 256);
    if (last) w.align();
    else {
        w.put(0, 3);                                   // an empty stored block: BFINAL 0, BTYPE 00, to the byte boundary,
        w.align();
        w.byte(0); w.byte(0); w.byte(0xff); w.byte(0xff);          // LEN 0, NLEN
    }
    if (!w.ovf) return w.pos;
    // stored: the fixed block did not fit len + 5 bytes
    Writer s{out, seg_cap(len), 0, 0, 0, false};
    s.byte(last ? 1 : 0);
    s.byte((uint8_t)len); s.byte((uint8_t)(len >> 8));
    s.byte((uint8_t)~len); s.byte((uint8_t)(~len >> 8));
    for (uint32_t k = 0; k < len; ++k) s.byte(in[k]);
    return s.pos;
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
