// zlib streams (RFC 1950) of any length through the decode core of bgzf_inflate.h: the header check, a Writer that keeps the
// output in a 64 KiB ring, and the Adler-32.  Plain C++ that compiles for the host and the device: the text zi_inflate_kernel
// runs with 64 lanes (zinflate_kernels.hip) is the text zi_inflate_host runs with one (tools/asan_zinflate.sh, under sanitizers).
//
// The ring.  Output position o is absolute; its byte lives at ring[(o + shift) & 0xFFFF], where shift = the slot's address modulo
// 16, so ring index and destination address agree modulo 16 and a completed half goes out in aligned 16-byte stores.  After
// every Writer call, o - flushed < HALF (flushed: a multiple of HALF, the bytes below it are in the destination and in the
// running Adler-32):
//   * literal() writes one byte and flushes the half it completes;
//   * stored() cuts its run at the half boundaries (a stored DEFLATE block holds up to 65 535 bytes, more than a half) and
//     flushes each half it completes; its source is the input, never the ring;
//   * match() does not cut.  It writes [o, o + n), n <= 258, and then flushes at most one half.  A write at position p takes
//     the ring byte of p - 65 536.  With p < o + 258 and o < flushed + HALF that is below flushed + 258 - HALF <= flushed: the
//     byte is in the destination already.  And it is below o - 65 536 + 258, while a match reads no further back than
//     o - 32 768: out of any match's reach.  A match's source [o - dist, o) is at most HALF bytes old, so it is still in the ring.
// No back-reference ever reads the destination, and the destination is written once, in order, inside [0, isize) only: every
// flush ends at a position the core has checked against isize.  A stream that fails has flushed the halves it completed.
#pragma once

#include "bgzf_inflate.h"
#include "zdeflate.h"

#include "../../include/dl4vc_chunks.h"

namespace zi {

constexpr uint32_t RING = 65536, MASK = RING - 1, HALF = 32768;
constexpr uint64_t MAX_OUTPUT = ZI_MAX_OUTPUT;

static_assert(ZI_BAD_BLOCK_TYPE == BZ_BAD_BLOCK_TYPE && ZI_BAD_STORED_LEN == BZ_BAD_STORED_LEN && ZI_BAD_CODE_LENGTHS == BZ_BAD_CODE_LENGTHS &&
                  ZI_BAD_SYMBOL == BZ_BAD_SYMBOL && ZI_DISTANCE_BEFORE_START == BZ_DISTANCE_BEFORE_START &&
                  ZI_OUTPUT_EXCEEDS_LENGTH == BZ_OUTPUT_EXCEEDS_ISIZE && ZI_OUTPUT_SHORT_OF_LENGTH == BZ_OUTPUT_SHORT_OF_ISIZE &&
                  ZI_INPUT_EXHAUSTED == BZ_INPUT_EXHAUSTED && ZI_TRAILING_INPUT == BZ_TRAILING_INPUT && ZI_BAD_SLOT == BZ_BAD_SLOT,
              "the shared causes keep the BZ_* numbers");

// One stream of a call, validated by the host (status != ZI_OK: refused, nothing of it is read or written).
struct StreamDesc {
    uint64_t in_off, out_off;
    uint32_t in_len, out_len;
    int32_t raw, status;
};

// The lanes that run a stream: one on the host.  (The device's: 64, in zinflate_kernels.hip.)
struct OneLane {
    static constexpr uint32_t WIDTH = 1;
    BZ_HD uint32_t lane() const { return 0; }
    BZ_HD void sync() const {}
    BZ_HD static void copy16(uint8_t* dst, const uint8_t* src) { memcpy(dst, src, 16); }
};

// Adler-32 (from the initial value 1) of the n bytes at ring positions r, r + 1, ...
BZ_HD inline uint32_t adler_ring(const uint8_t* ring, uint32_t r, uint32_t n) {
    uint32_t a = 1, b = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t stop = n - i < zd::ADLER_NMAX ? n : i + zd::ADLER_NMAX;
        for (; i < stop; ++i) {
            a += ring[(r + i) & MASK];
            b += a;
        }
        a %= zd::ADLER_BASE;
        b %= zd::ADLER_BASE;
    }
    return (b << 16) | a;
}

// The Writer of bz::inflate_block (its `out` is the ring).  Every lane of Par calls each method with the same arguments, so
// flushed and adler are the same in every lane.  A match byte k comes from position o - dist + k % dist, below o: no lane reads
// what another writes in the same copy.  The syncs (one wave: no other to wait for) keep the compiler from moving a read of
// the ring above the writes before it.
template <class Par>
struct RingWriter {
    Par par;
    uint8_t* dst;          // the slot
    uint32_t shift;        // its address modulo 16
    uint32_t* scratch;     // Par::WIDTH entries
    mutable uint32_t flushed = 0, adler = 1;

    BZ_HD void literal(uint8_t* ring, uint32_t o, uint8_t v) const {
        if (par.lane() == 0) ring[(o + shift) & MASK] = v;
        if (o + 1 - flushed >= HALF) flush(ring, flushed + HALF);
    }
    BZ_HD void stored(uint8_t* ring, uint32_t o, const uint8_t* src, uint32_t n) const {
        while (n > 0) {                                      // (each turn takes m >= 1 bytes: o - flushed < HALF)
            const uint32_t room = flushed + HALF - o, m = n < room ? n : room;
            for (uint32_t k = par.lane(); k < m; k += Par::WIDTH) ring[(o + k + shift) & MASK] = src[k];
            o += m;
            src += m;
            n -= m;
            if (o - flushed >= HALF) flush(ring, flushed + HALF);
        }
        par.sync();
    }
    BZ_HD void match(uint8_t* ring, uint32_t o, uint32_t dist, uint32_t n) const {
        par.sync();
        const uint32_t from = o - dist + shift, to = o + shift;
        if (dist >= n) {
            for (uint32_t k = par.lane(); k < n; k += Par::WIDTH) ring[(to + k) & MASK] = ring[(from + k) & MASK];
        } else {
            for (uint32_t k = par.lane(); k < n; k += Par::WIDTH) ring[(to + k) & MASK] = ring[(from + k % dist) & MASK];
        }
        par.sync();
        if (o + n - flushed >= HALF) flush(ring, flushed + HALF);
    }
    // What is left below `end` (the stream's length, after a clean decode).
    BZ_HD void finish(uint8_t* ring, uint32_t end) const {
        if (end > flushed) flush(ring, end);
    }

    // Positions [flushed, upto), at most HALF of them, to the destination and into the Adler-32: bytes up to the first 16-byte
    // boundary, whole 16-byte words, the rest.  A word never straddles the ring's end (its index is a multiple of 16).
    BZ_HD void flush(uint8_t* ring, uint32_t upto) const {
        par.sync();
        const uint32_t lane = par.lane(), p0 = flushed, len = upto - p0, r0 = p0 + shift;
        uint8_t* g = dst + p0;                               // (g's address = r0 modulo 16)
        const uint32_t to_boundary = (16 - (r0 & 15)) & 15, head = len < to_boundary ? len : to_boundary;
        for (uint32_t k = lane; k < head; k += Par::WIDTH) g[k] = ring[(r0 + k) & MASK];
        const uint32_t words = (len - head) / 16;
        for (uint32_t i = lane; i < words; i += Par::WIDTH) Par::copy16(g + head + 16 * i, ring + ((r0 + head + 16 * i) & MASK));
        for (uint32_t k = head + 16 * words + lane; k < len; k += Par::WIDTH) g[k] = ring[(r0 + k) & MASK];
        // Adler-32: lane i takes bytes [i * per, min(len, (i + 1) * per)); every lane then folds the slices in order
        const uint32_t per = (len + Par::WIDTH - 1) / Par::WIDTH;
        const uint32_t lo = len < lane * per ? len : lane * per, hi = len < lo + per ? len : lo + per;
        scratch[lane] = adler_ring(ring, r0 + lo, hi - lo);
        par.sync();
        uint32_t acc = adler;
        for (uint32_t i = 0; i < Par::WIDTH; ++i) {
            const uint32_t a = len < i * per ? len : i * per, b = len < a + per ? len : a + per;
            if (b == a) break;
            acc = zd::adler32_combine(acc, scratch[i], b - a);
        }
        par.sync();                                          // (scratch is written again by the next flush)
        adler = acc;
        flushed = upto;
    }
};

// CM = 8 (deflate), CINFO <= 7 (a window of at most 32 KiB), FCHECK, no preset dictionary
BZ_HD inline bool zlib_header_ok(uint8_t cmf, uint8_t flg) {
    return (cmf & 15) == 8 && (cmf >> 4) <= 7 && (((uint32_t)cmf << 8) | flg) % 31 == 0 && !(flg & 0x20);
}

// The stream in[0, n) into dst[0, out_len); ring: RING bytes at a 16-byte boundary, scratch: Par::WIDTH words.
template <class Par>
BZ_HD inline int inflate_stream(const uint8_t* in, uint32_t n, uint8_t* dst, uint32_t out_len, uint8_t* ring, bz::Tables& t,
                                uint32_t* scratch, const Par& par) {
    if (n < 2) return ZI_INPUT_EXHAUSTED;
    if (!zlib_header_ok(in[0], in[1])) return ZI_BAD_ZLIB_HEADER;
    if (n < 6) return ZI_INPUT_EXHAUSTED;
    RingWriter<Par> wr{par, dst, (uint32_t)((uintptr_t)dst & 15), scratch};
    uint32_t produced = 0;
    const int rc = bz::inflate_block(in + 2, n - 6, ring, out_len, t, &produced, wr);
    if (rc) return rc;
    wr.finish(ring, out_len);
    const uint8_t* tr = in + n - 4;
    const uint32_t want = ((uint32_t)tr[0] << 24) | ((uint32_t)tr[1] << 16) | ((uint32_t)tr[2] << 8) | tr[3];
    return wr.adler == want ? ZI_OK : ZI_ADLER_MISMATCH;
}

// A chunk that was not deflated: exactly its bytes.
template <class Par>
BZ_HD inline int copy_raw(const uint8_t* in, uint32_t n, uint8_t* dst, uint32_t out_len, const Par& par) {
    if (n != out_len) return ZI_RAW_SIZE_MISMATCH;
    for (uint32_t k = par.lane(); k < n; k += Par::WIDTH) dst[k] = in[k];
    return ZI_OK;
}

template <class Par>
BZ_HD inline int run_stream(const uint8_t* streams, const StreamDesc& d, uint8_t* out, uint8_t* ring, bz::Tables& t, uint32_t* scratch,
                            const Par& par) {
    if (d.status != ZI_OK) return d.status;
    return d.raw ? copy_raw(streams + d.in_off, d.in_len, out + d.out_off, d.out_len, par)
                 : inflate_stream(streams + d.in_off, d.in_len, out + d.out_off, d.out_len, ring, t, scratch, par);
}

}  // namespace zi
