// The decode core of the BGZF inflate: one block's raw DEFLATE body (RFC 1951) in, its bytes out.  Plain C++ that compiles for
// the host and the device, so the text that runs in bgzf_kernels.hip is the text that runs on the CPU under a sanitizer
// (tools/asan_bgzf.sh).  The bit reader, the code-length decoding, the canonical tables, the symbol loop and every bounds check
// are here:
//   * every loop consumes input bits or produces output bytes on each turn, or runs a fixed count;
//   * input is read only through Bits, which never looks past body + body_len;
//   * output is written only through a Writer, after o + n <= isize was checked at the call site;
//   * a match is taken only when its distance is <= the bytes already produced.
// Also the CRC-32 pieces (table, update, and zlib's x^(8n) mod P combination) shared by the host loop and the kernel.
#pragma once

#include <stdint.h>
#include <string.h>

#include "../../include/dl4vc_bgzf.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif

namespace bz {

constexpr int LIT_BITS = 10, DIST_BITS = 8;   // primary lookup widths; longer codes take the canonical walk
constexpr uint32_t MAX_ISIZE = 65536;

// RFC 1951 section 3.2.5 (length and distance bases and extra bits) and 3.2.7 (the order of the code-length code's lengths)
constexpr uint16_t LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint16_t DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
constexpr uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
constexpr uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// A canonical Huffman code: how many codes of each length, and the symbols in code order.
struct Huff {
    uint16_t count[16];
    uint16_t symbol[288];
};
// Everything one block's decode needs besides its input and output (about 4.4 KB; LDS on the device).
struct Tables {
    Huff lit, dist;
    uint16_t lit_fast[1 << LIT_BITS];    // entry = symbol << 4 | length, 0 = the code is longer than the table
    uint16_t dist_fast[1 << DIST_BITS];
    uint16_t lens[320];
};

struct Bits {
    const uint8_t* p;
    uint32_t len, pos;
    uint64_t buf;
    int cnt;
    // after fill(): cnt >= 33, or every input byte is in buf
    BZ_HD void fill() {
        if (cnt <= 32 && pos + 4 <= len) {
            const uint32_t v = (uint32_t)p[pos] | ((uint32_t)p[pos + 1] << 8) | ((uint32_t)p[pos + 2] << 16) | ((uint32_t)p[pos + 3] << 24);
            buf |= (uint64_t)v << cnt;
            pos += 4;
            cnt += 32;
            return;
        }
        while (cnt <= 56 && pos < len) {
            buf |= (uint64_t)p[pos++] << cnt;
            cnt += 8;
        }
    }
    BZ_HD void drop(int n) { buf >>= n; cnt -= n; }
    // n <= 16
    BZ_HD bool take(int n, uint32_t& v) {
        if (cnt < n) {
            fill();
            if (cnt < n) return false;
        }
        v = (uint32_t)buf & ((1u << n) - 1);
        drop(n);
        return true;
    }
};

BZ_HD inline uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

// Builds the code of n lengths (each <= 15).  false: over-subscribed, or incomplete and not zlib's one exception (a single
// code of length 1; no codes at all is accepted too and then every decode fails).
BZ_HD inline bool build(Huff& h, uint16_t* fast, int fast_bits, const uint16_t* lens, int n) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (int i = 0; i < n; ++i) ++h.count[lens[i] & 15];
    for (int i = 0; i < (1 << fast_bits); ++i) fast[i] = 0;
    if (h.count[0] == n) return true;
    int left = 1, max_len = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - (int)h.count[l];
        if (left < 0) return false;
        if (h.count[l]) max_len = l;
    }
    if (left > 0 && max_len != 1) return false;
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + h.count[l]);
    for (int i = 0; i < n; ++i)
        if (lens[i] & 15) h.symbol[offs[lens[i] & 15]++] = (uint16_t)i;
    // (not over-subscribed, so the codes of length <= fast_bits fill at most the whole table)
    uint32_t code = 0;
    int idx = 0;
    for (int l = 1; l <= fast_bits; ++l) {
        for (int k = 0; k < (int)h.count[l]; ++k, ++idx, ++code) {
            const uint16_t e = (uint16_t)((h.symbol[idx] << 4) | l);
            for (uint32_t j = reverse_bits(code, l); j < (1u << fast_bits); j += 1u << l) fast[j] = e;
        }
        code <<= 1;
    }
    return true;
}

BZ_HD inline int decode(Bits& b, const Huff& h, const uint16_t* fast, int fast_bits, uint32_t& sym) {
    b.fill();
    const uint16_t e = fast[(uint32_t)b.buf & ((1u << fast_bits) - 1)];
    if (e) {
        const int l = e & 15;
        if (l > b.cnt) return BZ_INPUT_EXHAUSTED;
        b.drop(l);
        sym = e >> 4;
        return BZ_OK;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        if (l > b.cnt) return BZ_INPUT_EXHAUSTED;
        code |= (int)((b.buf >> (l - 1)) & 1);
        const int c = h.count[l];
        if (code - c < first) {
            b.drop(l);
            sym = h.symbol[index + (code - first)];
            return BZ_OK;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return BZ_BAD_SYMBOL;   // a code outside an incomplete set
}

BZ_HD inline int read_dynamic(Bits& b, Tables& t) {
    uint32_t v;
    if (!b.take(14, v)) return BZ_INPUT_EXHAUSTED;
    const int nlen = 257 + (int)(v & 31), ndist = 1 + (int)((v >> 5) & 31), ncode = 4 + (int)(v >> 10);
    if (nlen > 286 || ndist > 30) return BZ_BAD_CODE_LENGTHS;
    for (int i = 0; i < 19; ++i) t.lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!b.take(3, v)) return BZ_INPUT_EXHAUSTED;
        t.lens[ORDER[i]] = (uint16_t)v;
    }
    if (!build(t.dist, t.dist_fast, DIST_BITS, t.lens, 19)) return BZ_BAD_CODE_LENGTHS;
    int i = 0;
    while (i < nlen + ndist) {          // (each turn consumes at least one bit and adds at least one length)
        uint32_t sym;
        const int rc = decode(b, t.dist, t.dist_fast, DIST_BITS, sym);
        if (rc) return rc;
        if (sym < 16) {
            t.lens[i++] = (uint16_t)sym;
            continue;
        }
        uint32_t rep;
        uint16_t val = 0;
        if (sym == 16) {
            if (i == 0) return BZ_BAD_CODE_LENGTHS;
            val = t.lens[i - 1];
            if (!b.take(2, rep)) return BZ_INPUT_EXHAUSTED;
            rep += 3;
        } else if (sym == 17) {
            if (!b.take(3, rep)) return BZ_INPUT_EXHAUSTED;
            rep += 3;
        } else {
            if (!b.take(7, rep)) return BZ_INPUT_EXHAUSTED;
            rep += 11;
        }
        if (i + (int)rep > nlen + ndist) return BZ_BAD_CODE_LENGTHS;
        for (uint32_t k = 0; k < rep; ++k) t.lens[i++] = val;
    }
    if (t.lens[256] == 0) return BZ_BAD_CODE_LENGTHS;   // no end-of-block code
    if (!build(t.lit, t.lit_fast, LIT_BITS, t.lens, nlen)) return BZ_BAD_CODE_LENGTHS;
    if (!build(t.dist, t.dist_fast, DIST_BITS, t.lens + nlen, ndist)) return BZ_BAD_CODE_LENGTHS;
    return BZ_OK;
}

BZ_HD inline void set_fixed(Tables& t) {
    for (int i = 0; i < 288; ++i) t.lens[i] = (uint16_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    (void)build(t.lit, t.lit_fast, LIT_BITS, t.lens, 288);
    for (int i = 0; i < 32; ++i) t.lens[i] = 5;        // (30 and 31 are in the code and refused when met)
    (void)build(t.dist, t.dist_fast, DIST_BITS, t.lens, 32);
}

// How decoded bytes reach out[]; the caller of each method has checked the bounds (o + n <= isize, dist <= o, n source bytes).
// This one is a single thread's; bgzf_kernels.hip has the wave's, for which every lane runs the decode in step.
struct SerialWriter {
    BZ_HD void literal(uint8_t* out, uint32_t o, uint8_t v) const { out[o] = v; }
    BZ_HD void stored(uint8_t* out, uint32_t o, const uint8_t* src, uint32_t n) const {
        for (uint32_t k = 0; k < n; ++k) out[o + k] = src[k];
    }
    BZ_HD void match(uint8_t* out, uint32_t o, uint32_t dist, uint32_t n) const {
        for (uint32_t k = 0; k < n; ++k) out[o + k] = out[o + k - dist];   // (byte order makes distance < length right)
    }
};

// Inflates body[0, body_len) into out[0, isize).  *produced = bytes written (also on failure).  The CRC is the caller's.
template <class Writer>
BZ_HD inline int inflate_block(const uint8_t* body, uint32_t body_len, uint8_t* out, uint32_t isize, Tables& t, uint32_t* produced,
                               const Writer& wr) {
    Bits b{body, body_len, 0, 0, 0};
    uint32_t o = 0;
    *produced = 0;
    for (;;) {                            // (each DEFLATE block consumes its 3 header bits)
        uint32_t hdr;
        if (!b.take(3, hdr)) return BZ_INPUT_EXHAUSTED;
        const int type = (int)(hdr >> 1);
        if (type == 3) return BZ_BAD_BLOCK_TYPE;
        if (type == 0) {
            b.drop(b.cnt & 7);
            uint32_t len, nlen;
            if (!b.take(16, len) || !b.take(16, nlen)) return BZ_INPUT_EXHAUSTED;
            if ((len ^ 0xffff) != nlen) return BZ_BAD_STORED_LEN;
            if (len > isize - o) return BZ_OUTPUT_EXCEEDS_ISIZE;
            // (cnt is a multiple of 8 here: first the bytes already in the bit buffer, then straight from the body)
            while (len > 0 && b.cnt >= 8) { wr.literal(out, o++, (uint8_t)b.buf); b.drop(8); --len; }
            if (len > b.len - b.pos) return BZ_INPUT_EXHAUSTED;
            wr.stored(out, o, b.p + b.pos, len);
            o += len;
            b.pos += len;
            *produced = o;
        } else {
            if (type == 1) {
                set_fixed(t);
            } else {
                const int rc = read_dynamic(b, t);
                if (rc) return rc;
            }
            for (;;) {                    // (each turn consumes at least one bit)
                uint32_t sym;
                int rc = decode(b, t.lit, t.lit_fast, LIT_BITS, sym);
                if (rc) { *produced = o; return rc; }
                if (sym < 256) {
                    if (o >= isize) { *produced = o; return BZ_OUTPUT_EXCEEDS_ISIZE; }
                    wr.literal(out, o++, (uint8_t)sym);
                    continue;
                }
                if (sym == 256) break;
                *produced = o;
                if (sym >= 286) return BZ_BAD_SYMBOL;
                sym -= 257;
                uint32_t extra = 0, dsym;
                if (LEXT[sym] && !b.take(LEXT[sym], extra)) return BZ_INPUT_EXHAUSTED;
                const uint32_t len = LBASE[sym] + extra;
                rc = decode(b, t.dist, t.dist_fast, DIST_BITS, dsym);
                if (rc) return rc;
                if (dsym >= 30) return BZ_BAD_SYMBOL;
                extra = 0;
                if (DEXT[dsym] && !b.take(DEXT[dsym], extra)) return BZ_INPUT_EXHAUSTED;
                const uint32_t dist = DBASE[dsym] + extra;
                if (dist > o) return BZ_DISTANCE_BEFORE_START;
                if (len > isize - o) return BZ_OUTPUT_EXCEEDS_ISIZE;
                wr.match(out, o, dist, len);
                o += len;
            }
            *produced = o;
        }
        if (hdr & 1) break;
    }
    if (o < isize) return BZ_OUTPUT_SHORT_OF_ISIZE;
    // whole bytes left in the bit buffer were not consumed; the bits of a started byte were
    if (b.pos - (uint32_t)(b.cnt >> 3) != body_len) return BZ_TRAILING_INPUT;
    return BZ_OK;
}

// ---- CRC-32 (the zlib polynomial, reflected) ---------------------------------------------------------------------------
constexpr uint32_t CRC_POLY = 0xedb88320u;

BZ_HD inline uint32_t crc_table_entry(uint32_t i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    return c;
}
// zlib.crc32 of p[0, n) (0 for n == 0), with table[i] = crc_table_entry(i)
BZ_HD inline uint32_t crc_bytes(const uint32_t* table, const uint8_t* p, uint32_t n) {
    uint32_t c = 0xffffffffu;
    for (uint32_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return c ^ 0xffffffffu;
}
// a(x) * b(x) mod P in the reflected representation (x^0 is bit 31)
BZ_HD inline uint32_t crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if (a & (1u << i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
// x^(8n) mod P
BZ_HD inline uint32_t crc_xpow8(uint32_t n) {
    uint32_t p = 1u << 31, base = 1u << 23;
    for (int i = 0; i < 32 && n; ++i, n >>= 1) {
        if (n & 1) p = crc_mulmod(p, base);
        base = crc_mulmod(base, base);
    }
    return p;
}
// crc(A || B) from crc(A), crc(B) and xp = crc_xpow8(len(B))
BZ_HD inline uint32_t crc_append(uint32_t crc_a, uint32_t crc_b, uint32_t xp) { return crc_mulmod(xp, crc_a) ^ crc_b; }

// ---- the block header and trailer --------------------------------------------------------------------------------------
struct BlockDesc {
    uint64_t body_off;     // of the DEFLATE body within the compressed bytes
    uint64_t out_off;
    uint32_t body_len;     // without the 8-byte trailer
    uint32_t isize;
    uint32_t crc;
    int32_t status;        // BZ_OK, or why the block cannot be decoded at all (BZ_BAD_HEADER, BZ_BAD_SLOT)
};

// Reads the header at blocks[off] (any XLEN, the BC subfield found by walking the extra field) and the trailer.  *bsize = the
// block's whole length.  BZ_BAD_HEADER when it is no BGZF block or does not lie inside [0, nbytes).
inline int parse_block(const uint8_t* blocks, uint64_t nbytes, uint64_t off, BlockDesc& d, uint32_t* bsize) {
    d = BlockDesc{};
    d.status = BZ_BAD_HEADER;
    if (off > nbytes || nbytes - off < 18) return d.status;
    const uint8_t* h = blocks + off;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return d.status;
    const uint32_t xlen = h[10] | ((uint32_t)h[11] << 8);
    if (nbytes - off < 12 + (uint64_t)xlen) return d.status;
    int64_t bs = -1;
    for (uint32_t i = 0; i + 4 <= xlen;) {
        const uint32_t slen = h[12 + i + 2] | ((uint32_t)h[12 + i + 3] << 8);
        if (h[12 + i] == 'B' && h[12 + i + 1] == 'C' && slen == 2 && i + 6 <= xlen) bs = h[12 + i + 4] | ((int64_t)h[12 + i + 5] << 8);
        i += 4 + slen;
    }
    if (bs < 0) return d.status;
    const int64_t body = bs + 1 - 12 - (int64_t)xlen;
    if (body < 8 || (uint64_t)(bs + 1) > nbytes - off) return d.status;
    const uint8_t* tr = h + bs + 1 - 8;
    d.crc = tr[0] | ((uint32_t)tr[1] << 8) | ((uint32_t)tr[2] << 16) | ((uint32_t)tr[3] << 24);
    d.isize = tr[4] | ((uint32_t)tr[5] << 8) | ((uint32_t)tr[6] << 16) | ((uint32_t)tr[7] << 24);
    if (d.isize > MAX_ISIZE) return d.status;
    d.body_off = off + 12 + xlen;
    d.body_len = (uint32_t)(body - 8);
    *bsize = (uint32_t)(bs + 1);
    d.status = BZ_OK;
    return BZ_OK;
}

// One block on the host: decode, then the CRC.  table: 256 entries of crc_table_entry.
inline int inflate_block_host(const uint8_t* comp, const BlockDesc& d, uint8_t* out, Tables& t, const uint32_t* table) {
    if (d.status) return d.status;
    uint32_t produced = 0;
    const int rc = inflate_block(comp + d.body_off, d.body_len, out + d.out_off, d.isize, t, &produced, SerialWriter());
    if (rc) return rc;
    return crc_bytes(table, out + d.out_off, d.isize) == d.crc ? BZ_OK : BZ_CRC_MISMATCH;
}

}  // namespace bz
