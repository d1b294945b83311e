// The record store of the candidate file's device loader (cl_store_*, include/dl4vc_chunks.h) where it needs no device: the
// definition of a record's extent, the layout of the trimmed records in slabs, and the CPU twins of the kernels of
// store_kernels.hip (record_extent, store_pack, store_assemble; record_spans, store_pack_compact).  Host only, no HIP include:
// tools/asan_store.sh and tools/asan_store_compact.sh compile it with a plain C++ compiler.
//
// A stored record is reads[kept][W] | qual[kept][W] | strand[kept][W] and zero bytes up to the next multiple of 16, where kept is
// 1 + the last stored row that holds a non-zero byte in any of the three planes (0: none does).  Rows >= kept are all-zero by
// that definition, so the assembly writes them as zeros and the store is exact whatever num_reads says.
//
// The compact format (FORMAT_COMPACT, chosen per store before its first append; windows of at most 255 columns).  For stored row
// r < kept, [c0_r, c0_r + n_r) is the smallest column range that contains every non-zero byte of the three planes in that row; a
// row below kept that is all zero has n_r = 0, c0_r = 0.  A compact record starts at a 16-byte boundary of a slab and holds
//   rowtab[kept + 1]  little-endian uint32: bits 0-23 off_r = the number of cells in rows < r, bits 24-31 c0_r (0 in the last
//                     entry); n_r = off_{r+1} - off_r, cells = off_kept
//   ts[cells]         for each cell, row by row, column by column: token | strand << 4
//   q[cells]          the quality byte
//   zeros up to the next multiple of 16:  span = pad16(4 (kept + 1) + 2 cells); kept = 0 takes no byte.
// Zero cells inside a span are stored like any other, so the format is exact without any assumption on the data.  A record with
// any byte >= 16 in the reads or strand plane is not mergeable and is stored in the rows layout inside the same store; the table
// entry of every record names its format.  CPU twins of record_spans, store_pack_compact and the compact side of store_assemble:
// spans_host, pack_compact_host, assemble_compact_plane_host.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "plan_entry.h"

namespace st {

constexpr int64_t SLAB_GUARD = 256;  // bytes of a device slab's allocation in front of its data (never written)
constexpr int64_t SLAB_PAD = 16;     // and behind them: a 16-byte load at a record's last bytes stays inside the allocation

enum { FORMAT_ROWS = 0, FORMAT_COMPACT = 1 };
constexpr int32_t COMPACT_MAX_WINDOW = 255;  // c0 and n of a row take eight bits each

inline uint64_t record_span(int64_t kept, int64_t W) { return ((uint64_t)(3 * kept * W) + 15u) & ~(uint64_t)15; }
inline uint64_t compact_span(int64_t kept, int64_t cells) {
    return kept ? ((uint64_t)(4 * (kept + 1) + 2 * cells) + 15u) & ~(uint64_t)15 : 0;
}
inline uint64_t format_span(int32_t format, int64_t kept, int64_t cells, int64_t W) {
    return format == FORMAT_COMPACT ? compact_span(kept, cells) : record_span(kept, W);
}

// what the spans of a record come to: kept as extent_host defines it, cells = the sum of n_r, mergeable = no byte >= 16 in the
// reads or strand plane
struct SpanSums {
    int32_t kept, cells, mergeable, pad;
};
// a row's span as the spans' scratch holds it: c0 | n << 8
inline uint16_t row_span(int32_t c0, int32_t n) { return (uint16_t)(c0 | n << 8); }

// Where the planes of the records to store lie: slot i's plane p, S rows of W bytes, at plane[p] + i * stride.  Records of
// record_bytes with their planes at plane_off (the inflated chunks of a file): plane[p] = records + plane_off[p], stride =
// record_bytes.  Three separate arrays [n_slots][S][W] (the pileup encoder's output): plane[p] = the array, stride = S * W.
struct HostSource {
    const uint8_t* plane[3];
    int64_t stride;
    const uint8_t* at(int p, int64_t slot) const { return plane[p] + (size_t)slot * (size_t)stride; }
};
inline HostSource record_source(const uint8_t* records, int64_t record_bytes, const int64_t* plane_off) {
    return HostSource{{records + plane_off[0], records + plane_off[1], records + plane_off[2]}, record_bytes};
}
inline HostSource planar_source(const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int32_t S, int32_t W) {
    return HostSource{{reads, qual, strand}, (int64_t)S * W};
}

// kept of the record at slot: planes of S rows of W bytes
inline int32_t extent_host(const HostSource& src, int64_t slot, int32_t S, int32_t W) {
    int32_t kept = 0;
    for (int p = 0; p < 3; ++p) {
        const uint8_t* q = src.at(p, slot);
        for (int64_t i = (int64_t)S * W - 1; i >= (int64_t)kept * W; --i)
            if (q[i]) {
                kept = (int32_t)(i / W) + 1;
                break;
            }
    }
    return kept;
}

// the spans of the record at slot (W <= COMPACT_MAX_WINDOW): rowspans[r] for every r < S (0 for a row without a non-zero byte)
inline SpanSums spans_host(const HostSource& src, int64_t slot, int32_t S, int32_t W, uint16_t* rowspans) {
    SpanSums out{0, 0, 1, 0};
    const uint8_t *a = src.at(0, slot), *q = src.at(1, slot), *b = src.at(2, slot);
    for (int32_t r = 0; r < S; ++r) {
        int32_t lo = W, hi = -1;
        for (int32_t c = 0; c < W; ++c) {
            const size_t i = (size_t)r * W + c;
            if (a[i] | q[i] | b[i]) {
                if (lo == W) lo = c;
                hi = c;
            }
            if ((a[i] | b[i]) >= 16) out.mergeable = 0;
        }
        const int32_t n = hi < 0 ? 0 : hi - lo + 1;
        rowspans[r] = row_span(n ? lo : 0, n);
        if (n) out.kept = r + 1;
        out.cells += n;
    }
    return out;
}

// the compact record of slot at dst, from the spans spans_host gave: compact_span(kept, cells) bytes
inline void pack_compact_host(const HostSource& src, int64_t slot, int32_t W, int32_t kept, const uint16_t* rowspans, uint8_t* dst) {
    if (!kept) return;
    const uint8_t *a = src.at(0, slot), *q = src.at(1, slot), *b = src.at(2, slot);
    uint32_t cells = 0;
    for (int32_t r = 0; r < kept; ++r) cells += rowspans[r] >> 8;
    uint8_t* ts = dst + 4 * ((size_t)kept + 1);
    uint8_t* qs = ts + cells;
    uint32_t off = 0;
    for (int32_t r = 0; r <= kept; ++r) {
        const uint32_t c0 = r < kept ? rowspans[r] & 255u : 0u, n = r < kept ? rowspans[r] >> 8 : 0u;
        const uint32_t e = off | c0 << 24;
        for (int k = 0; k < 4; ++k) dst[4 * (size_t)r + k] = (uint8_t)(e >> (8 * k));
        for (uint32_t j = 0; j < n; ++j) {
            const size_t i = (size_t)r * W + c0 + j;
            ts[off + j] = (uint8_t)(a[i] | b[i] << 4);
            qs[off + j] = q[i];
        }
        off += n;
    }
    const size_t body = 4 * ((size_t)kept + 1) + 2 * (size_t)cells;
    const size_t pad = (size_t)compact_span(kept, cells) - body;
    if (pad) memset(dst + body, 0, pad);
}

// the trimmed record of slot at dst: record_span(kept, W) bytes
inline void pack_host(const HostSource& src, int64_t slot, int32_t W, int32_t kept, uint8_t* dst) {
    const size_t n = (size_t)kept * W;
    for (int p = 0; p < 3; ++p)
        if (n) memcpy(dst + p * n, src.at(p, slot), n);
    const size_t pad = (size_t)record_span(kept, W) - 3 * n;
    if (pad) memset(dst + 3 * n, 0, pad);
}

// Where the records go.  Records are laid out in the order they are appended, each at a 16-byte boundary of a slab; one that does
// not fit what is left of the last slab opens the next, so none straddles two.  A slab holds slab_bytes, or what the capacity
// leaves when that is less.  A record without any row (kept = 0) takes no byte and is placed at (slab 0, offset 0).
struct Place {
    int32_t slab;
    uint64_t off;
};
struct Cursor {
    int64_t slabs = 0;
    uint64_t used = 0, cap = 0;      // of the last slab
    uint64_t stored = 0;             // sum of the spans of all records
};
enum { LAYOUT_OK = 0, LAYOUT_CAPACITY = 1, LAYOUT_SLAB = 2 };

// Places n records of the given spans (each 0 or a multiple of 16) behind cursor c (updated only on success); new_caps receives
// the sizes of the slabs to open.  *at: the first record that does not fit.
inline int layout_spans(Cursor& c, const uint64_t* spans, int64_t n, uint64_t slab_bytes, uint64_t capacity, Place* out,
                        std::vector<uint64_t>& new_caps, int64_t* at) {
    Cursor k = c;
    new_caps.clear();
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t b = spans[i];
        *at = i;
        if (b == 0) {
            out[i] = Place{0, 0};
            continue;
        }
        if (b > capacity || k.stored > capacity - b) return LAYOUT_CAPACITY;
        if (b > slab_bytes) return LAYOUT_SLAB;
        if (k.slabs == 0 || k.used + b > k.cap) {
            uint64_t cap = capacity - k.stored < slab_bytes ? capacity - k.stored : slab_bytes;
            cap &= ~(uint64_t)15;                        // (>= b: b is a multiple of 16 and fits both)
            new_caps.push_back(cap);
            ++k.slabs;
            k.used = 0;
            k.cap = cap;
        }
        out[i] = Place{(int32_t)(k.slabs - 1), k.used};
        k.used += b;
        k.stored += b;
    }
    c = k;
    return LAYOUT_OK;
}

// layout_spans for records in the rows layout, by their extents
inline int layout(Cursor& c, const int32_t* kept, int64_t n, int32_t W, uint64_t slab_bytes, uint64_t capacity, Place* out,
                  std::vector<uint64_t>& new_caps, int64_t* at) {
    std::vector<uint64_t> spans((size_t)n);
    for (int64_t i = 0; i < n; ++i) spans[(size_t)i] = record_span(kept[i], W);
    return layout_spans(c, spans.data(), n, slab_bytes, capacity, out, new_caps, at);
}

// One site of one plane, the CPU twin of store_assemble: R rows of L bytes at dst from the stored plane src[kept][L].  rows ==
// nullptr: the first R stored rows.  A row >= kept is zeros, and so is the reads plane (plane 0) of a row whose plan entry carries
// the zero-reads bit (plan_entry.h).
inline void assemble_plane_host(const uint8_t* src, int32_t kept, int plane, const int16_t* rows, int32_t R, int32_t L, uint8_t* dst) {
    for (int32_t r = 0; r < R; ++r) {
        const int32_t row = rows ? plan_entry::source_row(rows[r], plane) : r;
        if (row < kept) memcpy(dst + (size_t)r * L, src + (size_t)row * L, (size_t)L);
        else memset(dst + (size_t)r * L, 0, (size_t)L);
    }
}


// The same from a compact record at rec (rowtab | ts | q): plane 0 = ts & 15, 1 = q, 2 = ts >> 4; zeros outside a row's span.
inline void assemble_compact_plane_host(const uint8_t* rec, int32_t kept, int plane, const int16_t* rows, int32_t R, int32_t L, uint8_t* dst) {
    auto entry = [&](int32_t r) {
        const uint8_t* e = rec + 4 * (size_t)r;
        return (uint32_t)e[0] | (uint32_t)e[1] << 8 | (uint32_t)e[2] << 16 | (uint32_t)e[3] << 24;
    };
    if (!kept) {                                         // (no byte is stored: rec may be null)
        memset(dst, 0, (size_t)R * L);
        return;
    }
    const uint32_t cells = entry(kept) & 0xFFFFFFu;
    const uint8_t* ts = rec + 4 * ((size_t)kept + 1);
    const uint8_t* cell = plane == 1 ? ts + cells : ts;
    for (int32_t r = 0; r < R; ++r) {
        const int32_t row = rows ? plan_entry::source_row(rows[r], plane) : r;
        uint8_t* d = dst + (size_t)r * L;
        memset(d, 0, (size_t)L);
        if (row >= kept) continue;
        const uint32_t e = entry(row), off = e & 0xFFFFFFu, c0 = e >> 24, n = (entry(row + 1) & 0xFFFFFFu) - off;
        for (uint32_t j = 0; j < n; ++j) {
            const uint8_t x = cell[off + j];
            d[c0 + j] = plane == 0 ? (uint8_t)(x & 15) : plane == 2 ? (uint8_t)(x >> 4) : x;
        }
    }
}

}  // namespace st
