// The record store of the candidate file's device loader (cl_store_*, include/dl4vc_chunks.h) where it needs no device: the
// definition of a record's extent, the layout of the trimmed records in slabs, and the CPU twins of the three kernels of
// store_kernels.hip (record_extent, store_pack, store_assemble).  Host only, no HIP include: tools/asan_store.sh compiles it with
// a plain C++ compiler.
//
// A stored record is reads[kept][W] | qual[kept][W] | strand[kept][W] and zero bytes up to the next multiple of 16, where kept is
// 1 + the last stored row that holds a non-zero byte in any of the three planes (0: none does).  Rows >= kept are all-zero by
// that definition, so the assembly writes them as zeros and the store is exact whatever num_reads says.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace st {

constexpr int64_t SLAB_GUARD = 256;  // bytes of a device slab's allocation in front of its data (never written)
constexpr int64_t SLAB_PAD = 16;     // and behind them: a 16-byte load at a record's last bytes stays inside the allocation

inline uint64_t record_span(int64_t kept, int64_t W) { return ((uint64_t)(3 * kept * W) + 15u) & ~(uint64_t)15; }

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

// Places n records behind cursor c (updated only on success); new_caps receives the sizes of the slabs to open.  *at: the first
// record that does not fit.
inline int layout(Cursor& c, const int32_t* kept, int64_t n, int32_t W, uint64_t slab_bytes, uint64_t capacity, Place* out,
                  std::vector<uint64_t>& new_caps, int64_t* at) {
    Cursor k = c;
    new_caps.clear();
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t b = record_span(kept[i], W);
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

// One site of one plane, the CPU twin of store_assemble: R rows of L bytes at dst from the stored plane src[kept][L].  rows ==
// nullptr: the first R stored rows.  A row >= kept is zeros.
inline void assemble_plane_host(const uint8_t* src, int32_t kept, const int16_t* rows, int32_t R, int32_t L, uint8_t* dst) {
    for (int32_t r = 0; r < R; ++r) {
        const int32_t row = rows ? rows[r] : r;
        if (row < kept) memcpy(dst + (size_t)r * L, src + (size_t)row * L, (size_t)L);
        else memset(dst + (size_t)r * L, 0, (size_t)L);
    }
}

}  // namespace st
