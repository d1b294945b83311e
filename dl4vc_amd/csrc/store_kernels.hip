// The record store of the candidate file's device loader (cl_store_*): the records of a training file, inflated once, kept in
// device memory trimmed of their trailing all-zero rows, and the sites of every batch assembled from there.  The CPU twins of the
// kernels are in store_host.h; store_capi.cpp checks every index before a launch.
//
// record_extent: one workgroup per source slot (Source: an inflated record, or a slot of the pileup encoder's three plane
// arrays -- only the address of a slot's plane differs).  Each plane's S * W bytes are cut at the 16-byte boundaries of the SOURCE
// (a record is an odd number of bytes, so planes start at every alignment; a slot of S * W = 40 200 bytes starts 0 or 8 bytes
// past one, and a view of an allocation anywhere): the bytes before the first boundary and behind the
// last one are read one by one, everything between with aligned 16-byte loads.  Every lane keeps the highest row in which it saw
// a non-zero byte, the wave takes the maximum by shuffles, the four waves theirs through LDS, and lane 0 writes kept.
//
// store_pack: one workgroup per (record, plane) copies kept * W bytes to the record's place in a slab, cut at the 16-byte
// boundaries of the DESTINATION as assemble_planes does: aligned 16-byte stores, a 16-byte load at the source's own alignment,
// bytes one by one at both ends.  The strand plane's workgroup zeroes the bytes up to the record's 16-byte end, the reads plane's
// writes the record's table entry.  No load reaches past the plane it copies.
//
// store_assemble: assemble_planes (assemble_kernels.hip) with the store as the source: one workgroup per (site, plane), the span
// of R * L output bytes cut at the destination's 16-byte boundaries, every output byte written by exactly one lane.  A row >=
// kept is zeros, and so is the reads plane of a row whose plan entry carries the zero-reads bit (plan_entry.h: a flagged row of a
// compact record decodes its ts byte for the strand only); a 16-byte store whose source bytes do not lie in one stored row (it straddles two output rows, or the end of
// the kept rows) gathers its bytes one by one.  "First R rows" is min(kept, R) * L contiguous bytes and zeros behind them.
//
// A store set to the compact format (store_host.h) measures with record_spans instead of record_extent, packs its mergeable
// records with store_pack_compact (the others with store_pack) and, once it holds a compact record, assembles with
// store_assemble<true>, which looks at each site's format; a store of rows records alone keeps store_assemble<false>, the kernel
// above.  The three are described where they stand.
#include "plan_entry.h"
#include "store_device.h"

namespace st {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(1))) U128 { u32x4 v; };   // a 16-byte load at any byte address

__device__ __forceinline__ u32x4 load16_any(const uint8_t* p) { return reinterpret_cast<const U128*>(p)->v; }

__device__ __forceinline__ int head_bytes(const void* p, int span) {
    return min(span, (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u));
}

__global__ __launch_bounds__(STORE_BLOCK) void record_extent(Source src, const int32_t* __restrict__ slots, int32_t* __restrict__ kept) {
    __shared__ int32_t wave_rows[STORE_BLOCK / 64];
    const int tid = threadIdx.x;
    const size_t slot_off = (size_t)slots[blockIdx.x] * (size_t)src.stride;
    const int n = src.S * src.W;
    int rows = 0;                                          // 1 + the last row in which this lane saw a non-zero byte
    for (int p = 0; p < 3; ++p) {
        const uint8_t* q = src.plane[p] + slot_off;
        const int head = head_bytes(q, n);
        const int n16 = (n - head) >> 4;
        const int tail0 = head + (n16 << 4);
        int hi = -1;                                       // the last non-zero byte of this plane this lane saw
        for (int o = tid; o < head; o += STORE_BLOCK)
            if (q[o]) hi = o;
        const u32x4* body = reinterpret_cast<const u32x4*>(q + head);
        for (int j = tid; j < n16; j += STORE_BLOCK) {
            const u32x4 v = body[j];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            for (int k = 3; k >= 0; --k)
                if (w[k]) {
                    hi = head + (j << 4) + 4 * k + ((31 - __clz((int)w[k])) >> 3);
                    break;
                }
        }
        for (int o = tail0 + tid; o < n; o += STORE_BLOCK)
            if (q[o]) hi = max(hi, o);
        if (hi >= 0) rows = max(rows, hi / src.W + 1);
    }
    for (int d = 32; d >= 1; d >>= 1) rows = max(rows, __shfl_xor(rows, d, 64));
    if ((tid & 63) == 0) wave_rows[tid >> 6] = rows;
    __syncthreads();
    if (tid == 0) {
        int m = wave_rows[0];
        for (int k = 1; k < STORE_BLOCK / 64; ++k) m = max(m, wave_rows[k]);
        kept[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(STORE_BLOCK) void store_pack(Source src, const PackItem* __restrict__ items, DevRec* __restrict__ table) {
    const PackItem it = items[blockIdx.x];
    const int plane = blockIdx.y, tid = threadIdx.x;
    const int n = it.kept * src.W;
    if (plane == 0 && tid == 0) table[it.record] = DevRec{it.dst, it.kept, 0};
    if (n == 0) return;
    uint8_t* dst = reinterpret_cast<uint8_t*>(it.dst) + (size_t)plane * n;
    const uint8_t* s = src.plane[plane] + (size_t)it.slot * (size_t)src.stride;
    const int head = head_bytes(dst, n);
    const int n16 = (n - head) >> 4;
    const int tail0 = head + (n16 << 4);
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    for (int o = tid; o < head; o += STORE_BLOCK) dst[o] = s[o];
    for (int j = tid; j < n16; j += STORE_BLOCK) body[j] = load16_any(s + head + (j << 4));
    for (int o = tail0 + tid; o < n; o += STORE_BLOCK) dst[o] = s[o];
    if (plane == 2) {                                      // the record ends at a 16-byte boundary: zeros up to it
        const int pad = (16 - ((3 * n) & 15)) & 15;
        for (int o = tid; o < pad; o += STORE_BLOCK) dst[n + o] = 0;
    }
}

// byte o of a site's [R][L] span of plane p: the stored row of plan entry rows[o / L], zeros where that row was not kept or
// the entry forces this plane to zero (plan_entry.h)
__device__ __forceinline__ uint8_t row_byte(const uint8_t* plane, int kept, const int16_t* rows, int p, int L, int o) {
    const int r = o / L;
    const int row = plan_entry::source_row(rows[r], p);
    return row < kept ? plane[(size_t)row * L + (o - r * L)] : (uint8_t)0;
}

// ---- the compact format (store_host.h): rowtab[kept + 1] | ts[cells] | q[cells] | zeros to the next multiple of 16 -------------
constexpr uint32_t OFF_MASK = 0xFFFFFFu;                   // a rowtab entry: off in bits 0-23, c0 in bits 24-31

struct __attribute__((packed, aligned(1))) U32 { uint32_t v; };   // a 4-byte load at any byte address
__device__ __forceinline__ uint32_t load4_any(const uint8_t* p) { return reinterpret_cast<const U32*>(p)->v; }

// One wave per row, lane l the columns 4l .. 4l + 3 (W <= 255: one round): a 4-byte load per plane where the four columns lie
// inside the row, bytes one by one in the lane that holds the row's end -- no load reaches past the row it measures.  The lanes'
// first and last non-zero columns are reduced by shuffles; lane 0 writes the row's span.  kept, cells and the mergeable flag are
// summed per wave, then over the four waves through LDS.
__global__ __launch_bounds__(STORE_BLOCK) void record_spans(Source src, const int32_t* __restrict__ slots, SpanSums* __restrict__ sums,
                                                            uint16_t* __restrict__ rowspans) {
    __shared__ int32_t wave_kept[STORE_BLOCK / 64], wave_cells[STORE_BLOCK / 64], wave_bad[STORE_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slot_off = (size_t)slots[blockIdx.x] * (size_t)src.stride;
    const uint8_t* a = src.plane[0] + slot_off;
    const uint8_t* q = src.plane[1] + slot_off;
    const uint8_t* b = src.plane[2] + slot_off;
    const int W = src.W, c = 4 * lane;
    uint16_t* out = rowspans + (size_t)blockIdx.x * src.S;
    int kept = 0, cells = 0;
    uint32_t bad = 0;                                      // bits 4-7 of any byte of the reads or strand plane this lane saw
    for (int r = wave; r < src.S; r += STORE_BLOCK / 64) {
        const size_t o = (size_t)r * W + c;
        uint32_t x = 0, y = 0, z = 0;
        if (c + 4 <= W) {
            x = load4_any(a + o); y = load4_any(q + o); z = load4_any(b + o);
        } else {
            for (int k = 0; c + k < W; ++k) {
                x |= (uint32_t)a[o + k] << (8 * k); y |= (uint32_t)q[o + k] << (8 * k); z |= (uint32_t)b[o + k] << (8 * k);
            }
        }
        bad |= (x | z) & 0xF0F0F0F0u;
        const uint32_t nz = x | y | z;
        int lo = 256, hi = -1;
        if (nz) {
            lo = c + ((__ffs((int)nz) - 1) >> 3);
            hi = c + ((31 - __clz((int)nz)) >> 3);
        }
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d, 64));
            hi = max(hi, __shfl_xor(hi, d, 64));
        }
        const int n = hi < 0 ? 0 : hi - lo + 1;
        if (lane == 0) out[r] = (uint16_t)(n ? lo | n << 8 : 0);
        if (n) kept = r + 1;                               // (rows ascend within a wave)
        cells += n;
    }
    const int any_bad = __any(bad != 0);
    if (lane == 0) {
        wave_kept[wave] = kept; wave_cells[wave] = cells; wave_bad[wave] = any_bad;
    }
    __syncthreads();
    if (tid == 0) {
        SpanSums t{0, 0, 1, 0};
        for (int k = 0; k < STORE_BLOCK / 64; ++k) {
            t.kept = max(t.kept, wave_kept[k]);
            t.cells += wave_cells[k];
            if (wave_bad[k]) t.mergeable = 0;
        }
        sums[blockIdx.x] = t;
    }
}

// the row of a compact record that holds a cell, followed from cell to cell in ascending order
struct CellWalk {
    const uint32_t* rowtab;
    int kept, row;
    uint32_t off, next, c0;                                // of row: its first cell, the first cell behind it, its first column
};

// the last row r < kept with off_r <= cell (off_0 = 0, and off_kept = cells > cell)
__device__ __forceinline__ void seek(CellWalk& w, uint32_t cell) {
    int lo = 0, hi = w.kept;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((w.rowtab[mid] & OFF_MASK) <= cell) lo = mid; else hi = mid;
    }
    const uint32_t e = w.rowtab[lo];
    w.row = lo; w.off = e & OFF_MASK; w.c0 = e >> 24; w.next = w.rowtab[lo + 1] & OFF_MASK;
}

// byte p of what follows a compact record's rowtab: ts[cells] | q[cells] | zeros
__device__ __forceinline__ uint32_t packed_byte(const Source& src, const uint8_t* a, const uint8_t* q, const uint8_t* b, CellWalk& w, int& kind,
                                                int cells, int p) {
    if (p >= 2 * cells) return 0;
    const int k = p >= cells;
    const uint32_t cell = (uint32_t)(p - k * cells);
    if (k != kind) {
        seek(w, cell);
        kind = k;
    }
    while (cell >= w.next && w.row + 1 < w.kept) {         // (rows without a cell are passed over)
        const uint32_t e = w.rowtab[++w.row];
        w.off = w.next; w.c0 = e >> 24; w.next = w.rowtab[w.row + 1] & OFF_MASK;
    }
    const size_t i = (size_t)w.row * src.W + min(w.c0 + (cell - w.off), (uint32_t)src.W - 1u);
    return k ? (uint32_t)q[i] : (uint32_t)(uint8_t)(a[i] | b[i] << 4);
}

// One workgroup per record.  Pass 1 scans the spans record_spans wrote (four consecutive rows per lane, 1024 per round: the
// lanes' sums by shuffles, the waves' through LDS, a carry from round to round) and writes rowtab with aligned 16-byte stores,
// the entries of an incomplete last group one by one.  Pass 2 writes ts | q | pad as one span behind rowtab, cut at the 16-byte
// boundaries of the destination: every lane finds the row of its first cell by bisection in the rowtab just written (the
// barrier between the passes makes it visible to the workgroup) and walks on from there.  Every store lies inside
// [dst, dst + bytes): rowtab takes 4 (kept + 1) <= bytes, and pass 2 ends at bytes.
__global__ __launch_bounds__(STORE_BLOCK) void store_pack_compact(Source src, const PackItem* __restrict__ items,
                                                                  const uint16_t* __restrict__ rowspans, DevRec* __restrict__ table) {
    __shared__ uint32_t wave_sum[STORE_BLOCK / 64];
    const PackItem it = items[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) table[it.record] = DevRec{it.dst, it.kept, FORMAT_COMPACT};
    const int kept = it.kept, cells = it.cells;
    if (kept == 0 || it.bytes < 4 * (kept + 1)) return;
    uint8_t* dst = reinterpret_cast<uint8_t*>(it.dst);
    uint32_t* rowtab = reinterpret_cast<uint32_t*>(dst);
    const uint16_t* sp = rowspans + (size_t)it.entry * src.S;
    uint32_t carry = 0;
    for (int base = 0; base <= kept; base += 4 * STORE_BLOCK) {
        const int r0 = base + 4 * tid;
        uint32_t n[4], c0[4], sum = 0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t v = r0 + k < kept ? sp[r0 + k] : 0u;
            c0[k] = v & 255u; n[k] = v >> 8;
            sum += n[k];
        }
        uint32_t inc = sum;                                // the inclusive sum over the lanes of the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t off = carry + inc - sum, total = 0;
        for (int k = 0; k < STORE_BLOCK / 64; ++k) {
            if (k < wave) off += wave_sum[k];
            total += wave_sum[k];
        }
        __syncthreads();                                   // (wave_sum is written again in the next round)
        carry += total;
        uint32_t e[4];
        for (int k = 0; k < 4; ++k) {
            e[k] = min(off, (uint32_t)cells) | c0[k] << 24;
            off += n[k];
        }
        if (r0 + 3 <= kept) {
            *reinterpret_cast<u32x4*>(rowtab + r0) = u32x4{e[0], e[1], e[2], e[3]};
        } else {
            for (int k = 0; k < 4; ++k)
                if (r0 + k <= kept) rowtab[r0 + k] = e[k];
        }
    }
    __syncthreads();
    const uint8_t* a = src.plane[0] + (size_t)it.slot * (size_t)src.stride;
    const uint8_t* q = src.plane[1] + (size_t)it.slot * (size_t)src.stride;
    const uint8_t* b = src.plane[2] + (size_t)it.slot * (size_t)src.stride;
    const int first = 4 * (kept + 1), span = it.bytes - first;
    uint8_t* out = dst + first;
    const int head = head_bytes(out, span);
    const int n16 = (span - head) >> 4;
    const int tail0 = head + (n16 << 4);
    u32x4* body = reinterpret_cast<u32x4*>(out + head);
    CellWalk w{rowtab, kept, 0, 0u, 0u, 0u};
    int kind = -1;
    for (int o = tid; o < head; o += STORE_BLOCK) {
        kind = -1;
        out[o] = (uint8_t)packed_byte(src, a, q, b, w, kind, cells, o);
    }
    for (int j = tid; j < n16; j += STORE_BLOCK) {
        const int o = head + (j << 4);
        kind = -1;
        uint32_t v[4];
        for (int k = 0; k < 4; ++k) {
            uint32_t x = 0;
            for (int i = 0; i < 4; ++i) x |= packed_byte(src, a, q, b, w, kind, cells, o + 4 * k + i) << (8 * i);
            v[k] = x;
        }
        body[j] = u32x4{v[0], v[1], v[2], v[3]};
    }
    for (int o = tail0 + tid; o < span; o += STORE_BLOCK) {
        kind = -1;
        out[o] = (uint8_t)packed_byte(src, a, q, b, w, kind, cells, o);
    }
}

// plane 0 = ts & 15, 1 = q, 2 = ts >> 4
__device__ __forceinline__ uint32_t decode4(uint32_t x, int plane) {
    return plane == 0 ? x & 0x0F0F0F0Fu : plane == 2 ? (x >> 4) & 0x0F0F0F0Fu : x;
}

// byte o of a site's [R][L] span from a compact record (cell: ts, or q for plane 1); rows == nullptr: the first rows
__device__ __forceinline__ uint32_t compact_byte(const uint32_t* rowtab, const uint8_t* cell, int kept, int plane, const int16_t* rows, int L,
                                                 int o) {
    const int r = o / L, c = o - r * L;
    const int row = rows ? plan_entry::source_row(rows[r], plane) : r;
    if (row >= kept) return 0;
    const uint32_t e = rowtab[row], off = e & OFF_MASK, n = (rowtab[row + 1] & OFF_MASK) - off;
    const uint32_t j = (uint32_t)(c - (int)(e >> 24));
    return j < n ? decode4(cell[off + j], plane) : 0u;
}

// store_assemble's span of one (site, plane) from a compact record: the same cut at the destination's 16-byte boundaries, every
// output byte written by exactly one lane.  A 16-byte store that lies in one output row takes its row's rowtab entries once:
// inside the row's span it is one 16-byte load of the cells at their own alignment and a mask or a shift, outside it zeros, across
// an end of the span bytes one by one; a store that straddles output rows gathers every byte by itself.
__device__ __forceinline__ void assemble_compact(uint8_t* dst, int head, int n16, int tail0, int span, const DevRec& rec, int plane,
                                                 const int16_t* rows, int L) {
    const int tid = threadIdx.x, kept = rec.kept;
    const uint32_t* rowtab = reinterpret_cast<const uint32_t*>(rec.addr);
    const uint32_t cells = kept ? rowtab[kept] & OFF_MASK : 0u;
    const uint8_t* cell = reinterpret_cast<const uint8_t*>(rec.addr) + 4 * ((size_t)kept + 1) + (plane == 1 ? cells : 0u);
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    for (int o = tid; o < head; o += STORE_BLOCK) dst[o] = (uint8_t)compact_byte(rowtab, cell, kept, plane, rows, L, o);
    for (int j = tid; j < n16; j += STORE_BLOCK) {
        const int o = head + (j << 4);
        const int r = o / L, c = o - r * L;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (c + 16 <= L) {
            const int row = rows ? plan_entry::source_row(rows[r], plane) : r;
            if (row < kept) {
                const uint32_t e = rowtab[row], off = e & OFF_MASK;
                const int n = (int)((rowtab[row + 1] & OFF_MASK) - off);
                const int k0 = c - (int)(e >> 24);         // the store's first byte is cell k0 of the row
                if (k0 >= 0 && k0 + 16 <= n) {
                    const u32x4 x = load16_any(cell + off + k0);
                    v = u32x4{decode4(x.x, plane), decode4(x.y, plane), decode4(x.z, plane), decode4(x.w, plane)};
                } else if (k0 + 16 > 0 && k0 < n) {        // an end of the row's span lies inside the store
                    uint32_t w[4];
                    for (int k = 0; k < 4; ++k) {
                        uint32_t x = 0;
                        for (int i = 0; i < 4; ++i) {
                            const int t = k0 + 4 * k + i;
                            if (t >= 0 && t < n) x |= (uint32_t)cell[off + t] << (8 * i);
                        }
                        w[k] = decode4(x, plane);
                    }
                    v = u32x4{w[0], w[1], w[2], w[3]};
                }
            }
        } else {                                           // the store straddles two (L < 16: more) output rows
            uint32_t w[4];
            for (int k = 0; k < 4; ++k) {
                uint32_t x = 0;
                for (int i = 0; i < 4; ++i) x |= compact_byte(rowtab, cell, kept, plane, rows, L, o + 4 * k + i) << (8 * i);
                w[k] = x;
            }
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        body[j] = v;
    }
    for (int o = tail0 + tid; o < span; o += STORE_BLOCK) dst[o] = (uint8_t)compact_byte(rowtab, cell, kept, plane, rows, L, o);
}

// MIXED == false is the kernel of a store that holds rows records only: the format of a site's record is not looked at.
template <bool MIXED>
__global__ __launch_bounds__(STORE_BLOCK) void store_assemble(AssembleArgs a) {
    const int site = blockIdx.x, plane = blockIdx.y, tid = threadIdx.x;
    const int span = a.R * a.L;
    uint8_t* dst = a.dst[plane] + (size_t)site * span;
    const int head = head_bytes(dst, span);
    const int n16 = (span - head) >> 4;                    // aligned 16-byte stores
    const int tail0 = head + (n16 << 4);
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    if (!a.use[plane]) {
        for (int o = tid; o < head; o += STORE_BLOCK) dst[o] = 0;
        for (int j = tid; j < n16; j += STORE_BLOCK) body[j] = zero;
        for (int o = tail0 + tid; o < span; o += STORE_BLOCK) dst[o] = 0;
        return;
    }
    const pg::SiteSrc s = a.sites[site];
    const DevRec rec = a.table[s.slot];
    const int kept = rec.kept, L = a.L;
    if constexpr (MIXED) {
        if (rec.format == FORMAT_COMPACT) {
            assemble_compact(dst, head, n16, tail0, span, rec, plane, s.first_rows ? nullptr : a.rows + (size_t)site * a.R, L);
            return;
        }
    }
    const uint8_t* src = reinterpret_cast<const uint8_t*>(rec.addr) + (size_t)plane * kept * L;
    if (s.first_rows) {
        const int nv = min(kept, a.R) * L;                 // bytes that come from the store; zeros behind them
        for (int o = tid; o < head; o += STORE_BLOCK) dst[o] = o < nv ? src[o] : (uint8_t)0;
        for (int j = tid; j < n16; j += STORE_BLOCK) {
            const int o = head + (j << 4);
            u32x4 v = zero;
            if (o + 16 <= nv) {
                v = load16_any(src + o);
            } else if (o < nv) {                           // the store straddles the end of the kept rows
                uint32_t w[4];
                for (int k = 0; k < 4; ++k) {
                    uint32_t x = 0;
                    for (int b = 0; b < 4; ++b) {
                        const int i = o + 4 * k + b;
                        x |= (uint32_t)(i < nv ? src[i] : (uint8_t)0) << (8 * b);
                    }
                    w[k] = x;
                }
                v = u32x4{w[0], w[1], w[2], w[3]};
            }
            body[j] = v;
        }
        for (int o = tail0 + tid; o < span; o += STORE_BLOCK) dst[o] = o < nv ? src[o] : (uint8_t)0;
        return;
    }
    const int16_t* rows = a.rows + (size_t)site * a.R;
    for (int o = tid; o < head; o += STORE_BLOCK) dst[o] = row_byte(src, kept, rows, plane, L, o);
    for (int j = tid; j < n16; j += STORE_BLOCK) {
        const int o = head + (j << 4);
        const int r = o / L, c = o - r * L;
        u32x4 v = zero;
        if (c + 16 <= L) {
            const int row = plan_entry::source_row(rows[r], plane);
            if (row < kept) v = load16_any(src + (size_t)row * L + c);
        } else {                                           // the store straddles two (L < 16: more) output rows
            uint32_t w[4];
            for (int k = 0; k < 4; ++k) {
                uint32_t x = 0;
                for (int b = 0; b < 4; ++b) x |= (uint32_t)row_byte(src, kept, rows, plane, L, o + 4 * k + b) << (8 * b);
                w[k] = x;
            }
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        body[j] = v;
    }
    for (int o = tail0 + tid; o < span; o += STORE_BLOCK) dst[o] = row_byte(src, kept, rows, plane, L, o);
}

}  // namespace

hipError_t launch_extent(const Source& src, const int32_t* slots, int64_t n, int32_t* kept, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(record_extent, dim3((unsigned)n), dim3(STORE_BLOCK), 0, s, src, slots, kept);
    return hipGetLastError();
}

hipError_t launch_pack(const Source& src, const PackItem* items, int64_t n, DevRec* table, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(store_pack, dim3((unsigned)n, 3), dim3(STORE_BLOCK), 0, s, src, items, table);
    return hipGetLastError();
}

hipError_t launch_spans(const Source& src, const int32_t* slots, int64_t n, SpanSums* sums, uint16_t* rowspans, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(record_spans, dim3((unsigned)n), dim3(STORE_BLOCK), 0, s, src, slots, sums, rowspans);
    return hipGetLastError();
}

hipError_t launch_pack_compact(const Source& src, const PackItem* items, int64_t n, const uint16_t* rowspans, DevRec* table, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(store_pack_compact, dim3((unsigned)n), dim3(STORE_BLOCK), 0, s, src, items, rowspans, table);
    return hipGetLastError();
}

hipError_t launch_store_assemble(const AssembleArgs& a, int32_t m, bool any_compact, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (any_compact) hipLaunchKernelGGL(store_assemble<true>, dim3((unsigned)m, 3), dim3(STORE_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(store_assemble<false>, dim3((unsigned)m, 3), dim3(STORE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace st
