// The record store of the candidate file's device loader (cl_store_*): the records of a training file, inflated once, kept in
// device memory trimmed of their trailing all-zero rows, and the sites of every batch assembled from there.  The CPU twins of the
// three kernels are in store_host.h; store_capi.cpp checks every index before a launch.
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
// kept is zeros; a 16-byte store whose source bytes do not lie in one stored row (it straddles two output rows, or the end of
// the kept rows) gathers its bytes one by one.  "First R rows" is min(kept, R) * L contiguous bytes and zeros behind them.
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

// byte o of a site's [R][L] span: stored row rows[o / L], zeros where that row was not kept
__device__ __forceinline__ uint8_t row_byte(const uint8_t* plane, int kept, const int16_t* rows, int L, int o) {
    const int r = o / L;
    const int row = rows[r];
    return row < kept ? plane[(size_t)row * L + (o - r * L)] : (uint8_t)0;
}

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
    for (int o = tid; o < head; o += STORE_BLOCK) dst[o] = row_byte(src, kept, rows, L, o);
    for (int j = tid; j < n16; j += STORE_BLOCK) {
        const int o = head + (j << 4);
        const int r = o / L, c = o - r * L;
        u32x4 v = zero;
        if (c + 16 <= L) {
            const int row = rows[r];
            if (row < kept) v = load16_any(src + (size_t)row * L + c);
        } else {                                           // the store straddles two (L < 16: more) output rows
            uint32_t w[4];
            for (int k = 0; k < 4; ++k) {
                uint32_t x = 0;
                for (int b = 0; b < 4; ++b) x |= (uint32_t)row_byte(src, kept, rows, L, o + 4 * k + b) << (8 * b);
                w[k] = x;
            }
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        body[j] = v;
    }
    for (int o = tail0 + tid; o < span; o += STORE_BLOCK) dst[o] = row_byte(src, kept, rows, L, o);
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

hipError_t launch_store_assemble(const AssembleArgs& a, int32_t m, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(store_assemble, dim3((unsigned)m, 3), dim3(STORE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace st
