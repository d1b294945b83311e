// Site assembly of libdl4vc_pileup.so (pg_assemble_device): the stored planes [n][S][L] the encoder left in device memory ->
// the planes [m][R][L] the forward reads, compacted over the locations that gave a record, R chosen rows per site.  A slot's plane
// starts slot_stride bytes after the one before: S * L for the encoder's planes, the record size where the planes lie inside the
// inflated records of a candidate file (cl_assemble_device).
//
// One workgroup copies one plane of one site: a span of R * L output bytes.  Rows are L = 2 w + 1 bytes (201), so neither a row
// nor a site slab starts on a 16-byte boundary.  The span is cut at the 16-byte boundaries of the DESTINATION: the bytes before
// the first boundary and after the last one are written one by one, everything between as aligned 16-byte stores, each output
// byte by exactly one lane.  The 16 source bytes of a body store lie in one source row for all but one store in L / 16; they are
// read with one 16-byte load at the source's own (arbitrary) alignment.  A store that straddles two output rows gathers its bytes
// one by one.  "First R rows" is the same code with the whole span as one row of R * L bytes: no store straddles, the copy is
// one contiguous stream.  A plane the model does not use is zero-filled by the same head / body / tail split.  A row whose plan
// entry carries the zero-reads bit (plan_entry.h) is zeros in the reads plane and the stored row in the other two.
//
// center_counts (cl_center_counts_device): the read tokens of an assembled reads plane [m][R][L] counted at the two columns the
// training targets look at (alleles.count_center_support: the centre column and the one after it).  One 64-lane wave per site:
// lane i takes rows i, i + 64, ..., adds its two tokens to 2 x 16 integer counters in LDS, and lanes 0..31 write the counters out,
// every output element once.  Integer adds in LDS: the counts do not depend on the order the lanes arrive in.
#include "pileup_device.h"
#include "plan_entry.h"

namespace pg {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(1))) U128 { u32x4 v; };   // a 16-byte load at any byte address

__device__ __forceinline__ u32x4 load16_any(const uint8_t* p) { return reinterpret_cast<const U128*>(p)->v; }

// (plan_entry.h: the reads plane of a row whose plan entry carries the zero-reads bit is zeros)
__device__ __forceinline__ uint8_t gather_byte(const uint8_t* slab, const int16_t* rows, int plane, int L, int o) {
    const int r = o / L;
    const int row = plan_entry::source_row(rows[r], plane);
    return row == plan_entry::NO_ROW ? (uint8_t)0 : slab[(size_t)row * L + (o - r * L)];
}

__global__ __launch_bounds__(ASSEMBLE_BLOCK) void assemble_planes(AssembleArgs a) {
    const int site = blockIdx.x, plane = blockIdx.y;
    const int span = a.R * a.L;
    uint8_t* dst = a.dst[plane] + (size_t)site * span;
    const int head = min(span, (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u));
    const int n16 = (span - head) >> 4;                    // aligned 16-byte stores
    const int tail0 = head + (n16 << 4);
    u32x4* body = reinterpret_cast<u32x4*>(dst + head);
    if (!a.use[plane]) {
        for (int o = threadIdx.x; o < head; o += ASSEMBLE_BLOCK) dst[o] = 0;
        for (int j = threadIdx.x; j < n16; j += ASSEMBLE_BLOCK) body[j] = u32x4{0u, 0u, 0u, 0u};
        for (int o = tail0 + threadIdx.x; o < span; o += ASSEMBLE_BLOCK) dst[o] = 0;
        return;
    }
    const SiteSrc s = a.sites[site];
    const uint8_t* slab = a.src[plane] + (size_t)s.slot * (size_t)a.slot_stride;
    if (s.first_rows) {
        for (int o = threadIdx.x; o < head; o += ASSEMBLE_BLOCK) dst[o] = slab[o];
        for (int j = threadIdx.x; j < n16; j += ASSEMBLE_BLOCK) body[j] = load16_any(slab + head + (j << 4));
        for (int o = tail0 + threadIdx.x; o < span; o += ASSEMBLE_BLOCK) dst[o] = slab[o];
        return;
    }
    const int16_t* rows = a.rows + (size_t)site * a.R;
    const int L = a.L;
    for (int o = threadIdx.x; o < head; o += ASSEMBLE_BLOCK) dst[o] = gather_byte(slab, rows, plane, L, o);
    for (int j = threadIdx.x; j < n16; j += ASSEMBLE_BLOCK) {
        const int o = head + (j << 4);
        const int r = o / L, c = o - r * L;
        u32x4 v;
        if (c + 16 <= L) {
            const int row = plan_entry::source_row(rows[r], plane);
            v = row == plan_entry::NO_ROW ? u32x4{0u, 0u, 0u, 0u} : load16_any(slab + (size_t)row * L + c);
        } else {                                           // the store straddles two (L < 16: more) output rows
            uint32_t w[4];
            for (int k = 0; k < 4; ++k) {
                uint32_t x = 0;
                for (int b = 0; b < 4; ++b) x |= (uint32_t)gather_byte(slab, rows, plane, L, o + 4 * k + b) << (8 * b);
                w[k] = x;
            }
            v = u32x4{w[0], w[1], w[2], w[3]};
        }
        body[j] = v;
    }
    for (int o = tail0 + threadIdx.x; o < span; o += ASSEMBLE_BLOCK) dst[o] = gather_byte(slab, rows, plane, L, o);
}

__global__ __launch_bounds__(COUNTS_BLOCK) void center_counts(const uint8_t* __restrict__ reads, int R, int L, int col,
                                                              int32_t* __restrict__ counts) {
    __shared__ int32_t cnt[2 * COUNT_TOKENS];
    const int lane = threadIdx.x;
    if (lane < 2 * COUNT_TOKENS) cnt[lane] = 0;
    __syncthreads();
    const uint8_t* site = reads + (size_t)blockIdx.x * (size_t)R * (size_t)L + col;
    for (int r = lane; r < R; r += COUNTS_BLOCK) {
        const uint8_t a = site[(size_t)r * L], b = site[(size_t)r * L + 1];
        if (a < COUNT_TOKENS) atomicAdd(&cnt[a], 1);
        if (b < COUNT_TOKENS) atomicAdd(&cnt[COUNT_TOKENS + b], 1);
    }
    __syncthreads();
    if (lane < 2 * COUNT_TOKENS) counts[(size_t)blockIdx.x * (2 * COUNT_TOKENS) + lane] = cnt[lane];
}

}  // namespace

hipError_t launch_center_counts(const uint8_t* reads, int64_t m, int32_t R, int32_t L, int32_t col, int32_t* counts, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(center_counts, dim3((unsigned)m), dim3(COUNTS_BLOCK), 0, s, reads, R, L, col, counts);
    return hipGetLastError();
}

hipError_t launch_assemble(const AssembleArgs& a, int32_t m, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(assemble_planes, dim3((unsigned)m, 3), dim3(ASSEMBLE_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace pg
