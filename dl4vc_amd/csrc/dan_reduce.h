// The two reductions over the read axis behind the segment kernels, once for the three formats y crosses HBM in.  Each of
// dan_kernels.hip, dan_kernels_bf16p.hip and dan_kernels_bf16x.hip instantiates the pair for its own format, so that the object's
// compiler flags hold for its tails too (the bf16x3 object has its own schedule).
//   read mean   pool[site][p][c] = (((+0 + y[site][0]) + y[site][1]) + ...) / R                         (dl4vc/model.py:772)
//   final pool  feat[site][c*L + p] = max_r y, feat[site][C*L + c*L + p] = (y[site][0] + y[site][1] + ...) / R, both from row 0
// fp32 sums in read order (like AvgPool2d on the CPU; model.py:824-839), the division a division; a row the segment kernels
// skipped is read through row_src (dan_kernels.h: the empty-row map), the same rows in the same order.
#pragma once
#include "dan_kernels.h"

namespace dan {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));

// One activation format: a row of y is PLANES planes of [L][CPAD] elements, read as vectors of N; a value is the sum of its planes'
// elements (hi + lo, formed before it is added or compared).  UNROLL = rows in flight per lane.
struct RowsFp32 { typedef v4f vec; static constexpr int N = 4, PLANES = 1, UNROLL = 8; };     // dan_kernels.hip
struct RowsBf16 { typedef bf8 vec; static constexpr int N = 8, PLANES = 1, UNROLL = 8; };     // dan_kernels_bf16p.hip
struct RowsBf16x2 { typedef bf8 vec; static constexpr int N = 8, PLANES = 2, UNROLL = 4; };   // dan_kernels_bf16x.hip (hi, lo)

// the N values at p of a row whose planes lie `plane` vectors apart
template <class F>
__device__ __forceinline__ void load_row(const typename F::vec* p, int plane, float (&f)[F::N]) {
    const typename F::vec v = p[0];
    if constexpr (F::PLANES == 2) {
        const typename F::vec lo = p[plane];
#pragma unroll
        for (int j = 0; j < F::N; ++j) f[j] = (float)v[j] + (float)lo[j];
    } else {
#pragma unroll
        for (int j = 0; j < F::N; ++j) f[j] = (float)v[j];
    }
}

template <class F>
__global__ __launch_bounds__(256) void read_mean_kernel(const typename F::vec* __restrict__ y, v4f* __restrict__ pool, int R, int L,
                                                        const int* __restrict__ row_src) {
    constexpr int N = F::N;
    const int nv = L * (CPAD / N);                             // vectors per plane of a row
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int site = blockIdx.y;
    float sum[N];
#pragma unroll
    for (int j = 0; j < N; ++j) sum[j] = 0.f;
    const int* rs = row_src ? row_src + (size_t)site * R : nullptr;
#pragma unroll F::UNROLL
    for (int r = 0; r < R; ++r) {
        float f[N];
        load_row<F>(y + (size_t)(rs ? rs[r] : site * R + r) * (F::PLANES * nv) + i, nv, f);
#pragma unroll
        for (int j = 0; j < N; ++j) sum[j] += f[j];
    }
    v4f* out = pool + ((size_t)site * nv + i) * (N / 4);
#pragma unroll
    for (int k = 0; k < N / 4; ++k) {
        v4f o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = sum[4 * k + j] / (float)R;
        out[k] = o;
    }
}

// A workgroup = 32 positions of one site (128-byte runs in the feature row): thread = (vector column cv, position pl) in PT / PP
// passes of PP positions, transposed through LDS into the channel-major feature row.
template <class F>
__global__ __launch_bounds__(256) void final_pool_kernel(const typename F::vec* __restrict__ y, float* __restrict__ feat, long long fs,
                                                         int R, int L, int C, const int* __restrict__ row_src) {
    constexpr int N = F::N, CV = CPAD / N, PP = 256 / CV;
    constexpr int PT = 32, PS = PT + 1;
    __shared__ float tmax[CPAD * PS], tavg[CPAD * PS];
    const int pt = blockIdx.x, site = blockIdx.y, tid = threadIdx.x;
    const int cv = tid % CV, pl = tid / CV;
    const int nv = L * CV;
#pragma unroll
    for (int pass = 0; pass < PT / PP; ++pass) {
        const int pp = pass * PP + pl, p = pt * PT + pp;
        float mx[N], sum[N];
#pragma unroll
        for (int j = 0; j < N; ++j) { mx[j] = 0.f; sum[j] = 0.f; }
        if (p < L) {
            const size_t off = (size_t)p * CV + cv;
            const int* rs = row_src ? row_src + (size_t)site * R : nullptr;
            auto row = [&](int r) { return y + (size_t)(rs ? rs[r] : site * R + r) * (F::PLANES * nv) + off; };
            load_row<F>(row(0), nv, mx);
#pragma unroll
            for (int j = 0; j < N; ++j) sum[j] = mx[j];
#pragma unroll F::UNROLL
            for (int r = 1; r < R; ++r) {
                float f[N];
                load_row<F>(row(r), nv, f);
#pragma unroll
                for (int j = 0; j < N; ++j) { mx[j] = fmaxf(mx[j], f[j]); sum[j] += f[j]; }
            }
#pragma unroll
            for (int j = 0; j < N; ++j) sum[j] = sum[j] / (float)R;
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            tmax[(cv * N + j) * PS + pp] = mx[j];
            tavg[(cv * N + j) * PS + pp] = sum[j];
        }
    }
    __syncthreads();
    float* row = feat + (size_t)site * fs;
    for (int idx = tid; idx < CPAD * PT; idx += 256) {
        const int c = idx / PT, pp = idx % PT, p = pt * PT + pp;
        if (c < C && p < L) {
            row[(size_t)c * L + p] = tmax[c * PS + pp];                         // max block first (model.py:833)
            row[(size_t)C * L + (size_t)c * L + p] = tavg[c * PS + pp];
        }
    }
}

template <class F>
void launch_read_mean_t(const void* y, float* pool, int n_sites, int R, int L, const int* row_src, hipStream_t s) {
    const int nv = L * (CPAD / F::N);
    hipLaunchKernelGGL(read_mean_kernel<F>, dim3((nv + 255) / 256, n_sites), dim3(256), 0, s, (const typename F::vec*)y, (v4f*)pool, R, L, row_src);
}

template <class F>
void launch_final_pool_t(const void* y, float* feat, long long fs, int n_sites, int R, int L, int C, const int* row_src,
                         hipStream_t s) {
    hipLaunchKernelGGL(final_pool_kernel<F>, dim3((L + 31) / 32, n_sites), dim3(256), 0, s, (const typename F::vec*)y, feat, fs, R, L, C, row_src);
}

}  // namespace dan
