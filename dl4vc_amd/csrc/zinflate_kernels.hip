// zlib stream inflate on the GPU (gfx950), for streams longer than a BGZF block: the HDF5 chunks of the candidate dataset.
//
// zi_inflate_kernel: one 64-lane workgroup per stream, the form of bgzf_inflate_kernel.  Every lane runs the decode core of
// bgzf_inflate.h in step on the same bits, and the wave shares the copies: lane 0 writes the literals, lane k the bytes k,
// k + 64, ... of a match, a stored run or a flush.  The output goes through the 64 KiB ring of zinflate.h in LDS, so
// back-references never touch HBM; each completed half leaves in 16-byte stores and enters the Adler-32 (a slice per lane, folded
// by zlib's adler32_combine arithmetic).  A raw chunk is a plain copy.  No atomics; LDS: ring 65 536 + tables 4 416 + 256 + 4.
#include "zinflate_device.h"

namespace zi {
namespace {

constexpr int WAVE = 64;

struct WaveLanes {
    static constexpr uint32_t WIDTH = WAVE;
    __device__ uint32_t lane() const { return threadIdx.x; }
    __device__ void sync() const { __syncthreads(); }
    // (both addresses are multiples of 16: zinflate.h)
    __device__ static void copy16(uint8_t* dst, const uint8_t* src) { *(uint4*)dst = *(const uint4*)src; }
};

__global__ __launch_bounds__(WAVE) void zi_inflate_kernel(const uint8_t* __restrict__ comp, const StreamDesc* __restrict__ tab, int64_t n,
                                                          uint8_t* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ __align__(16) uint8_t ring[RING];
    __shared__ bz::Tables tables;
    __shared__ uint32_t lane_adler[WAVE];
    const int64_t s = blockIdx.x;
    if (s >= n) return;
    const StreamDesc d = tab[s];
    const int st = run_stream(comp, d, out, ring, tables, lane_adler, WaveLanes{});   // (uniform: every lane has the same st)
    if (threadIdx.x == 0) status[s] = st;
}

}  // namespace

hipError_t launch_inflate(const uint8_t* comp, const StreamDesc* tab, int64_t n, uint8_t* out, int32_t* status, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(zi_inflate_kernel, dim3((unsigned)n), dim3(WAVE), 0, stream, comp, tab, n, out, status);
    return hipGetLastError();
}

}  // namespace zi
