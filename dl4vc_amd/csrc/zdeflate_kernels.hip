// Kernels of the device compressor (zdeflate_device.h): the candidate records of an HDF5 chunk packed into the compound layout,
// compressed into zlib streams (zdeflate.h, one lane per segment), and the streams placed one behind the other.  wave64, gfx950.
#include "device_buffer.h"
#include "zdeflate_device.h"

#include <rocprim/device/device_scan.hpp>

namespace zd {

namespace {

__device__ __forceinline__ uint8_t pack_byte(const PackArgs& a, int64_t rec, uint32_t o) {
    if (rec >= a.n_records) return 0;
    const uint8_t* blob = a.blob + (size_t)rec * (a.head + a.mid);
    if (o < a.head) return blob[o];
    o -= a.head;
    const size_t slot = (size_t)a.slots[rec] * a.plane;
    if (o < a.plane) return a.planes[0][slot + o];
    o -= a.plane;
    if (o < a.mid) return blob[a.head + o];
    o -= a.mid;
    if (o < a.plane) return a.planes[1][slot + o];
    return a.planes[2][slot + (o - a.plane)];          // (o - plane < plane: o was below the item size)
}

// One thread per 8 output bytes (the image is 8-byte aligned and a multiple of 8 long): every byte has this one writer.
__global__ __launch_bounds__(COPY_BLOCK) void hdf_pack_kernel(PackArgs a, uint64_t n_words, uint64_t* image) {
    const uint64_t t = (uint64_t)blockIdx.x * COPY_BLOCK + threadIdx.x;
    if (t >= n_words) return;
    const uint32_t itemsize = a.head + a.mid + 3 * a.plane;
    int64_t rec = (int64_t)(t * 8 / itemsize);
    uint32_t o = (uint32_t)(t * 8 % itemsize);
    uint64_t v = 0;
    for (int k = 0; k < 8; ++k) {
        v |= (uint64_t)pack_byte(a, rec, o) << (8 * k);
        if (++o == itemsize) {
            o = 0;
            ++rec;
        }
    }
    image[t] = v;
}

// One lane per segment; segment g of the launch is segment k = g % spc of chunk g / spc.
__global__ __launch_bounds__(DEFLATE_BLOCK) void zd_deflate_kernel(const uint8_t* in, uint64_t chunk_bytes, uint32_t spc, uint64_t n_segs,
                                                                   uint32_t seg, int reversed, uint8_t* tmp, uint32_t tmp_stride,
                                                                   uint32_t* seg_size, uint32_t* seg_adler) {
    __shared__ uint16_t heads[HASH_SIZE * DEFLATE_BLOCK];       // entry h of lane t: heads[h * DEFLATE_BLOCK + t]
    uint64_t g = (uint64_t)blockIdx.x * DEFLATE_BLOCK + threadIdx.x;
    if (g >= n_segs) return;
    if (reversed) g = n_segs - 1 - g;
    const uint64_t chunk = g / spc;
    const uint32_t k = (uint32_t)(g % spc);
    const uint64_t off = (uint64_t)k * seg;
    const uint32_t len = (uint32_t)(chunk_bytes - off < seg ? chunk_bytes - off : seg);
    const uint8_t* src = in + chunk * chunk_bytes + off;
    seg_adler[g] = adler32(src, len);
    seg_size[g] = deflate_segment(src, len, k + 1 == spc, tmp + g * tmp_stride, heads + threadIdx.x, DEFLATE_BLOCK);
}

// The same mapping in dynamic mode (ZD_DYNAMIC): a lane counts its segment's symbols, builds its three codes and parses again to
// emit.  The hash heads and the counts, which become the code tables, lie in LDS interleaved by lane (118 528 bytes: one workgroup
// per CU); the code construction's array is the lane's own (scratch), touched between the two parses only.
__global__ __launch_bounds__(DEFLATE_BLOCK) void zd_deflate_dyn_kernel(const uint8_t* in, uint64_t chunk_bytes, uint32_t spc, uint64_t n_segs,
                                                                       uint32_t seg, int reversed, uint8_t* tmp, uint32_t tmp_stride,
                                                                       uint32_t* seg_size, uint32_t* seg_adler, uint8_t* seg_kind) {
    __shared__ uint16_t heads[HASH_SIZE * DEFLATE_BLOCK];       // entry h of lane t: heads[h * DEFLATE_BLOCK + t]
    __shared__ uint32_t work[WORK_SIZE * DEFLATE_BLOCK];        // entry e of lane t: work[e * DEFLATE_BLOCK + t]
    uint32_t build[BUILD_SIZE];
    uint64_t g = (uint64_t)blockIdx.x * DEFLATE_BLOCK + threadIdx.x;
    if (g >= n_segs) return;
    if (reversed) g = n_segs - 1 - g;
    const uint64_t chunk = g / spc;
    const uint32_t k = (uint32_t)(g % spc);
    const uint64_t off = (uint64_t)k * seg;
    const uint32_t len = (uint32_t)(chunk_bytes - off < seg ? chunk_bytes - off : seg);
    const uint8_t* src = in + chunk * chunk_bytes + off;
    int kind = KIND_FIXED;
    seg_adler[g] = adler32(src, len);
    seg_size[g] = deflate_segment_dynamic(src, len, k + 1 == spc, tmp + g * tmp_stride, heads + threadIdx.x, DEFLATE_BLOCK,
                                          work + threadIdx.x, DEFLATE_BLOCK, build, &kind);
    seg_kind[g] = (uint8_t)kind;
}

// One thread per chunk: its segments' offsets, the stream's size, Adler-32 and "store"; out_size is what the gather places.
__global__ __launch_bounds__(COPY_BLOCK) void zd_finish_kernel(uint64_t chunk_bytes, uint32_t spc, uint32_t seg, int64_t n_chunks,
                                                               int raw_on_store, const uint32_t* seg_size, const uint32_t* seg_adler,
                                                               uint64_t* seg_off, uint64_t* out_size, uint32_t* adlers, uint8_t* store) {
    const int64_t c = (int64_t)blockIdx.x * COPY_BLOCK + threadIdx.x;
    if (c >= n_chunks) return;
    const StreamInfo r = finish_stream(chunk_bytes, seg, seg_size + c * spc, seg_adler + c * spc, seg_off + c * spc);
    out_size[c] = r.store && raw_on_store ? chunk_bytes : r.size;
    adlers[c] = r.adler;
    store[c] = (uint8_t)r.store;
}

// Block (k, chunk): segment k's bytes to their place behind the chunk's header; block (spc, chunk): header and Adler-32.  A
// "store" chunk under raw_on_store: block k copies the segment's raw bytes instead.  Every output byte has one writer.
__global__ __launch_bounds__(COPY_BLOCK) void zd_gather_kernel(const uint8_t* in, uint64_t chunk_bytes, uint32_t spc, uint32_t seg,
                                                               int raw_on_store, const uint8_t* tmp, uint32_t tmp_stride,
                                                               const uint32_t* seg_size, const uint64_t* seg_off, const uint64_t* chunk_off,
                                                               const uint32_t* adlers, const uint8_t* store, uint8_t* out) {
    const uint64_t c = blockIdx.y;
    const uint32_t k = blockIdx.x;
    uint8_t* dst = out + chunk_off[c];
    const bool raw = raw_on_store && store[c];
    if (k == spc) {
        if (raw || threadIdx.x >= 6) return;
        const uint64_t g = c * spc + spc - 1;
        const uint64_t end = 2 + seg_off[g] + seg_size[g];
        const uint32_t a = adlers[c];
        if (threadIdx.x == 0) dst[0] = ZLIB_CMF;
        else if (threadIdx.x == 1) dst[1] = ZLIB_FLG;
        else dst[end + (threadIdx.x - 2)] = (uint8_t)(a >> (8 * (5 - threadIdx.x)));       // big-endian
        return;
    }
    const uint64_t g = c * spc + k;
    const uint8_t* src;
    uint64_t n;
    if (raw) {
        const uint64_t off = (uint64_t)k * seg;
        src = in + c * chunk_bytes + off;
        n = chunk_bytes - off < seg ? chunk_bytes - off : seg;
        dst += off;
    } else {
        src = tmp + g * tmp_stride;
        n = seg_size[g];
        dst += 2 + seg_off[g];
    }
    for (uint64_t i = threadIdx.x; i < n; i += COPY_BLOCK) dst[i] = src[i];
}

}  // namespace

struct Ctx {
    dev::Buffer tmp;
    dev::Array<uint32_t> seg_size, seg_adler;
    dev::Array<uint64_t> seg_off, out_size, chunk_off;
    dev::Array<uint32_t> adlers;
    dev::Buffer store, scan;
    dev::Buffer seg_kind;                                       // dynamic mode only
};

Ctx* ctx_create() { return new Ctx(); }

void ctx_destroy(Ctx* c) { delete c; }

hipError_t launch_pack(const PackArgs& a, uint64_t image_bytes, uint8_t* image, hipStream_t s) {
    const uint64_t n_words = image_bytes / 8;
    if (!n_words) return hipSuccess;
    hipLaunchKernelGGL(hdf_pack_kernel, dim3((unsigned)((n_words + COPY_BLOCK - 1) / COPY_BLOCK)), dim3(COPY_BLOCK), 0, s, a, n_words,
                       (uint64_t*)image);
    return hipGetLastError();
}

int run(Ctx* c, const uint8_t* in, uint64_t chunk_bytes, int64_t n_chunks, uint32_t seg, bool reversed, bool raw_on_store, bool dynamic,
        uint8_t* out, hipStream_t s, hipEvent_t mid, Streams* res, const char** msg) {
    static thread_local char text[256];
    auto bad = [&](const char* what, hipError_t e) {
        snprintf(text, sizeof text, "%s: %s", what, hipGetErrorString(e));
        *msg = text;
        return -2;
    };
    const uint64_t spc64 = n_segments(chunk_bytes, seg);
    const uint64_t n_segs = spc64 * (uint64_t)n_chunks;
    if (n_chunks < 1 || n_chunks > 65535 || seg < MIN_SEG || seg > MAX_SEG || chunk_bytes > MAX_STREAM || n_segs > (1ull << 30)) {
        *msg = "zd::run: shape outside the kernels' limits";
        return -2;
    }
    const uint32_t spc = (uint32_t)spc64;
    const uint32_t tmp_stride = seg_cap(seg);
    if (c->tmp.ensure((size_t)n_segs * tmp_stride) || c->seg_size.ensure((size_t)n_segs) || c->seg_adler.ensure((size_t)n_segs) ||
        c->seg_off.ensure((size_t)n_segs) || c->out_size.ensure((size_t)n_chunks) || c->chunk_off.ensure((size_t)n_chunks) ||
        c->adlers.ensure((size_t)n_chunks) || c->store.ensure((size_t)n_chunks) || (dynamic && c->seg_kind.ensure((size_t)n_segs))) {
        *msg = "zd::run: hipMalloc failed";
        return -2;
    }
    size_t scan_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, scan_bytes, c->out_size.p, c->chunk_off.p, (uint64_t)0, (size_t)n_chunks, rocprim::plus<uint64_t>(), s);
    if (e != hipSuccess) return bad("rocprim::exclusive_scan (size)", e);
    if (c->scan.ensure(scan_bytes + 16)) {
        *msg = "zd::run: hipMalloc failed";
        return -2;
    }
    const dim3 deflate_grid((unsigned)((n_segs + DEFLATE_BLOCK - 1) / DEFLATE_BLOCK));
    if (dynamic)
        hipLaunchKernelGGL(zd_deflate_dyn_kernel, deflate_grid, dim3(DEFLATE_BLOCK), 0, s, in, chunk_bytes, spc, n_segs, seg, reversed ? 1 : 0,
                           c->tmp.p, tmp_stride, c->seg_size.p, c->seg_adler.p, c->seg_kind.p);
    else
        hipLaunchKernelGGL(zd_deflate_kernel, deflate_grid, dim3(DEFLATE_BLOCK), 0, s, in, chunk_bytes, spc, n_segs, seg, reversed ? 1 : 0,
                           c->tmp.p, tmp_stride, c->seg_size.p, c->seg_adler.p);
    if ((e = hipGetLastError()) != hipSuccess) return bad(dynamic ? "zd_deflate_dyn_kernel" : "zd_deflate_kernel", e);
    if (mid && (e = hipEventRecord(mid, s)) != hipSuccess) return bad("hipEventRecord", e);
    hipLaunchKernelGGL(zd_finish_kernel, dim3((unsigned)((n_chunks + COPY_BLOCK - 1) / COPY_BLOCK)), dim3(COPY_BLOCK), 0, s, chunk_bytes, spc, seg,
                       n_chunks, raw_on_store ? 1 : 0, c->seg_size.p, c->seg_adler.p, c->seg_off.p, c->out_size.p, c->adlers.p, c->store.p);
    if ((e = hipGetLastError()) != hipSuccess) return bad("zd_finish_kernel", e);
    e = rocprim::exclusive_scan(c->scan.p, scan_bytes, c->out_size.p, c->chunk_off.p, (uint64_t)0, (size_t)n_chunks, rocprim::plus<uint64_t>(), s);
    if (e != hipSuccess) return bad("rocprim::exclusive_scan", e);
    hipLaunchKernelGGL(zd_gather_kernel, dim3(spc + 1, (unsigned)n_chunks), dim3(COPY_BLOCK), 0, s, in, chunk_bytes, spc, seg,
                       raw_on_store ? 1 : 0, c->tmp.p, tmp_stride, c->seg_size.p, c->seg_off.p, c->chunk_off.p, c->adlers.p, c->store.p, out);
    if ((e = hipGetLastError()) != hipSuccess) return bad("zd_gather_kernel", e);
    *res = Streams{c->chunk_off.p, c->out_size.p, c->adlers.p, c->store.p, dynamic ? c->seg_kind.p : nullptr, n_segs};
    return 0;
}

}  // namespace zd
