// BGZF inflate and BAM record framing on the GPU (gfx950).
//
// bgzf_inflate_kernel: one 64-lane workgroup per BGZF block.  Every lane runs the decode core of bgzf_inflate.h (the text the
// host runs) in step on the same bits, so the symbol decoding costs what one lane's would, and the wave shares the copies:
// lane 0 writes the literals, lane k the bytes k, k + 64, ... of a match or a stored run (WaveWriter).  The Huffman tables and
// the block's whole output window are in LDS, so back-references never touch HBM; then the wave computes the CRC-32 (a slice
// per lane, combined by x^(8n) mod P) and, when the block is good, writes the window out in 16-byte stores.  The window sits at
// the slot's own alignment (out_off & 15), so LDS and global addresses agree modulo 16.  A block that fails writes nothing but
// its status.
//
// bam_walk_kernel / bam_frame_kernel / bam_emit_kernel: record starts are found by following block_size from known record
// boundaries (one thread per segment), each record is framed with the checks of bamn::frame_record (one thread per slot), and
// listed once per subregion it overlaps, at the place an exclusive scan of the per-record counts gives it.
#include "bgzf_device.h"

#include <rocprim/device/device_scan.hpp>

namespace bz {
namespace {

constexpr int WAVE = 64;

// The wave's writes into the LDS window.  All 64 lanes call each method with the same arguments (the decode is uniform).  A match
// byte k comes from out[o - dist + k % dist], which lies before o: no lane reads what another writes in the same copy, also when
// the distance is below the length.  One wave's LDS operations complete in the order they are issued; the barrier (one wave: no
// other to wait for) keeps the compiler from moving a later read of the window above the copy.
struct WaveWriter {
    uint32_t lane;
    __device__ void literal(uint8_t* out, uint32_t o, uint8_t v) const {
        if (lane == 0) out[o] = v;
    }
    __device__ void stored(uint8_t* out, uint32_t o, const uint8_t* src, uint32_t n) const {
        for (uint32_t k = lane; k < n; k += WAVE) out[o + k] = src[k];
        __syncthreads();
    }
    __device__ void match(uint8_t* out, uint32_t o, uint32_t dist, uint32_t n) const {
        __syncthreads();
        const uint8_t* from = out + o - dist;
        if (dist >= n) {
            for (uint32_t k = lane; k < n; k += WAVE) out[o + k] = from[k];
        } else {
            for (uint32_t k = lane; k < n; k += WAVE) out[o + k] = from[k % dist];
        }
        __syncthreads();
    }
};

__global__ __launch_bounds__(WAVE) void bgzf_inflate_kernel(const uint8_t* __restrict__ comp, const BlockDesc* __restrict__ tab,
                                                            int64_t n, uint8_t* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ __align__(16) uint8_t win[MAX_ISIZE + 16];
    __shared__ Tables tables;
    __shared__ uint32_t crc_table[256];
    __shared__ uint32_t lane_crc[WAVE];
    __shared__ int s_status;
    const int64_t blk = blockIdx.x;
    if (blk >= n) return;
    const BlockDesc d = tab[blk];
    if (d.status != BZ_OK || d.isize > MAX_ISIZE) {       // (the host refused it; nothing of it is read)
        if (threadIdx.x == 0) status[blk] = d.status != BZ_OK ? d.status : BZ_BAD_HEADER;
        return;
    }
    const int lane = threadIdx.x;
    const uint32_t shift = (uint32_t)(d.out_off & 15);
    uint8_t* w = win + shift;
    for (int i = lane; i < 256; i += WAVE) crc_table[i] = crc_table_entry((uint32_t)i);
    __syncthreads();
    {
        uint32_t produced;
        const int st = inflate_block(comp + d.body_off, d.body_len, w, d.isize, tables, &produced, WaveWriter{(uint32_t)lane});
        if (lane == 0) s_status = st;
    }
    __syncthreads();
    if (s_status != BZ_OK) {
        if (lane == 0) status[blk] = s_status;
        return;
    }
    // CRC: lane i takes bytes [i * per, min(isize, (i + 1) * per))
    const uint32_t per = (d.isize + WAVE - 1) / WAVE;
    const uint32_t lo = min(d.isize, (uint32_t)lane * per), hi = min(d.isize, lo + per);
    lane_crc[lane] = crc_bytes(crc_table, w + lo, hi - lo);
    __syncthreads();
    if (lane == 0) {
        const uint32_t xp = crc_xpow8(per);
        uint32_t acc = 0;                                   // (the CRC of no bytes)
        for (int i = 0; i < WAVE; ++i) {
            const uint32_t a = min(d.isize, (uint32_t)i * per), b = min(d.isize, a + per);
            if (b == a) break;
            acc = crc_append(acc, lane_crc[i], b - a == per ? xp : crc_xpow8(b - a));
        }
        s_status = acc == d.crc ? BZ_OK : BZ_CRC_MISMATCH;
        status[blk] = s_status;
    }
    __syncthreads();
    if (s_status != BZ_OK) return;
    // out: bytes up to the first 16-byte boundary, whole 16-byte words, the rest
    uint8_t* g = out + d.out_off;
    const uint32_t head = min(d.isize, (16 - shift) & 15);
    if ((uint32_t)lane < head) g[lane] = w[lane];
    const uint32_t words = (d.isize - head) / 16;
    const uint4* src = (const uint4*)(w + head);            // win + shift + head is a multiple of 16, and so is g + head
    uint4* dst = (uint4*)(g + head);
    for (uint32_t i = lane; i < words; i += WAVE) dst[i] = src[i];
    const uint32_t done = head + words * 16;
    if (done + lane < d.isize) g[done + lane] = w[done + lane];
}

__device__ inline uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ inline uint32_t ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ inline void report(unsigned long long* err, uint64_t off, uint32_t reason) {
    atomicMin(err, (unsigned long long)((off << 8) | reason));
}

// One thread per segment: rec_off[slot_base + k] = offset of the k-th record's block_size field.
__global__ void bam_walk_kernel(const uint8_t* __restrict__ infl, uint64_t total, const Segment* __restrict__ segs, uint64_t n_segs,
                                uint64_t n_slots, uint64_t* __restrict__ rec_off, unsigned long long* __restrict__ n_records,
                                unsigned long long* __restrict__ err) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_segs) return;
    const Segment sg = segs[s];
    if (sg.start > sg.stop || sg.stop > total) { report(err, sg.start, R_OVER_STOP); return; }
    const uint64_t cap = (sg.stop - sg.start) / 36 + 1;
    uint64_t at = sg.start, k = 0;
    while (at < sg.stop) {                                  // (each turn advances at by at least 36)
        if (sg.stop - at < 4) { report(err, at, R_OVER_STOP); return; }
        const uint32_t size = ld32(infl + at);
        if (size < 32 || size > (1u << 28)) { report(err, at, R_BLOCK_SIZE); return; }
        if ((uint64_t)size + 4 > total - at) { report(err, at, R_TRUNCATED); return; }
        if ((uint64_t)size + 4 > sg.stop - at) { report(err, at, R_OVER_STOP); return; }
        if (k >= cap || sg.slot_base + k >= n_slots) { report(err, at, R_OVER_STOP); return; }
        rec_off[sg.slot_base + k] = at;
        ++k;
        at += (uint64_t)size + 4;
    }
    atomicAdd(n_records, (unsigned long long)k);
}

__device__ inline int aux_value_size(uint8_t type) {
    switch (type) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return -1;
    }
}

struct Framed {
    int32_t tid, pos, md_off, md_len;
    int64_t endpos;
};

// bamn::frame_record and cand_capi.cpp::endpos on the device; R_NONE or the reason
__device__ uint32_t frame(const uint8_t* __restrict__ b, uint64_t size, Framed& fr) {
    fr.tid = (int32_t)ld32(b);
    fr.pos = (int32_t)ld32(b + 4);
    const uint32_t l_name = b[8];
    const uint32_t n_cig = ld16(b + 12), flag = ld16(b + 14);
    const int32_t l_seq = (int32_t)ld32(b + 16);
    if (l_name < 1) return R_L_NAME;
    if (l_seq < 0) return R_L_SEQ;
    const uint64_t cig = 32 + (uint64_t)l_name;
    if (cig > size) return R_NAME_EXCEEDS;
    const uint64_t seq = cig + 4 * (uint64_t)n_cig;
    if (seq > size) return R_CIGAR_EXCEEDS;
    const uint64_t aux = seq + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (aux > size) return R_SEQ_EXCEEDS;
    fr.md_off = -1; fr.md_len = -1;
    uint64_t o = aux;
    while (o < size) {                                      // (each turn advances o by at least 3)
        if (o + 3 > size) return R_AUX_TAG;
        const bool md = b[o] == 'M' && b[o + 1] == 'D';
        const uint8_t t = b[o + 2];
        o += 3;
        if (t == 'Z' || t == 'H') {
            uint64_t z = o;
            while (z < size && b[z] != 0) ++z;
            if (z >= size) return R_AUX_NUL;
            if (md && t == 'Z' && fr.md_off < 0) { fr.md_off = (int32_t)o; fr.md_len = (int32_t)(z - o); }
            o = z + 1;
        } else if (t == 'B') {
            if (o + 5 > size) return R_AUX_ARRAY;
            const int es = aux_value_size(b[o]);
            const uint32_t n = ld32(b + o + 1);
            if (es < 0) return R_AUX_ARRAY_TYPE;
            if ((uint64_t)n * (uint64_t)es > size - (o + 5)) return R_AUX_ARRAY;
            o += 5 + (uint64_t)n * (uint64_t)es;
        } else {
            const int vs = aux_value_size(t);
            if (vs < 0) return R_AUX_TYPE;
            if (o + (uint64_t)vs > size) return R_AUX_VALUE;
            o += (uint64_t)vs;
        }
    }
    if (flag & 0x4) {
        fr.endpos = (int64_t)fr.pos + 1;
    } else {
        int64_t rlen = 0;
        for (uint32_t i = 0; i < n_cig; ++i) {
            const uint32_t v = ld32(b + cig + 4 * i);
            const int op = v & 0xf;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += v >> 4;
        }
        fr.endpos = (int64_t)fr.pos + (rlen > 0 ? rlen : 1);
    }
    return R_NONE;
}

__device__ inline bool belongs(const Framed& fr, const SubRange& s) {
    return fr.tid == s.tid && fr.pos < s.end && fr.endpos > (int64_t)s.start;
}

// One thread per slot: frames the record there (if any) and counts the subregions it belongs to.
__global__ void bam_frame_kernel(const uint8_t* __restrict__ infl, const uint64_t* __restrict__ rec_off, uint64_t n_slots,
                                 const SubRange* __restrict__ subs, uint32_t n_subs, uint32_t* __restrict__ count,
                                 int32_t* __restrict__ md_off, int32_t* __restrict__ md_len, unsigned long long* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    uint32_t c = 0;
    const uint64_t at = rec_off[i];
    if (at != NO_RECORD) {
        const uint32_t size = ld32(infl + at);              // (checked by the walk: 32 <= size, at + 4 + size <= total)
        Framed fr;
        const uint32_t why = frame(infl + at + 4, size, fr);
        if (why != R_NONE) {
            report(err, at, why);
        } else {
            for (uint32_t s = 0; s < n_subs; ++s) c += belongs(fr, subs[s]) ? 1u : 0u;
            md_off[i] = fr.md_off;
            md_len[i] = fr.md_len;
        }
    }
    count[i] = c;
}

// One thread per slot: the record's entries, one per subregion, at first[i] (the exclusive scan of count).
__global__ void bam_emit_kernel(const uint8_t* __restrict__ infl, const uint64_t* __restrict__ rec_off, uint64_t n_slots,
                                const SubRange* __restrict__ subs, uint32_t n_subs, const uint32_t* __restrict__ count,
                                const uint32_t* __restrict__ first, const int32_t* __restrict__ md_off,
                                const int32_t* __restrict__ md_len, cand::ReadMeta* __restrict__ meta) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots || count[i] == 0) return;
    const uint64_t at = rec_off[i];
    const uint8_t* b = infl + at + 4;
    const uint32_t size = ld32(infl + at);
    Framed fr;
    fr.tid = (int32_t)ld32(b);
    fr.pos = (int32_t)ld32(b + 4);
    const uint32_t l_name = b[8], n_cig = ld16(b + 12), flag = ld16(b + 14);
    int64_t rlen = 0;
    if (!(flag & 0x4))
        for (uint32_t k = 0; k < n_cig; ++k) {
            const uint32_t v = ld32(b + 32 + l_name + 4 * k);
            const int op = v & 0xf;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rlen += v >> 4;
        }
    fr.endpos = (int64_t)fr.pos + (rlen > 0 ? rlen : 1);
    cand::ReadMeta m;
    m.off = at + 4;
    m.len = size;
    m.md_off = md_off[i];
    m.md_len = md_len[i];
    uint32_t k = first[i];
    const uint32_t end = k + count[i];
    for (uint32_t s = 0; s < n_subs && k < end; ++s)
        if (belongs(fr, subs[s])) {
            m.sub = s;
            meta[k++] = m;
        }
}

struct DBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> T* as() const { return (T*)p; }
    ~DBuf() { if (p) (void)hipFree(p); }
};

}  // namespace

const char* reason_text(uint32_t r) {
    static const char* const TEXT[R_COUNT] = {
        "no error",
        "corrupt BAM record (block_size)",
        "truncated BAM record",
        "corrupt BAM record (block_size runs past the next indexed record)",
        "corrupt BAM record (l_read_name)",
        "corrupt BAM record (l_seq)",
        "corrupt BAM record (l_read_name exceeds the record)",
        "corrupt BAM record (n_cigar_op exceeds the record)",
        "corrupt BAM record (l_seq exceeds the record)",
        "corrupt BAM record (aux tag runs past the record)",
        "corrupt BAM record (aux string without its NUL)",
        "corrupt BAM record (aux array runs past the record)",
        "corrupt BAM record (aux array element type)",
        "corrupt BAM record (aux value type)",
        "corrupt BAM record (aux value runs past the record)",
    };
    return r < R_COUNT ? TEXT[r] : "corrupt BAM record";
}

hipError_t launch_inflate(const uint8_t* comp, const BlockDesc* tab, int64_t n, uint8_t* out, int32_t* status, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n), dim3(WAVE), 0, stream, comp, tab, n, out, status);
    return hipGetLastError();
}

struct Framer {
    DBuf segs, subs, rec_off, count, first, md_off, md_len, meta, scalars, temp;
};

Framer* framer_create() { return new Framer(); }
void framer_destroy(Framer* f) { delete f; }

#define BZ_CHECK(x)                                                        \
    do {                                                                   \
        const hipError_t e_ = (x);                                         \
        if (e_ != hipSuccess) { *msg = hipGetErrorString(e_); return -2; } \
    } while (0)

int walk_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs, uint64_t n_segs, uint64_t n_slots,
                 hipStream_t stream, const uint64_t** rec_off, uint64_t* n_records, uint64_t* err, const char** msg) {
    *rec_off = nullptr; *n_records = 0; *err = NO_ERROR;
    if (n_segs == 0 || n_slots == 0) return 0;
    if (n_slots >= (1ull << 31)) { *msg = "too many record slots in one batch"; return -2; }
    BZ_CHECK(f->segs.ensure(n_segs * sizeof(Segment)));
    BZ_CHECK(f->rec_off.ensure(n_slots * 8));
    BZ_CHECK(f->scalars.ensure(2 * 8));
    unsigned long long* sc = f->scalars.as<unsigned long long>();   // [0] records walked, [1] first refused record
    BZ_CHECK(hipMemcpyAsync(f->segs.p, segs, n_segs * sizeof(Segment), hipMemcpyHostToDevice, stream));
    BZ_CHECK(hipMemsetAsync(f->rec_off.p, 0xff, n_slots * 8, stream));
    BZ_CHECK(hipMemsetAsync(sc, 0, 8, stream));
    BZ_CHECK(hipMemsetAsync(sc + 1, 0xff, 8, stream));
    hipLaunchKernelGGL(bam_walk_kernel, dim3((unsigned)((n_segs + 63) / 64)), dim3(64), 0, stream, infl, infl_bytes,
                       f->segs.as<const Segment>(), n_segs, n_slots, f->rec_off.as<uint64_t>(), sc, sc + 1);
    BZ_CHECK(hipGetLastError());
    unsigned long long h[2];
    BZ_CHECK(hipMemcpyAsync(h, sc, 16, hipMemcpyDeviceToHost, stream));
    BZ_CHECK(hipStreamSynchronize(stream));
    *n_records = h[0];
    *err = h[1];                                           // (a refused walk leaves slots unset: nothing is framed from them)
    *rec_off = f->rec_off.as<const uint64_t>();
    return 0;
}

int frame_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs, uint64_t n_segs, uint64_t n_slots,
                  const SubRange* subs, uint32_t n_subs, hipStream_t stream, const cand::ReadMeta** meta, uint64_t* n_reads,
                  uint64_t* n_records, uint64_t* err, const char** msg) {
    *meta = nullptr; *n_reads = 0; *n_records = 0; *err = NO_ERROR;
    if (n_segs == 0 || n_slots == 0) return 0;
    const int TB = 256;
    const uint64_t* walked = nullptr;
    if (const int rc = walk_records(f, infl, infl_bytes, segs, n_segs, n_slots, stream, &walked, n_records, err, msg)) return rc;
    if (*err != NO_ERROR) return 0;
    BZ_CHECK(f->subs.ensure((n_subs + 1) * sizeof(SubRange)));
    BZ_CHECK(f->count.ensure((n_slots + 1) * 4));
    BZ_CHECK(f->first.ensure((n_slots + 1) * 4));
    BZ_CHECK(f->md_off.ensure(n_slots * 4));
    BZ_CHECK(f->md_len.ensure(n_slots * 4));
    unsigned long long* sc = f->scalars.as<unsigned long long>();
    unsigned long long h[2];
    BZ_CHECK(hipMemcpyAsync(f->subs.p, subs, n_subs * sizeof(SubRange), hipMemcpyHostToDevice, stream));
    const unsigned grid = (unsigned)((n_slots + TB - 1) / TB);
    hipLaunchKernelGGL(bam_frame_kernel, dim3(grid), dim3(TB), 0, stream, infl, f->rec_off.as<const uint64_t>(), n_slots,
                       f->subs.as<const SubRange>(), n_subs, f->count.as<uint32_t>(), f->md_off.as<int32_t>(), f->md_len.as<int32_t>(),
                       sc + 1);
    BZ_CHECK(hipGetLastError());
    BZ_CHECK(hipMemsetAsync(f->count.as<uint32_t>() + n_slots, 0, 4, stream));
    size_t tb = 0;
    BZ_CHECK(rocprim::exclusive_scan(nullptr, tb, f->count.as<uint32_t>(), f->first.as<uint32_t>(), 0u, (size_t)n_slots + 1,
                                     rocprim::plus<uint32_t>(), stream));
    BZ_CHECK(f->temp.ensure(tb));
    tb = f->temp.cap;
    BZ_CHECK(rocprim::exclusive_scan(f->temp.p, tb, f->count.as<uint32_t>(), f->first.as<uint32_t>(), 0u, (size_t)n_slots + 1,
                                     rocprim::plus<uint32_t>(), stream));
    uint32_t total = 0;
    BZ_CHECK(hipMemcpyAsync(&total, f->first.as<uint32_t>() + n_slots, 4, hipMemcpyDeviceToHost, stream));
    BZ_CHECK(hipMemcpyAsync(h, sc, 16, hipMemcpyDeviceToHost, stream));
    BZ_CHECK(hipStreamSynchronize(stream));
    if (h[1] != NO_ERROR) { *err = h[1]; return 0; }
    BZ_CHECK(f->meta.ensure(((size_t)total + 1) * sizeof(cand::ReadMeta)));
    if (total) {
        hipLaunchKernelGGL(bam_emit_kernel, dim3(grid), dim3(TB), 0, stream, infl, f->rec_off.as<const uint64_t>(), n_slots,
                           f->subs.as<const SubRange>(), n_subs, f->count.as<const uint32_t>(), f->first.as<const uint32_t>(),
                           f->md_off.as<const int32_t>(), f->md_len.as<const int32_t>(), f->meta.as<cand::ReadMeta>());
        BZ_CHECK(hipGetLastError());
    }
    *meta = f->meta.as<const cand::ReadMeta>();
    *n_reads = total;
    return 0;
}

}  // namespace bz
