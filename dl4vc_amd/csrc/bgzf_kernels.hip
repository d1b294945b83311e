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
// boundaries (one thread per segment), each record is framed by the frame core of bam_frame.h (one thread per slot), and
// listed once per subregion it overlaps, at the place an exclusive scan of the per-record counts gives it.
#include "bgzf_device.h"
#include "device_buffer.h"

#include <rocprim/device/device_scan.hpp>

namespace bz {
namespace {

namespace F = bamn::frame;
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
    if (sg.start > sg.stop || sg.stop > total) { report(err, sg.start, F::W_OVER_STOP); return; }
    const uint64_t cap = (sg.stop - sg.start) / 36 + 1;
    uint64_t at = sg.start, k = 0;
    while (at < sg.stop) {                                  // (each turn advances at by at least 36)
        uint32_t size;
        if (const uint32_t why = F::next_record(infl, total, sg.stop, at, size)) { report(err, at, why); return; }
        if (k >= cap || sg.slot_base + k >= n_slots) { report(err, at, F::W_OVER_STOP); return; }
        rec_off[sg.slot_base + k] = at;
        ++k;
        at += (uint64_t)size + 4;
    }
    atomicAdd(n_records, (unsigned long long)k);
}

// the record's overlap with a subregion (htslib's rule); fr holds the CIGAR sums
__device__ inline bool belongs(const F::Framed& fr, const SubRange& s) {
    return fr.tid == s.tid && fr.pos < s.end && F::endpos(fr) > (int64_t)s.start;
}

// One thread per slot: frames the record there (if any) and counts the subregions it belongs to.  With a sample rule (threshold
// != 0) a record the rule drops belongs to none, after it has been framed and checked like every other; *seen then gathers the
// memberships in front of the rule, one atomic add per workgroup.  With `census` (given when the read filter is on or the read
// stats were asked for; filter = exclude | require << 16) the workgroup counts its memberships in LDS in front of the filter, a
// record the filter drops belongs to no subregion, and the rule and *seen come behind the filter.
__global__ void bam_frame_kernel(const uint8_t* __restrict__ infl, const uint64_t* __restrict__ rec_off, uint64_t n_slots,
                                 const SubRange* __restrict__ subs, uint32_t n_subs, uint32_t* __restrict__ count,
                                 int32_t* __restrict__ md_off, int32_t* __restrict__ md_len, unsigned long long* __restrict__ err,
                                 uint32_t sample_seed, uint32_t sample_threshold, unsigned long long* __restrict__ seen,
                                 uint32_t filter, uint32_t min_mapq, unsigned long long* __restrict__ census) {
    __shared__ uint32_t s_seen;
    __shared__ uint32_t s_cen[F::CENSUS_WORDS];
    const bool on = sample_threshold != 0;                  // (uniform)
    const bool cen = census != nullptr;                     // (uniform)
    if (on || cen) {
        if (threadIdx.x == 0) s_seen = 0;
        if (cen) F::census_clear(s_cen);
        __syncthreads();
    }
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots) {
        uint32_t c = 0;
        const uint64_t at = rec_off[i];
        if (at != NO_RECORD) {
            const uint32_t size = F::ld32(infl + at);       // (checked by the walk: 32 <= size, at + 4 + size <= total)
            const uint8_t* b = infl + at + 4;
            F::Framed fr;
            const uint32_t why = F::frame_record(b, size, fr);
            if (why != F::W_NONE) {
                report(err, at, why);
            } else {
                F::cigar_sums(b, fr);
                for (uint32_t s = 0; s < n_subs; ++s) c += belongs(fr, subs[s]) ? 1u : 0u;
                md_off[i] = fr.md_off;
                md_len[i] = fr.md_len;
                if (cen && c) {
                    const F::ReadFilter flt{(uint16_t)filter, (uint16_t)(filter >> 16), (uint8_t)min_mapq};
                    if (!F::census_count(s_cen, b, fr, flt, c)) c = 0;
                }
                if (on && c) {
                    atomicAdd(&s_seen, c);
                    if (!F::sampled(b, fr, F::SampleRule{sample_seed, sample_threshold})) c = 0;
                }
                if (cen && c) atomicAdd(&s_cen[F::CENSUS_KEPT], c);
            }
        }
        count[i] = c;
    }
    if (on || cen) {
        __syncthreads();
        if (on && threadIdx.x == 0 && s_seen) atomicAdd(seen, (unsigned long long)s_seen);
        if (cen) F::census_flush(s_cen, census);
    }
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
    const uint32_t size = F::ld32(infl + at);
    F::Framed fr;
    (void)F::frame_record(b, size, fr, false);              // (framed cleanly by bam_frame_kernel)
    F::cigar_sums(b, fr);
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

}  // namespace

hipError_t launch_inflate(const uint8_t* comp, const BlockDesc* tab, int64_t n, uint8_t* out, int32_t* status, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3((unsigned)n), dim3(WAVE), 0, stream, comp, tab, n, out, status);
    return hipGetLastError();
}

struct Framer {
    dev::Buffer segs, subs, rec_off, count, first, md_off, md_len, meta, scalars, temp;
};

Framer* framer_create() { return new Framer(); }
void framer_destroy(Framer* f) { delete f; }

int walk_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs, uint64_t n_segs, uint64_t n_slots,
                 hipStream_t stream, const uint64_t** rec_off, uint64_t* n_records, uint64_t* err, const char** msg) {
    *rec_off = nullptr; *n_records = 0; *err = NO_ERROR;
    if (n_segs == 0 || n_slots == 0) return 0;
    if (n_slots >= (1ull << 31)) { *msg = "too many record slots in one batch"; return -2; }
    HIP_CHECK_MSG(f->segs.ensure(n_segs * sizeof(Segment)));
    HIP_CHECK_MSG(f->rec_off.ensure(n_slots * 8));
    HIP_CHECK_MSG(f->scalars.ensure((3 + F::CENSUS_WORDS) * 8));
    // [0] records walked, [1] first refused record, [2] frame_records: seen, [3, 3 + CENSUS_WORDS): frame_records: the read census
    unsigned long long* sc = f->scalars.as<unsigned long long>();
    HIP_CHECK_MSG(hipMemcpyAsync(f->segs.p, segs, n_segs * sizeof(Segment), hipMemcpyHostToDevice, stream));
    HIP_CHECK_MSG(hipMemsetAsync(f->rec_off.p, 0xff, n_slots * 8, stream));
    HIP_CHECK_MSG(hipMemsetAsync(sc, 0, 8, stream));
    HIP_CHECK_MSG(hipMemsetAsync(sc + 1, 0xff, 8, stream));
    hipLaunchKernelGGL(bam_walk_kernel, dim3((unsigned)((n_segs + 63) / 64)), dim3(64), 0, stream, infl, infl_bytes,
                       f->segs.as<const Segment>(), n_segs, n_slots, f->rec_off.as<uint64_t>(), sc, sc + 1);
    HIP_CHECK_MSG(hipGetLastError());
    unsigned long long h[2];
    HIP_CHECK_MSG(hipMemcpyAsync(h, sc, 16, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipStreamSynchronize(stream));
    *n_records = h[0];
    *err = h[1];                                           // (a refused walk leaves slots unset: nothing is framed from them)
    *rec_off = f->rec_off.as<const uint64_t>();
    return 0;
}

int frame_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs, uint64_t n_segs, uint64_t n_slots,
                  const SubRange* subs, uint32_t n_subs, hipStream_t stream, const cand::ReadMeta** meta, uint64_t* n_reads,
                  uint64_t* n_records, uint64_t* err, const char** msg, F::SampleRule rule, uint64_t* n_seen, F::ReadFilter filter,
                  F::Census* census) {
    *meta = nullptr; *n_reads = 0; *n_records = 0; *err = NO_ERROR;
    if (n_seen) *n_seen = 0;
    if (n_segs == 0 || n_slots == 0) return 0;
    const int TB = 256;
    const uint64_t* walked = nullptr;
    if (const int rc = walk_records(f, infl, infl_bytes, segs, n_segs, n_slots, stream, &walked, n_records, err, msg)) return rc;
    if (*err != NO_ERROR) return 0;
    HIP_CHECK_MSG(f->subs.ensure((n_subs + 1) * sizeof(SubRange)));
    HIP_CHECK_MSG(f->count.ensure((n_slots + 1) * 4));
    HIP_CHECK_MSG(f->first.ensure((n_slots + 1) * 4));
    HIP_CHECK_MSG(f->md_off.ensure(n_slots * 4));
    HIP_CHECK_MSG(f->md_len.ensure(n_slots * 4));
    unsigned long long* sc = f->scalars.as<unsigned long long>();
    unsigned long long h[3 + F::CENSUS_WORDS];
    const bool cen = census != nullptr || F::filter_on(filter);
    HIP_CHECK_MSG(hipMemcpyAsync(f->subs.p, subs, n_subs * sizeof(SubRange), hipMemcpyHostToDevice, stream));
    HIP_CHECK_MSG(hipMemsetAsync(sc + 2, 0, cen ? (1 + F::CENSUS_WORDS) * 8 : 8, stream));
    const unsigned grid = (unsigned)((n_slots + TB - 1) / TB);
    hipLaunchKernelGGL(bam_frame_kernel, dim3(grid), dim3(TB), 0, stream, infl, f->rec_off.as<const uint64_t>(), n_slots,
                       f->subs.as<const SubRange>(), n_subs, f->count.as<uint32_t>(), f->md_off.as<int32_t>(), f->md_len.as<int32_t>(),
                       sc + 1, rule.seed, rule.threshold, sc + 2, (uint32_t)filter.exclude | (uint32_t)filter.require << 16,
                       (uint32_t)filter.min_mapq, cen ? sc + 3 : nullptr);
    HIP_CHECK_MSG(hipGetLastError());
    HIP_CHECK_MSG(hipMemsetAsync(f->count.as<uint32_t>() + n_slots, 0, 4, stream));
    size_t tb = 0;
    HIP_CHECK_MSG(rocprim::exclusive_scan(nullptr, tb, f->count.as<uint32_t>(), f->first.as<uint32_t>(), 0u, (size_t)n_slots + 1,
                                          rocprim::plus<uint32_t>(), stream));
    HIP_CHECK_MSG(f->temp.ensure(tb));
    tb = f->temp.cap;
    HIP_CHECK_MSG(rocprim::exclusive_scan(f->temp.p, tb, f->count.as<uint32_t>(), f->first.as<uint32_t>(), 0u, (size_t)n_slots + 1,
                                          rocprim::plus<uint32_t>(), stream));
    uint32_t total = 0;
    HIP_CHECK_MSG(hipMemcpyAsync(&total, f->first.as<uint32_t>() + n_slots, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipMemcpyAsync(h, sc, cen ? sizeof(h) : 24, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipStreamSynchronize(stream));
    if (h[1] != NO_ERROR) { *err = h[1]; return 0; }
    if (n_seen) *n_seen = rule.threshold ? h[2] : total;
    if (census && cen)
        for (int k = 0; k < F::CENSUS_WORDS; ++k) census->w[k] += h[3 + k];
    HIP_CHECK_MSG(f->meta.ensure(((size_t)total + 1) * sizeof(cand::ReadMeta)));
    if (total) {
        hipLaunchKernelGGL(bam_emit_kernel, dim3(grid), dim3(TB), 0, stream, infl, f->rec_off.as<const uint64_t>(), n_slots,
                           f->subs.as<const SubRange>(), n_subs, f->count.as<const uint32_t>(), f->first.as<const uint32_t>(),
                           f->md_off.as<const int32_t>(), f->md_len.as<const int32_t>(), f->meta.as<cand::ReadMeta>());
        HIP_CHECK_MSG(hipGetLastError());
    }
    *meta = f->meta.as<const cand::ReadMeta>();
    *n_reads = total;
    return 0;
}

}  // namespace bz
