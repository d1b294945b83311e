// Framing for the GPU pileup encoder when the BAM is inflated on the device (pg_set_inflate_device; gfx950).  The inflate and the
// record walk are bgzf_kernels.hip's; these kernels turn the walked record slots into what the encode kernels read:
//   pileup_frame_kernel   one thread per record slot: the checks of the frame core (bam_frame.h, the text the host path runs),
//                         then the runs the record belongs to, found by binary search in the run table (sorted by tid and start;
//                         the runs' stops rise with their starts, so they are neighbours);
//   pileup_pair_kernel    one (run, slot) pair per membership, at the place an exclusive scan of the counts gives it; a stable
//                         radix sort on the run id then makes them run-major, in file order inside a run;
//   pileup_emit_kernel    one thread per pair: its pg::Rec, its reference length, and the ends of each run's record range;
//   pileup_run_kernel     one workgroup per run: res (the exclusive scan of the reference lengths), the run's longest reference
//                         span and whether its positions never decrease;
//   pileup_locate_kernel  one thread per location: the two lower bounds that give Loc::first and Loc::last.
// Every output element has one writer; the only atomic is the integer minimum on the error word (lowest offset wins).
#include "device_buffer.h"
#include "pileup_device.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace pg {
namespace {

namespace F = pg::frame;
constexpr int TB = 256;

__device__ inline void report(unsigned long long* err, uint64_t off, uint32_t why) {
    atomicMin(err, (unsigned long long)((off << 8) | why));
}

// With a sample rule (sample_threshold != 0, bam_frame.h) a record the rule drops belongs to no run, after it has been framed
// and checked like every other; *seen then gathers the memberships in front of the rule, one atomic add per workgroup.  With
// `census` (given when the read filter is on or the read stats were asked for; filter = exclude | require << 16) the workgroup
// counts its memberships in LDS in front of the filter, a record the filter drops belongs to no run, and the rule and *seen come
// behind the filter.
__global__ void __launch_bounds__(TB) pileup_frame_kernel(const uint8_t* __restrict__ infl, const uint64_t* __restrict__ rec_off,
                                                          uint32_t n_slots, const RunDesc* __restrict__ runs, int32_t n_runs,
                                                          uint32_t* __restrict__ count, int32_t* __restrict__ first_run,
                                                          unsigned long long* __restrict__ err, uint32_t sample_seed,
                                                          uint32_t sample_threshold, unsigned long long* __restrict__ seen,
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
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots) {
        uint32_t c = 0;
        int32_t k0 = 0;
        const uint64_t at = rec_off[i];
        if (at != F::NO_RECORD) {
            const uint32_t size = F::ld32(infl + at);       // (checked by the walk: 32 <= size, at + 4 + size <= total)
            const uint8_t* b = infl + at + 4;
            F::Framed fr;
            uint32_t why = F::frame_record(b, size, fr);
            if (why == F::W_NONE && fr.tid >= 0) {
                why = F::walk_cigar(b, fr);
                if (why != F::W_NONE) {                     // an error only for a contig some run asks for (the host meets no other)
                    int32_t lo = 0, hi = n_runs;
                    while (lo < hi) {
                        const int32_t mid = (lo + hi) >> 1;
                        if (runs[mid].tid < fr.tid) lo = mid + 1; else hi = mid;
                    }
                    if (lo >= n_runs || runs[lo].tid != fr.tid) why = F::W_NONE;
                } else {
                    // the first run of the contig that stops after the record's start
                    int32_t lo = 0, hi = n_runs;
                    while (lo < hi) {
                        const int32_t mid = (lo + hi) >> 1;
                        const RunDesc r = runs[mid];
                        if (r.tid < fr.tid || (r.tid == fr.tid && r.stop <= (int64_t)fr.pos)) lo = mid + 1; else hi = mid;
                    }
                    k0 = lo;
                    for (int32_t k = lo; k < n_runs; ++k) {
                        const RunDesc r = runs[k];
                        if (!F::keeps(fr, r.tid, r.s0, r.stop)) break;
                        ++c;
                    }
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
            if (why != F::W_NONE) report(err, at, why);
        }
        count[i] = c;
        first_run[i] = k0;
    }
    if (on || cen) {
        __syncthreads();
        if (on && threadIdx.x == 0 && s_seen) atomicAdd(seen, (unsigned long long)s_seen);
        if (cen) F::census_flush(s_cen, census);
    }
}

__global__ void __launch_bounds__(TB) pileup_pair_kernel(uint32_t n_slots, const uint32_t* __restrict__ count,
                                                         const uint32_t* __restrict__ first, const int32_t* __restrict__ first_run,
                                                         uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t c = count[i], f = first[i];
    for (uint32_t j = 0; j < c; ++j) {
        keys[f + j] = (uint32_t)first_run[i] + j;
        vals[f + j] = i;
    }
}

__global__ void __launch_bounds__(TB) pileup_emit_kernel(const uint8_t* __restrict__ infl, const uint64_t* __restrict__ rec_off,
                                                         const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                         uint32_t n_pairs, Rec* __restrict__ recs, unsigned long long* __restrict__ nref,
                                                         int32_t* __restrict__ rec0, int32_t* __restrict__ rec1) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const uint64_t at = rec_off[vals[p]];
    const uint8_t* b = infl + at + 4;
    F::Framed fr;
    (void)F::frame_record(b, F::ld32(infl + at), fr, false);   // (framed cleanly by pileup_frame_kernel)
    (void)F::walk_cigar(b, fr);
    F::fill_rec(fr, at + 4, 0, recs[p]);
    nref[p] = (unsigned long long)fr.nref;
    const uint32_t run = keys[p];
    if (p == 0 || keys[p - 1] != run) rec0[run] = (int32_t)p;
    if (p + 1 == n_pairs || keys[p + 1] != run) rec1[run] = (int32_t)(p + 1);
}

__global__ void __launch_bounds__(TB) pileup_run_kernel(Rec* __restrict__ recs, const unsigned long long* __restrict__ res,
                                                        const int32_t* __restrict__ rec0, const int32_t* __restrict__ rec1,
                                                        int32_t n_runs, RunOut* __restrict__ out) {
    __shared__ int64_t s_max[TB];
    __shared__ int32_t s_bad[TB];
    const int32_t run = blockIdx.x;
    if (run >= n_runs) return;
    const int32_t a = rec0[run], e = rec1[run];
    int64_t mx = 0;
    int32_t bad = 0;
    for (int32_t p = a + (int32_t)threadIdx.x; p < e; p += TB) {
        const unsigned long long r = res[p];
        recs[p].res = (int32_t)(r < (unsigned long long)INT32_MAX ? r : (unsigned long long)INT32_MAX);
        const int32_t pos = recs[p].pos;
        mx = max(mx, (int64_t)recs[p].end - (int64_t)pos);
        if (p > a && pos < recs[p - 1].pos) bad = 1;
    }
    s_max[threadIdx.x] = mx;
    s_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int s = TB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + s]);
            s_bad[threadIdx.x] |= s_bad[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[run] = RunOut{a, e, s_max[0], s_bad[0] ? 0 : 1, 0};
}

__device__ inline int32_t lower_pos(const Rec* __restrict__ recs, int32_t lo, int32_t hi, int64_t v) {
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)recs[mid].pos < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(TB) pileup_locate_kernel(const Rec* __restrict__ recs, const RunOut* __restrict__ runs, int32_t n_runs,
                                                           const int32_t* __restrict__ loc_run, Loc* __restrict__ locs, int32_t n_locs) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_locs) return;
    const int32_t r = loc_run[i];
    if (r < 0 || r >= n_runs || locs[i].pre >= 0) return;
    const RunOut ro = runs[r];
    if (!ro.sorted) { locs[i].pre = 2; return; }            // (the stable order by clipped start needs sorted records)
    locs[i].first = lower_pos(recs, ro.rec0, ro.rec1, (int64_t)locs[i].s0 - ro.max_nref);
    locs[i].last = lower_pos(recs, ro.rec0, ro.rec1, (int64_t)locs[i].stop);
}

}  // namespace

struct Framing {
    dev::Buffer runs, count, first, first_run, keys, vals, keys2, vals2, recs, nref, res, rec0, rec1, out, err, temp, loc_run;
};

Framing* framing_create() { return new Framing(); }
void framing_destroy(Framing* f) { delete f; }

int frame_runs(Framing* f, const uint8_t* infl, const uint64_t* rec_off, uint64_t n_slots, const RunDesc* runs, int32_t n_runs,
               hipStream_t stream, Rec** recs, int64_t* n_recs, int64_t* n_res, const RunOut** run_out, uint64_t* err, const char** msg,
               F::SampleRule rule, int64_t* n_seen, F::ReadFilter filter, F::Census* census) {
    if (n_seen) *n_seen = 0;
    *recs = nullptr; *n_recs = 0; *n_res = 0; *run_out = nullptr; *err = FRAME_NO_ERROR;
    if (n_runs <= 0) return 0;
    if (n_slots >= (1ull << 31)) { *msg = "too many record slots in one group"; return -2; }
    const uint32_t ns = (uint32_t)n_slots;
    HIP_CHECK_MSG(f->runs.ensure((size_t)n_runs * sizeof(RunDesc)));
    HIP_CHECK_MSG(f->rec0.ensure((size_t)n_runs * 4));
    HIP_CHECK_MSG(f->rec1.ensure((size_t)n_runs * 4));
    HIP_CHECK_MSG(f->out.ensure((size_t)n_runs * sizeof(RunOut)));
    HIP_CHECK_MSG(f->count.ensure(((size_t)ns + 1) * 4));
    HIP_CHECK_MSG(f->first.ensure(((size_t)ns + 1) * 4));
    HIP_CHECK_MSG(f->first_run.ensure(((size_t)ns + 1) * 4));
    // [0] first refused record, [1] memberships in front of the sample rule, [2, 2 + CENSUS_WORDS): the read census
    HIP_CHECK_MSG(f->err.ensure((2 + F::CENSUS_WORDS) * 8));
    const bool cen = census != nullptr || F::filter_on(filter);
    unsigned long long* d_err = f->err.as<unsigned long long>();
    HIP_CHECK_MSG(hipMemcpyAsync(f->runs.p, runs, (size_t)n_runs * sizeof(RunDesc), hipMemcpyHostToDevice, stream));
    HIP_CHECK_MSG(hipMemsetAsync(d_err, 0xff, 8, stream));
    HIP_CHECK_MSG(hipMemsetAsync(d_err + 1, 0, cen ? (1 + F::CENSUS_WORDS) * 8 : 8, stream));
    HIP_CHECK_MSG(hipMemsetAsync(f->rec0.p, 0, (size_t)n_runs * 4, stream));
    HIP_CHECK_MSG(hipMemsetAsync(f->rec1.p, 0, (size_t)n_runs * 4, stream));
    uint32_t total = 0;
    if (ns > 0) {
        const unsigned grid = (ns + TB - 1) / TB;
        hipLaunchKernelGGL(pileup_frame_kernel, dim3(grid), dim3(TB), 0, stream, infl, rec_off, ns, f->runs.as<const RunDesc>(), n_runs,
                           f->count.as<uint32_t>(), f->first_run.as<int32_t>(), d_err, rule.seed, rule.threshold, d_err + 1,
                           (uint32_t)filter.exclude | (uint32_t)filter.require << 16, (uint32_t)filter.min_mapq, cen ? d_err + 2 : nullptr);
        HIP_CHECK_MSG(hipGetLastError());
        HIP_CHECK_MSG(hipMemsetAsync(f->count.as<uint32_t>() + ns, 0, 4, stream));
        size_t tb = 0;
        HIP_CHECK_MSG(rocprim::exclusive_scan(nullptr, tb, f->count.as<uint32_t>(), f->first.as<uint32_t>(), 0u, (size_t)ns + 1,
                                              rocprim::plus<uint32_t>(), stream));
        HIP_CHECK_MSG(f->temp.ensure(tb));
        tb = f->temp.cap;
        HIP_CHECK_MSG(rocprim::exclusive_scan(f->temp.p, tb, f->count.as<uint32_t>(), f->first.as<uint32_t>(), 0u, (size_t)ns + 1,
                                              rocprim::plus<uint32_t>(), stream));
        unsigned long long h_err[2 + F::CENSUS_WORDS] = {0, 0};
        HIP_CHECK_MSG(hipMemcpyAsync(&total, f->first.as<uint32_t>() + ns, 4, hipMemcpyDeviceToHost, stream));
        HIP_CHECK_MSG(hipMemcpyAsync(h_err, d_err, cen ? sizeof(h_err) : 16, hipMemcpyDeviceToHost, stream));
        HIP_CHECK_MSG(hipStreamSynchronize(stream));
        if (h_err[0] != FRAME_NO_ERROR) { *err = h_err[0]; return 0; }
        if (n_seen) *n_seen = rule.threshold ? (int64_t)h_err[1] : (int64_t)total;
        if (census && cen)
            for (int k = 0; k < F::CENSUS_WORDS; ++k) census->w[k] += h_err[2 + k];
        if (total >= (1u << 31)) { *msg = "too many records in one group"; return -2; }
    }
    HIP_CHECK_MSG(f->recs.ensure(((size_t)total + 1) * sizeof(Rec)));
    if (total > 0) {
        const unsigned grid = (ns + TB - 1) / TB, pgrid = (total + TB - 1) / TB;
        HIP_CHECK_MSG(f->keys.ensure((size_t)total * 4));
        HIP_CHECK_MSG(f->vals.ensure((size_t)total * 4));
        HIP_CHECK_MSG(f->keys2.ensure((size_t)total * 4));
        HIP_CHECK_MSG(f->vals2.ensure((size_t)total * 4));
        HIP_CHECK_MSG(f->nref.ensure(((size_t)total + 1) * 8));
        HIP_CHECK_MSG(f->res.ensure(((size_t)total + 1) * 8));
        hipLaunchKernelGGL(pileup_pair_kernel, dim3(grid), dim3(TB), 0, stream, ns, f->count.as<const uint32_t>(), f->first.as<const uint32_t>(),
                           f->first_run.as<const int32_t>(), f->keys.as<uint32_t>(), f->vals.as<uint32_t>());
        HIP_CHECK_MSG(hipGetLastError());
        unsigned bits = 1;
        while (bits < 32 && (1ull << bits) < (unsigned long long)n_runs) ++bits;
        size_t tb = 0;
        HIP_CHECK_MSG(rocprim::radix_sort_pairs(nullptr, tb, f->keys.as<uint32_t>(), f->keys2.as<uint32_t>(), f->vals.as<uint32_t>(),
                                                f->vals2.as<uint32_t>(), (size_t)total, 0, bits, stream));
        HIP_CHECK_MSG(f->temp.ensure(tb));
        tb = f->temp.cap;
        HIP_CHECK_MSG(rocprim::radix_sort_pairs(f->temp.p, tb, f->keys.as<uint32_t>(), f->keys2.as<uint32_t>(), f->vals.as<uint32_t>(),
                                                f->vals2.as<uint32_t>(), (size_t)total, 0, bits, stream));
        hipLaunchKernelGGL(pileup_emit_kernel, dim3(pgrid), dim3(TB), 0, stream, infl, rec_off, f->keys2.as<const uint32_t>(),
                           f->vals2.as<const uint32_t>(), total, f->recs.as<Rec>(), f->nref.as<unsigned long long>(), f->rec0.as<int32_t>(),
                           f->rec1.as<int32_t>());
        HIP_CHECK_MSG(hipGetLastError());
        HIP_CHECK_MSG(hipMemsetAsync(f->nref.as<unsigned long long>() + total, 0, 8, stream));
        tb = 0;
        HIP_CHECK_MSG(rocprim::exclusive_scan(nullptr, tb, f->nref.as<unsigned long long>(), f->res.as<unsigned long long>(), 0ull,
                                              (size_t)total + 1, rocprim::plus<unsigned long long>(), stream));
        HIP_CHECK_MSG(f->temp.ensure(tb));
        tb = f->temp.cap;
        HIP_CHECK_MSG(rocprim::exclusive_scan(f->temp.p, tb, f->nref.as<unsigned long long>(), f->res.as<unsigned long long>(), 0ull,
                                              (size_t)total + 1, rocprim::plus<unsigned long long>(), stream));
    }
    hipLaunchKernelGGL(pileup_run_kernel, dim3((unsigned)n_runs), dim3(TB), 0, stream, f->recs.as<Rec>(), f->res.as<const unsigned long long>(),
                       f->rec0.as<const int32_t>(), f->rec1.as<const int32_t>(), n_runs, f->out.as<RunOut>());
    HIP_CHECK_MSG(hipGetLastError());
    unsigned long long h_res = 0;
    if (total > 0) HIP_CHECK_MSG(hipMemcpyAsync(&h_res, f->res.as<unsigned long long>() + total, 8, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipStreamSynchronize(stream));
    *recs = f->recs.as<Rec>();
    *n_recs = (int64_t)total;
    *n_res = (int64_t)std::min<unsigned long long>(h_res, (unsigned long long)INT64_MAX);
    *run_out = f->out.as<const RunOut>();
    return 0;
}

int locate(Framing* f, const Rec* recs, const RunOut* run_out, int32_t n_runs, const int32_t* loc_run, Loc* locs, int32_t n_locs,
           hipStream_t stream, const char** msg, hipEvent_t uploaded) {
    if (n_locs <= 0) {
        if (uploaded) HIP_CHECK_MSG(hipEventRecord(uploaded, stream));
        return 0;
    }
    HIP_CHECK_MSG(f->loc_run.ensure((size_t)n_locs * 4));
    HIP_CHECK_MSG(hipMemcpyAsync(f->loc_run.p, loc_run, (size_t)n_locs * 4, hipMemcpyHostToDevice, stream));
    if (uploaded) HIP_CHECK_MSG(hipEventRecord(uploaded, stream));
    hipLaunchKernelGGL(pileup_locate_kernel, dim3((unsigned)((n_locs + TB - 1) / TB)), dim3(TB), 0, stream, recs, run_out, n_runs,
                       f->loc_run.as<const int32_t>(), locs, n_locs);
    HIP_CHECK_MSG(hipGetLastError());
    return 0;
}

}  // namespace pg
