// Host side of libdl4vc_pileup.so (C ABI: include/dl4vc_pileup_gpu.h).  Locations are sorted by (tid, position) and cut
// into runs; worker threads, each with its own BAM and FASTA handles, fetch every run's records once (BAI linear index; a
// BAM without one gets the same index built by one scan), frame and validate them (the frame core of bam_frame.h), and read
// the run's reference slice as tokens.  The records of a batch of locations go to the device in one pinned buffer; the
// kernels (pileup_kernels.hip) do the rest.  Every extern "C" body catches what it throws: a corrupt file is an error code,
// never an abort.
//
// With pg_set_inflate_device() the host does none of the per-record work: encode_all_device() takes every run's byte ranges from
// the BAI bins (bgzf_plan.h), reads their BGZF blocks as they are into pinned memory, and the device inflates them group of runs
// by group of runs, walks the record chain (bgzf_kernels.hip), frames the records and finds each location's records
// (pileup_frame_kernels.hip); the same resolve / encode kernels follow, reading the records where they lie in the inflated buffer.
//
// pg_compress_records_device() takes the stored planes where pg_encode_device left them: the records are packed into the HDF5
// compound layout, compressed into the dataset's chunks (zdeflate_kernels.hip, zdeflate.h) and only those bytes come back.
#include "../../include/dl4vc_pileup_gpu.h"
#include "assemble_host.h"
#include "bam_native.h"
#include "bgzf_device.h"
#include "device_buffer.h"
#include "fasta_native.h"
#include "pileup_device.h"
#include "pileup_fetch.h"
#include "zdeflate_device.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr int BATCH_LOCS = 512;                          // locations per device batch
constexpr int64_t RUN_GAP = 4096, RUN_SPAN = 1 << 20;    // a run: locations closer than RUN_GAP, at most RUN_SPAN bases
constexpr int MAX_THREADS = 8;
constexpr uint64_t DEFAULT_INFLATED = 256ull << 20;      // inflated bytes of one group of runs (pg_set_inflate_device)

// the converter's token table (dan_pileup.cpp::Tables); REF_UNKNOWN for a character outside it
struct RefTokens {
    uint8_t tok[256];
    RefTokens() {
        memset(tok, pg::REF_UNKNOWN, sizeof tok);
        auto set = [&](const char* cs, uint8_t v) { for (; *cs; ++cs) tok[(uint8_t)*cs] = v; };
        set("Aa", 1); set("TtUu", 2); set("Gg", 3); set("Cc", 4); set("-*NnXx.,", 5); set("e", 7);
        set("?MmKkRrYySsWwBbVvHhDd", 9);
    }
};
const RefTokens RT;

struct Entry {
    int32_t tid, pos1;
    int64_t idx;          // position in the caller's arrays
    int32_t pre;          // -1: encode on the device; 0 / 2: decided here
};

struct Run : pgh::RunRecs {  // (the records a worker fills: bytes, recs, max_nref, nres, sorted, err)
    int64_t e0, e1;       // entries [e0, e1) of the sorted list
    int32_t tid;
    int64_t s0, stop;     // union of the locations' fetch windows
    const char* contig;
    std::vector<uint8_t> ref;    // tokens of [s0, stop), filled by a worker
};

// One host framing thread's file handles, kept for the encoder's life (a FASTA without .fai is scanned once, at pg_open).
struct Worker {
    bamn::BamFile bam;
    fastan::Fasta fasta;
    std::vector<uint8_t> blk;
    pg::frame::Census census;    // the read census of this thread's runs in the call in progress
};

}  // namespace

// (members are destroyed last to first: the buffers and the kernel-side contexts go before the stream they were used on)
struct pg_encoder : pgh::AssembleState {   // (err, device and the staging of pg_assemble_device: assemble_host.h)
    std::string bam_path, fasta_path;
    pe_options opt{};
    bamn::BamFile header;
    fastan::Fasta fasta;
    bamn::Bai bai;
    bool have_bai = false, scanned = false;
    std::vector<std::unique_ptr<Worker>> workers;
    dev::Stream stream;
    dev::Buffer d_buf;
    dev::Array<pg::Rec> d_recs;
    dev::Array<pg::Loc> d_locs;
    dev::Buffer d_ref;
    dev::Array<int32_t> d_qpos, d_indel;
    dev::Buffer d_isdel;
    dev::Buffer d_small;                              // ref [B][W] | num [B] i32 | status [B] i8 (SmallLayout)
    dev::Buffer d_planes;                             // pg_encode: [3][B][max_reads][W]
    dev::Pinned h_buf, h_planes;
    pg_stats st{};                                    // stages of the last encode call
    bool census = false;                              // the call in progress is pg_census: statuses only, no plane is written
    dev::Event ev[4];
    // the device inflate path (pg_set_inflate_device)
    bool inflate_device = false;
    uint64_t max_inflated = DEFAULT_INFLATED;
    bz::InflateStage inflate;
    std::unique_ptr<bz::Framer, void (*)(bz::Framer*)> walker{nullptr, bz::framer_destroy};
    std::unique_ptr<pg::Framing, void (*)(pg::Framing*)> framing{nullptr, pg::framing_destroy};
    // read subsampling (pg_set_subsample): the rule and the counts of the last call
    pg::frame::SampleRule sample{0, 0};
    pg_subsample_stats sst{};
    // read filter and census (pg_set_read_filter, pg_set_read_stats): the census is collected with a filter or when asked for
    pg::frame::ReadFilter filter{0, 0, 0};
    bool read_stats = false;
    pg::frame::Census read_census;
    bool collects() const { return read_stats || pg::frame::filter_on(filter); }
    // pg_compress_records_device: the compressor's buffers, the packed chunk image, the streams, the blob and slots (device and
    // pinned staging), the pinned bytes handed to the caller
    std::unique_ptr<zd::Ctx, void (*)(zd::Ctx*)> zctx{nullptr, zd::ctx_destroy};
    bool compress_dynamic = false;              // pg_set_compress_codes
    std::vector<uint8_t> seg_kind;
    dev::Buffer d_image, d_zout, d_blob;
    dev::Pinned h_blob, h_zout;
    dev::Event zev[5];
    ~pg_encoder() { wait_meta(); }              // (the last assembly may still be reading its staging and the planes)
};

namespace {

template <class... A>
int fail(pg_encoder* h, int code, const char* fmt, A... a) { return capi::failf(h ? h->err : pgh::g_err, code, fmt, a...); }

int get_tid(const bamn::BamFile& b, const std::string& name) {
    auto it = b.tid_of.find(name);
    if (it != b.tid_of.end()) return it->second;
    const std::string alt = name.rfind("chr", 0) == 0 ? name.substr(3) : "chr" + name;
    it = b.tid_of.find(alt);
    return it == b.tid_of.end() ? -1 : it->second;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// A BAM without a BAI: the linear index (the smallest virtual offset of a record overlapping each 16 kbp window) from one scan.
int build_linear_index(pg_encoder* h) {
    bamn::BamFile bam;
    if (!bam.open(h->bam_path)) return fail(h, -3, "%s", bam.err.c_str());
    std::vector<uint8_t> blk;
    h->bai.linear.assign(bam.refs.size(), {});
    for (;;) {
        const int64_t voff = bam.r.tell();
        const int got = bam.next_block(blk);
        if (got == 0) break;
        if (got < 0) return fail(h, -3, "%s (record at virtual offset %lld)", bam.err.c_str(), (long long)voff);
        pg::frame::Framed fr;
        if (const uint32_t why = pg::frame::frame_record(blk.data(), blk.size(), fr))
            return fail(h, -3, "%s (record at virtual offset %lld)", pg::frame::why_text(why), (long long)voff);
        if (fr.tid < 0 || fr.tid >= (int)bam.refs.size() || fr.pos < 0) continue;
        if (const uint32_t why = pg::frame::walk_cigar(blk.data(), fr))
            return fail(h, -3, "%s (record at virtual offset %lld)", pg::frame::why_text(why), (long long)voff);
        const int64_t end = (int64_t)fr.pos + std::max<int64_t>(fr.nref, 1);
        auto& lin = h->bai.linear[fr.tid];
        const size_t w1 = (size_t)((end - 1) >> 14);
        if (lin.size() <= w1) lin.resize(w1 + 1, 0);
        for (size_t w = (size_t)(fr.pos >> 14); w <= w1; ++w) if (!lin[w]) lin[w] = (uint64_t)voff;
    }
    h->have_bai = true;
    return 0;
}

// the run's reference tokens
void fetch_ref(fastan::Fasta& fasta, Run& run) {
    std::string seq;
    fasta.fetch(run.contig, run.s0, run.stop, seq);
    run.ref.resize((size_t)(run.stop - run.s0));
    for (size_t i = 0; i < run.ref.size(); ++i) run.ref[i] = i < seq.size() ? RT.tok[(uint8_t)seq[i]] : 5;
}

// The records of one run (pileup_fetch.h), plus the run's reference tokens.
void fetch_run(pg_encoder* h, Worker* wk, Run& run) {
    fetch_ref(wk->fasta, run);
    pgh::fetch_records(h->bai, wk->bam, wk->blk, run.tid, run.s0, run.stop, run, h->sample, h->filter, h->collects() ? &wk->census : nullptr);
}

// the fetch window of the location at pos1 (1-based): bases [s0, stop), the location's own column at ci
struct Window { int64_t s0, stop; int32_t ci; };
Window loc_window(int32_t pos1, int w) {
    const int64_t s0 = std::max<int64_t>((int64_t)pos1 - (w + 2), 0);
    return Window{s0, (int64_t)pos1 + w + 3, (int32_t)(pos1 - 1 - s0)};
}

// The runs of sorted entries [b0, b1), appended to runs: locations closer than RUN_GAP, at most RUN_SPAN bases, one contig name.
void build_runs(const pe_options& o, const char* const* contigs, const std::vector<Entry>& es, int64_t b0, int64_t b1, std::vector<Run>& runs) {
    const int w = o.window_size;
    const size_t first = runs.size();
    for (int64_t i = b0; i < b1; ++i) {
        const Entry& e = es[i];
        if (e.pre >= 0) continue;
        const Window v = loc_window(e.pos1, w);
        const int64_t s0 = v.s0, stop = v.stop;
        if (runs.size() > first) {
            Run& r = runs.back();
            if (r.e1 == i && r.tid == e.tid && strcmp(r.contig, contigs[e.idx]) == 0 && s0 <= r.stop + RUN_GAP && stop - r.s0 <= RUN_SPAN) {
                r.e1 = i + 1;
                r.stop = std::max(r.stop, stop);
                continue;
            }
        }
        Run r;
        r.e0 = i; r.e1 = i + 1; r.tid = e.tid; r.s0 = s0; r.stop = stop; r.contig = contigs[e.idx];
        runs.push_back(std::move(r));
    }
}

// one worker per thread, file handles opened once per encoder; 0 or an error
int ensure_workers(pg_encoder* h, int nt) {
    while ((int)h->workers.size() < nt) {
        auto wk = std::make_unique<Worker>();
        if (!wk->bam.open(h->bam_path)) return fail(h, -3, "%s", wk->bam.err.c_str());
        wk->fasta.f = fopen(h->fasta_path.c_str(), "rb");
        if (!wk->fasta.f) return fail(h, -3, "cannot open %s", h->fasta_path.c_str());
        wk->fasta.index = h->fasta.index;
        h->workers.push_back(std::move(wk));
    }
    return 0;
}

// job(worker, r) for every r in [r0, r1) on the worker threads; "" or what a job threw
template <class Job>
std::string on_workers(pg_encoder* h, int nt, size_t r0, size_t r1, Job job) {
    std::atomic<size_t> next{r0};
    std::mutex mu;
    std::string job_err;
    auto worker = [&](Worker* wk) {
        try {
            for (;;) {
                const size_t r = next.fetch_add(1);
                if (r >= r1) return;
                job(wk, r);
            }
        } catch (const std::exception& ex) {
            std::lock_guard<std::mutex> lk(mu);
            job_err = std::string("host framing: ") + ex.what();
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < nt && r1 > r0; ++t) pool.emplace_back(worker, h->workers[t].get());
    if (r1 > r0) worker(h->workers[0].get());
    for (auto& t : pool) t.join();
    return job_err;
}

int thread_count(size_t jobs) {
    return std::max(1, std::min<int>({MAX_THREADS, (int)std::max(1u, std::thread::hardware_concurrency()), (int)jobs}));
}

struct Outs {
    uint8_t *reads, *qual, *strand, *ref;
    int32_t* num;
    int8_t* status;
    bool device_planes;   // the planes are the caller's device arrays, written at slot = entry.idx; else the encoder's own, at the
                          // position in the batch, and copied back
};

// where the kernel writes a batch's three planes
struct Planes { uint8_t *R, *Q, *S; };
Planes batch_planes(pg_encoder* h, const Outs& out) {
    const size_t stride = (size_t)h->opt.max_reads * (2 * h->opt.window_size + 1) * BATCH_LOCS;
    uint8_t* own = h->d_planes.p;
    return out.device_planes ? Planes{out.reads, out.qual, out.strand} : Planes{own, own + stride, own + 2 * stride};
}

// d_small of a batch of nb locations: ref [nb][W] at 0 | num [nb] i32 | status [nb] i8
struct SmallLayout {
    size_t num, status, bytes;
    SmallLayout(int64_t nb, int W) : num(((size_t)nb * W + 3) & ~(size_t)3), status(num + (size_t)nb * 4), bytes(status + (size_t)nb) {}
};

// The location table of sorted entries [b0, b0 + nb): slot and pre.  An entry that place_loc() does not reach lies in no run of
// the batch: its status is decided already, or it is declined.
std::vector<pg::Loc> loc_table(const std::vector<Entry>& es, int64_t b0, int64_t nb, bool by_index) {
    std::vector<pg::Loc> locs((size_t)nb);
    for (int64_t i = 0; i < nb; ++i) {
        const Entry& e = es[b0 + i];
        locs[i] = pg::Loc{};
        locs[i].pre = e.pre >= 0 ? e.pre : 2;
        locs[i].slot = by_index ? e.idx : i;
    }
    return locs;
}

// entry e of a run that begins at base run_s0 and whose reference tokens begin at ref0 of the batch's
void place_loc(pg::Loc& L, const Entry& e, int w, int64_t ref0, int64_t run_s0) {
    const Window v = loc_window(e.pos1, w);
    L.s0 = (int32_t)v.s0; L.stop = (int32_t)v.stop; L.ci = v.ci;
    L.ref = ref0 + (v.s0 - run_s0);
    L.pre = e.pre;
}

// Census or encode of the nb locations in d_locs over the records at (buf, recs), then `end` is recorded and the stream waited for
// (also after a failure: the pageable uploads in front have then read their host vectors); begin..end is the stage's time.
hipError_t run_locations(pg_encoder* h, const uint8_t* buf, const pg::Rec* recs, int64_t nb, const Planes& pl, hipEvent_t begin, hipEvent_t end) {
    const pe_options& o = h->opt;
    const int w = o.window_size, W = 2 * w + 1;
    const SmallLayout sl(nb, W);
    const pg::Params P{w, W, o.max_reads, o.max_insert_length, o.max_insert_length_variant};
    hipStream_t s = h->stream;
    int8_t* d_status = (int8_t*)(h->d_small.p + sl.status);
    hipError_t e = h->census ? pg::launch_census(buf, recs, h->d_locs.p, (int32_t)nb, h->d_ref.p, h->d_qpos.p, h->d_indel.p, h->d_isdel.p, P, d_status, s)
                             : pg::launch_encode(buf, recs, h->d_locs.p, (int32_t)nb, h->d_ref.p, h->d_qpos.p, h->d_indel.p, h->d_isdel.p, P, pl.R, pl.Q,
                                                 pl.S, h->d_small.p, (int32_t*)(h->d_small.p + sl.num), d_status, s);
    if (e == hipSuccess) e = hipEventRecord(end, s);
    const hipError_t waited = hipStreamSynchronize(s);
    if (e == hipSuccess) e = waited;
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, begin, end);
    if (e == hipSuccess) (h->census ? h->st.census_ms : h->st.encode_ms) += ms;
    return e;
}

// Encodes sorted entries [b0, b1) on h->stream with the records framed on the host; ref / num / status of the batch are left
// in h->d_small.
int encode_batch(pg_encoder* h, const char* const* contigs, std::vector<Entry>& es, int64_t b0, int64_t b1, const Outs& out) {
    const pe_options& o = h->opt;
    const int w = o.window_size, W = 2 * w + 1;
    const auto t_host = std::chrono::steady_clock::now();
    std::vector<Run> runs;
    build_runs(o, contigs, es, b0, b1, runs);
    // host framing, one run at a time per worker; the workers' file handles are opened once per encoder
    {
        const int nt = thread_count(runs.size());
        if (const int rc = ensure_workers(h, nt)) return rc;
        for (int t = 0; t < nt; ++t) h->workers[t]->census = pg::frame::Census{};
        const std::string job_err = on_workers(h, nt, 0, runs.size(), [&](Worker* wk, size_t r) { fetch_run(h, wk, runs[r]); });
        if (!job_err.empty()) return fail(h, -3, "%s", job_err.c_str());
        if (h->collects())
            for (int t = 0; t < nt; ++t) h->read_census.add(h->workers[t]->census);
        for (auto& r : runs) if (!r.err.empty()) return fail(h, -3, "%s", r.err.c_str());
    }
    // gather
    size_t bytes = 0, n_recs = 0, n_ref = 0;
    int64_t n_res = 0;
    for (auto& r : runs) { bytes += r.bytes.size(); n_recs += r.recs.size(); n_ref += r.ref.size(); n_res += r.nres; }
    if (n_res > INT32_MAX || n_recs > INT32_MAX) return fail(h, -1, "batch too large (%lld reference positions of records)", (long long)n_res);
    if (h->h_buf.ensure(bytes + 4)) return fail(h, -2, "pinned allocation of %zu bytes failed", bytes);
    std::vector<pg::Rec> recs;
    recs.reserve(n_recs);
    std::vector<uint8_t> ref;
    ref.reserve(n_ref);
    const int64_t nb = b1 - b0;
    std::vector<pg::Loc> locs = loc_table(es, b0, nb, out.device_planes);
    size_t at = 0;
    int64_t res = 0;
    for (auto& r : runs) {
        const int32_t rec0 = (int32_t)recs.size();
        const int64_t ref0 = (int64_t)ref.size();
        if (!r.bytes.empty()) memcpy(h->h_buf.p + at, r.bytes.data(), r.bytes.size());
        for (auto m : r.recs) { m.off += at; m.res += (int32_t)res; recs.push_back(m); }   // (res + nres <= INT32_MAX, checked above)
        ref.insert(ref.end(), r.ref.begin(), r.ref.end());
        for (int64_t i = r.e0; i < r.e1; ++i) {
            pg::Loc& L = locs[i - b0];
            place_loc(L, es[i], w, ref0, r.s0);
            if (!r.sorted) { L.pre = 2; continue; }                // (the stable order by clipped start needs sorted records)
            auto lower = std::lower_bound(r.recs.begin(), r.recs.end(), (int64_t)L.s0 - r.max_nref,
                                          [](const pg::Rec& m, int64_t v) { return (int64_t)m.pos < v; });
            auto upper = std::lower_bound(r.recs.begin(), r.recs.end(), (int64_t)L.stop, [](const pg::Rec& m, int64_t v) { return (int64_t)m.pos < v; });
            L.first = rec0 + (int32_t)(lower - r.recs.begin());
            L.last = rec0 + (int32_t)(upper - r.recs.begin());
        }
        at += r.bytes.size();
        res += r.nres;
        h->sst.records_seen += r.seen;
        std::vector<uint8_t>().swap(r.bytes);
    }
    h->st.host_frame_ms += ms_since(t_host);
    h->st.host_records += (int64_t)recs.size();
    h->st.records += (int64_t)recs.size();
    h->sst.records_kept += (int64_t)recs.size();
    // device
    hipStream_t s = h->stream;
    if (h->d_buf.ensure(bytes + 4) || h->d_recs.ensure(recs.size() + 1) || h->d_locs.ensure(locs.size() + 1) || h->d_ref.ensure(ref.size() + 1) ||
        h->d_qpos.ensure((size_t)res + 1) || h->d_indel.ensure((size_t)res + 1) || h->d_isdel.ensure((size_t)res + 1) ||
        h->d_small.ensure(SmallLayout(nb, W).bytes + 16))
        return fail(h, -2, "hipMalloc failed (batch of %lld locations, %zu records)", (long long)nb, recs.size());
    hipError_t rc = hipSuccess;
    auto ok = [&](hipError_t r) { if (rc == hipSuccess) rc = r; };
    ok(hipEventRecord(h->ev[0], s));
    if (bytes) ok(hipMemcpyAsync(h->d_buf.p, h->h_buf.p, bytes, hipMemcpyHostToDevice, s));
    if (!recs.empty()) ok(hipMemcpyAsync(h->d_recs.p, recs.data(), recs.size() * sizeof(pg::Rec), hipMemcpyHostToDevice, s));
    ok(hipMemcpyAsync(h->d_locs.p, locs.data(), locs.size() * sizeof(pg::Loc), hipMemcpyHostToDevice, s));
    if (!ref.empty()) ok(hipMemcpyAsync(h->d_ref.p, ref.data(), ref.size(), hipMemcpyHostToDevice, s));
    ok(hipEventRecord(h->ev[1], s));
    ok(pg::launch_resolve(h->d_buf.p, h->d_recs.p, (int32_t)recs.size(), h->d_qpos.p, h->d_indel.p, h->d_isdel.p, s));
    ok(run_locations(h, h->d_buf.p, h->d_recs.p, nb, batch_planes(h, out), h->ev[1], h->ev[2]));
    float ms = 0.f;
    if (rc == hipSuccess && hipEventElapsedTime(&ms, h->ev[0], h->ev[1]) == hipSuccess) h->st.upload_ms += ms;
    if (rc != hipSuccess) return fail(h, -2, "device: %s", hipGetErrorString(rc));
    return 0;
}

// Copies ref / num / status (and, unless the planes are the caller's device arrays, the planes) of the piece [i0, i1) of the
// sorted entries, which the encode kernel left at the piece's slots, to the caller's arrays.
int copy_back(pg_encoder* h, const std::vector<Entry>& es, int64_t i0, int64_t i1, const Outs& out, std::vector<uint8_t>& small) {
    const int W = 2 * h->opt.window_size + 1;
    const size_t plane = (size_t)h->opt.max_reads * W;
    const int64_t nb = i1 - i0;
    const SmallLayout sl(nb, W);
    small.resize(sl.bytes);
    // (census_locations wrote the statuses alone)
    const size_t from = h->census ? sl.status : 0;
    if (sl.bytes > from && hipMemcpy(small.data() + from, h->d_small.p + from, sl.bytes - from, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, -2, "hipMemcpy failed");
    const int32_t* num = (const int32_t*)(small.data() + sl.num);
    const int8_t* st = (const int8_t*)(small.data() + sl.status);
    if (h->census) {
        for (int64_t i = 0; i < nb; ++i) out.status[es[i0 + i].idx] = st[i];
        return 0;
    }
    if (!out.device_planes) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int c = 0; c < 3; ++c)
            if (hipMemcpy(h->h_planes.p + c * plane * BATCH_LOCS, h->d_planes.p + c * plane * BATCH_LOCS, plane * nb, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(h, -2, "hipMemcpy failed");
        h->st.copy_back_ms += ms_since(t0);
    }
    for (int64_t i = 0; i < nb; ++i) {
        const int64_t j = es[i0 + i].idx;
        out.status[j] = st[i];
        out.num[j] = num[i];
        memcpy(out.ref + (size_t)j * W, small.data() + (size_t)i * W, W);
        if (!out.device_planes)
            for (int c = 0; c < 3; ++c) {
                uint8_t* dst = c == 0 ? out.reads : c == 1 ? out.qual : out.strand;
                memcpy(dst + (size_t)j * plane, h->h_planes.p + c * plane * BATCH_LOCS + (size_t)i * plane, plane);
            }
    }
    return 0;
}

// ---- the device inflate path (pg_set_inflate_device) ------------------------------------------------------------------------
#define PG_TRY(x) DEV_TRY(h->err, "device inflate: ", x)

// Encodes the piece [i0, i1) of the sorted entries (at most BATCH_LOCS) from the group's records on the device; runs
// [ra, rb) are the group's runs that lie in the piece (g0: the group's first run).
int encode_piece(pg_encoder* h, const std::vector<Entry>& es, int64_t i0, int64_t i1, const std::vector<Run>& runs, size_t ra, size_t rb,
                 size_t g0, size_t g1, const pg::Rec* d_grecs, const pg::RunOut* d_run_out, const Outs& out) {
    const int w = h->opt.window_size, W = 2 * w + 1;
    const int64_t nb = i1 - i0;
    std::vector<pg::Loc> locs = loc_table(es, i0, nb, out.device_planes);
    std::vector<int32_t> loc_run((size_t)nb, -1);
    std::vector<uint8_t> ref;
    for (size_t r = ra; r < rb; ++r) {
        const Run& run = runs[r];
        const int64_t ref0 = (int64_t)ref.size();
        ref.insert(ref.end(), run.ref.begin(), run.ref.end());
        for (int64_t i = run.e0; i < run.e1; ++i) {
            place_loc(locs[i - i0], es[i], w, ref0, run.s0);
            loc_run[i - i0] = (int32_t)(r - g0);
        }
    }
    hipStream_t s = h->stream;
    if (h->d_locs.ensure(locs.size() + 1) || h->d_ref.ensure(ref.size() + 1) || h->d_small.ensure(SmallLayout(nb, W).bytes + 16))
        return fail(h, -2, "hipMalloc failed (piece of %lld locations)", (long long)nb);
    // device events between the stages, as on the host path: upload | location search | encode
    PG_TRY(hipEventRecord(h->ev[0], s));
    PG_TRY(hipMemcpyAsync(h->d_locs.p, locs.data(), locs.size() * sizeof(pg::Loc), hipMemcpyHostToDevice, s));
    if (!ref.empty()) PG_TRY(hipMemcpyAsync(h->d_ref.p, ref.data(), ref.size(), hipMemcpyHostToDevice, s));
    const char* msg = nullptr;
    if (g1 > g0 && pg::locate(h->framing.get(), d_grecs, d_run_out, (int32_t)(g1 - g0), loc_run.data(), h->d_locs.p, (int32_t)nb, s, &msg, h->ev[1]))
        return fail(h, -2, "device framing: %s", msg);
    if (g1 == g0) PG_TRY(hipEventRecord(h->ev[1], s));
    PG_TRY(hipEventRecord(h->ev[2], s));
    PG_TRY(run_locations(h, h->inflate.d_infl.p, d_grecs, nb, batch_planes(h, out), h->ev[2], h->ev[3]));
    float ms = 0.f;
    PG_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->st.upload_ms += ms;
    PG_TRY(hipEventElapsedTime(&ms, h->ev[1], h->ev[2]));
    h->st.frame_ms += ms;
    return 0;
}

// the pieces of [e0, e1): cut where the BATCH_LOCS batches of the sorted list are cut
int encode_pieces(pg_encoder* h, const std::vector<Entry>& es, int64_t e0, int64_t e1, const std::vector<Run>& runs, size_t g0, size_t g1,
                  const pg::Rec* d_grecs, const pg::RunOut* d_run_out, const Outs& out, std::vector<uint8_t>& small) {
    size_t r = g0;
    for (int64_t i0 = e0; i0 < e1;) {
        const int64_t i1 = std::min<int64_t>(e1, (i0 / BATCH_LOCS + 1) * BATCH_LOCS);
        const size_t ra = r;
        while (r < g1 && runs[r].e1 <= i1) ++r;
        int rc = encode_piece(h, es, i0, i1, runs, ra, r, g0, g1, d_grecs, d_run_out, out);
        if (rc) return rc;
        rc = copy_back(h, es, i0, i1, out, small);
        if (rc) return rc;
        i0 = i1;
    }
    return 0;
}

// The whole call with the BGZF blocks inflated and the records framed on the device: the runs of encode_batch over every
// batch, their byte ranges from the BAI bins, the touched blocks read as they are; then, group of runs by group of runs,
// inflate, walk, frame, resolve and encode.  The host does no per-record work.
int encode_all_device(pg_encoder* h, const char* const* contigs, std::vector<Entry>& es, const Outs& out) {
    const int64_t n = (int64_t)es.size();
    const pe_options& o = h->opt;
    std::vector<uint8_t> small;
    std::vector<Run> runs;
    for (int64_t b0 = 0; b0 < n; b0 += BATCH_LOCS) build_runs(o, contigs, es, b0, std::min<int64_t>(n, b0 + BATCH_LOCS), runs);
    if (runs.empty()) return encode_pieces(h, es, 0, n, runs, 0, 0, nullptr, nullptr, out, small);
    if (runs.size() > (size_t)INT32_MAX) return fail(h, -1, "too many runs of locations in one call");
    hipStream_t s = h->stream;
    bz::InflateStage& inf = h->inflate;
    // read: the byte ranges of every run, and the blocks they touch into pinned memory
    const auto t_read = std::chrono::steady_clock::now();
    std::vector<pgh::Region> regs(runs.size());
    for (size_t r = 0; r < runs.size(); ++r) regs[r] = pgh::Region{runs[r].tid, runs[r].s0, runs[r].stop};
    bz::BlockPlan all;
    std::string perr;
    all.plan(h->bai, regs.data(), (int64_t)regs.size());
    if (const int rc = inf.read(all, h->bam_path, h->err)) return rc;
    // every run's inflated size, from the trailers of the blocks its own ranges touch
    std::vector<uint64_t> run_bytes(runs.size());
    for (size_t r = 0; r < runs.size(); ++r) {
        bz::BlockPlan one;
        one.plan(h->bai, &regs[r], 1);
        if (!one.adopt(all, perr)) return fail(h, -3, "%s", perr.c_str());
        run_bytes[r] = one.infl_bytes;
    }
    h->st.read_ms += ms_since(t_read);
    if (const int rc = inf.upload(all, s, h->err, h->ev[0])) return rc;
    PG_TRY(hipEventRecord(h->ev[1], s));
    PG_TRY(hipStreamSynchronize(s));
    float ms = 0.f;
    PG_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->st.upload_ms += ms;
    h->st.compressed_bytes += (int64_t)all.comp_bytes;
    if (!h->walker) h->walker.reset(bz::framer_create());
    if (!h->framing) h->framing.reset(pg::framing_create());
    const int nt = thread_count(runs.size());
    if (const int rc = ensure_workers(h, nt)) return rc;
    for (size_t g0 = 0; g0 < runs.size();) {
        // the longest prefix of the remaining runs within the budget (one run over it is a group of its own)
        size_t g1 = g0 + 1;
        uint64_t sum = run_bytes[g0];
        while (g1 < runs.size() && sum + run_bytes[g1] <= h->max_inflated) sum += run_bytes[g1++];
        const auto t_plan = std::chrono::steady_clock::now();
        bz::BlockPlan pl;
        pl.plan(h->bai, regs.data() + g0, (int64_t)(g1 - g0));
        if (!pl.adopt(all, perr) || !pl.segments(perr)) return fail(h, -3, "%s", perr.c_str());
        h->st.read_ms += ms_since(t_plan);
        ++h->st.groups;
        h->st.blocks += (int64_t)pl.tab.size();
        h->st.inflated_bytes += (int64_t)pl.infl_bytes;
        if (const int rc = inf.enqueue(pl, s, h->err)) return rc;
        // the reference tokens of the group's runs, on the worker threads while the device inflates
        const std::string werr = on_workers(h, nt, g0, g1, [&](Worker* wk, size_t r) { fetch_ref(wk->fasta, runs[r]); });
        const int inflated = inf.finish(pl, s, &h->st.inflate_ms, h->err);
        if (!werr.empty()) return fail(h, -3, "%s", werr.c_str());
        if (inflated) return inflated;
        // walk, frame, list per run (both calls wait for their kernels: the events bracket them)
        PG_TRY(hipEventRecord(h->ev[2], s));
        const uint64_t* d_rec_off = nullptr;
        uint64_t n_walked = 0, err = bz::NO_ERROR;
        const char* msg = nullptr;
        if (bz::walk_records(h->walker.get(), inf.d_infl.p, pl.infl_bytes, pl.segs.data(), pl.segs.size(), pl.n_slots, s, &d_rec_off, &n_walked, &err, &msg))
            return fail(h, -2, "device framing: %s", msg);
        if (err != bz::NO_ERROR)
            return fail(h, -3, "%s (record at virtual offset %lld)", pg::frame::why_text((uint32_t)(err & 0xff)), (long long)pl.voff_of(err >> 8));
        std::vector<pg::RunDesc> rd(g1 - g0);
        for (size_t r = g0; r < g1; ++r) rd[r - g0] = pg::RunDesc{runs[r].tid, 0, runs[r].s0, runs[r].stop};
        pg::Rec* d_grecs = nullptr;
        const pg::RunOut* d_run_out = nullptr;
        int64_t n_recs = 0, n_res = 0, n_seen = 0;
        if (pg::frame_runs(h->framing.get(), inf.d_infl.p, d_rec_off, d_rec_off ? pl.n_slots : 0, rd.data(), (int32_t)rd.size(), s, &d_grecs, &n_recs,
                           &n_res, &d_run_out, &err, &msg, h->sample, &n_seen, h->filter, h->collects() ? &h->read_census : nullptr))
            return fail(h, -2, "device framing: %s", msg);
        if (err != pg::FRAME_NO_ERROR)
            return fail(h, -3, "%s (record at virtual offset %lld)", pg::frame::why_text((uint32_t)(err & 0xff)), (long long)pl.voff_of(err >> 8));
        PG_TRY(hipEventRecord(h->ev[3], s));
        PG_TRY(hipEventSynchronize(h->ev[3]));
        PG_TRY(hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
        h->st.frame_ms += ms;
        h->st.records += n_recs;
        h->sst.records_seen += n_seen;
        h->sst.records_kept += n_recs;
        if (n_res > INT32_MAX || n_recs > INT32_MAX) return fail(h, -1, "batch too large (%lld reference positions of records)", (long long)n_res);
        if (h->d_qpos.ensure((size_t)n_res + 1) || h->d_indel.ensure((size_t)n_res + 1) || h->d_isdel.ensure((size_t)n_res + 1))
            return fail(h, -2, "hipMalloc failed (group of %lld records)", (long long)n_recs);
        PG_TRY(hipEventRecord(h->ev[0], s));
        PG_TRY(pg::launch_resolve(inf.d_infl.p, d_grecs, (int32_t)n_recs, h->d_qpos.p, h->d_indel.p, h->d_isdel.p, s));
        PG_TRY(hipEventRecord(h->ev[1], s));
        PG_TRY(hipStreamSynchronize(s));
        PG_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        (h->census ? h->st.census_ms : h->st.encode_ms) += ms;
        // the group's entries; the last group takes the entries decided on the host as well
        const int64_t e0 = g0 == 0 ? 0 : runs[g0].e0, e1 = g1 == runs.size() ? n : runs[g1].e0;
        if (const int rc = encode_pieces(h, es, e0, e1, runs, g0, g1, d_grecs, d_run_out, out, small)) return rc;
        for (size_t r = g0; r < g1; ++r) std::vector<uint8_t>().swap(runs[r].ref);
        g0 = g1;
    }
    return 0;
}
#undef PG_TRY

int encode_all(pg_encoder* h, const char* const* contigs, const int32_t* positions, int64_t n, const Outs& out, void* stream,
               bool census = false) {
    // (pg_census: device_planes with no plane -- nothing but status_out is written, on the device or here)
    if (n < 0 || (n > 0 && (!contigs || !positions || !out.status)) ||
        (n > 0 && !census && (!out.reads || !out.qual || !out.strand || !out.ref || !out.num)))
        return fail(h, -1, "null argument");
    h->census = census;
    const pe_options& o = h->opt;
    const int W = 2 * o.window_size + 1, MR = o.max_reads;
    const size_t plane = (size_t)MR * W;
    // (a BAM without a BAI is indexed by one scan here, before the device is touched: a corrupt record needs no GPU)
    if (!h->have_bai && !h->scanned) {
        h->scanned = true;
        const int rc = build_linear_index(h);
        if (rc) { h->scanned = false; return rc; }
    }
    dev::DeviceGuard guard;                               // the caller's current device is restored on every return
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, -2, "hipSetDevice(%d) failed", h->device);
    if (h->stream.ensure() != hipSuccess) return fail(h, -2, "hipStreamCreate failed");
    for (dev::Event& e : h->ev)
        if (e.ensure() != hipSuccess) return fail(h, -2, "hipEventCreate failed");
    h->st = pg_stats{};
    h->sst = pg_subsample_stats{};
    h->read_census = pg::frame::Census{};
    // the caller's stream must not run ahead of (or behind) our work on its planes
    hipStream_t cs = (hipStream_t)stream;
    if (out.device_planes) {
        dev::Event ev;
        if (ev.ensure(hipEventDisableTiming) != hipSuccess) return fail(h, -2, "hipEventCreate failed");
        if (hipEventRecord(ev, cs) != hipSuccess || hipStreamWaitEvent(h->stream, ev, 0) != hipSuccess)
            return fail(h, -2, "cannot order the encoder after the caller's stream");
    }
    std::vector<Entry> es((size_t)n);
    const bool plan = o.window_size <= pg::MAX_WINDOW && o.min_base_quality <= 0;
    std::string last_name;
    int last_tid = -1;
    bool last_fa = false;
    for (int64_t i = 0; i < n; ++i) {
        if (!contigs[i]) return fail(h, -1, "contig %lld is NULL", (long long)i);
        if (i == 0 || last_name != contigs[i]) {
            last_name = contigs[i];
            last_tid = get_tid(h->header, last_name);
            last_fa = h->fasta.entry(last_name) != nullptr;
        }
        Entry& e = es[i];
        e.tid = last_tid; e.pos1 = positions[i]; e.idx = i;
        e.pre = last_tid < 0 ? 0 : (!last_fa || !plan) ? 2 : -1;   // (encode_one's order: no tid, no FASTA sequence, options)
        if (e.pre < 0 && (positions[i] < 1 || (int64_t)positions[i] + o.window_size + 3 > INT32_MAX)) e.pre = 2;
    }
    std::stable_sort(es.begin(), es.end(), [](const Entry& a, const Entry& b) {
        const int ka = a.pre < 0 ? 0 : 1, kb = b.pre < 0 ? 0 : 1;
        if (ka != kb) return ka < kb;
        return a.tid != b.tid ? a.tid < b.tid : a.pos1 < b.pos1;
    });
    if (!out.device_planes && h->d_planes.ensure(3 * plane * BATCH_LOCS)) return fail(h, -2, "hipMalloc of the plane buffer failed");
    if (!out.device_planes && h->h_planes.ensure(3 * plane * BATCH_LOCS)) return fail(h, -2, "hipHostMalloc of the plane buffer failed");
    if (h->inflate_device) return encode_all_device(h, contigs, es, out);
    std::vector<uint8_t> small;
    for (int64_t b0 = 0; b0 < n; b0 += BATCH_LOCS) {
        const int64_t b1 = std::min<int64_t>(n, b0 + BATCH_LOCS);
        int rc = encode_batch(h, contigs, es, b0, b1, out);
        if (rc) return rc;
        rc = copy_back(h, es, b0, b1, out, small);
        if (rc) return rc;
    }
    return 0;
}

constexpr int64_t Z_CHUNKS = 512;           // chunks per pass of pg_compress_records_device (4 096 records at 8 per chunk)

int compress_records(pg_encoder* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, const int32_t* slots,
                     const uint8_t* blob, int64_t n, int32_t rpc, const uint8_t** out, uint64_t* offsets, uint64_t* sizes, uint32_t* adlers,
                     uint8_t* store, void* stream) {
    if (!out || n < 0 || n_slots < 0) return fail(h, -1, "pg_compress_records_device: null argument or negative count");
    *out = nullptr;
    if (rpc < 1 || rpc > 64) return fail(h, -1, "pg_compress_records_device: 1..64 records per chunk");
    const pe_options& o = h->opt;
    const uint32_t W = 2 * (uint32_t)o.window_size + 1;
    if ((uint64_t)o.max_reads * W > (1u << 24)) return fail(h, -1, "pg_compress_records_device: record planes too large");
    const uint32_t plane = (uint32_t)o.max_reads * W, head = 16 + 15 * W, mid = W + 4 + 1 + 128, blob_bytes = head + mid;
    const uint64_t itemsize = (uint64_t)blob_bytes + 3ull * plane, chunk_bytes = itemsize * (uint64_t)rpc;
    if (chunk_bytes > zd::MAX_STREAM) return fail(h, -1, "pg_compress_records_device: a chunk of %llu bytes is too large", (unsigned long long)chunk_bytes);
    h->st.pack_ms = h->st.deflate_ms = h->st.gather_ms = h->st.compress_copy_back_ms = 0;
    h->st.chunks = h->st.raw_bytes = h->st.chunk_bytes_out = h->st.stored_chunks = 0;
    h->st.fixed_segments = h->st.dynamic_segments = h->st.stored_segments = 0;
    if (n == 0) return 0;
    if (!reads || !qual || !strand || !slots || !blob || !offsets || !sizes || !adlers || !store)
        return fail(h, -1, "pg_compress_records_device: null argument");
    // every index the pack kernel follows is checked here
    for (int64_t i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= n_slots)
            return fail(h, -1, "pg_compress_records_device: record %lld names slot %d of %lld", (long long)i, slots[i], (long long)n_slots);
    dev::DeviceGuard guard;
    if (hipSetDevice(h->device) != hipSuccess) return fail(h, -2, "hipSetDevice(%d) failed", h->device);
    for (dev::Event& e : h->zev)
        if (e.ensure() != hipSuccess) return fail(h, -2, "hipEventCreate failed");
    if (!h->zctx) h->zctx.reset(zd::ctx_create());
    const int64_t n_chunks = (n + rpc - 1) / rpc;
    const int64_t pass_chunks = std::min<int64_t>(n_chunks, Z_CHUNKS), pass_records = pass_chunks * rpc;
    const uint64_t cbound = zd::bound(chunk_bytes, zd::DEFAULT_SEG);
    const size_t stage = (size_t)pass_records * (blob_bytes + 4);            // blob | slots of one pass
    if (h->d_image.ensure((size_t)pass_chunks * chunk_bytes + 8) || h->d_zout.ensure((size_t)pass_chunks * cbound) || h->d_blob.ensure(stage))
        return fail(h, -2, "hipMalloc failed (%lld chunks of %llu bytes)", (long long)pass_chunks, (unsigned long long)chunk_bytes);
    if (h->h_blob.ensure(stage)) return fail(h, -2, "hipHostMalloc of the blob staging failed");
    hipStream_t s = (hipStream_t)stream;
#define PZ_TRY(x) DEV_TRY(h->err, "pg_compress_records_device: ", x)
    uint64_t total = 0;
    for (int64_t c0 = 0; c0 < n_chunks; c0 += pass_chunks) {
        const int64_t nc = std::min<int64_t>(pass_chunks, n_chunks - c0);
        const int64_t r0 = c0 * rpc, nr = std::min<int64_t>(n - r0, nc * rpc);
        const size_t b_blob = (size_t)nr * blob_bytes;
        memcpy(h->h_blob.p, blob + (size_t)r0 * blob_bytes, b_blob);
        memcpy(h->h_blob.p + (size_t)pass_records * blob_bytes, slots + r0, (size_t)nr * 4);
        PZ_TRY(hipEventRecord(h->zev[0], s));
        PZ_TRY(hipMemcpyAsync(h->d_blob.p, h->h_blob.p, b_blob, hipMemcpyHostToDevice, s));
        PZ_TRY(hipMemcpyAsync(h->d_blob.p + (size_t)pass_records * blob_bytes, h->h_blob.p + (size_t)pass_records * blob_bytes, (size_t)nr * 4,
                              hipMemcpyHostToDevice, s));
        zd::PackArgs a{};
        a.planes[0] = reads; a.planes[1] = qual; a.planes[2] = strand;
        a.blob = h->d_blob.p;
        a.slots = (const int32_t*)(h->d_blob.p + (size_t)pass_records * blob_bytes);
        a.n_records = nr; a.plane = plane; a.head = head; a.mid = mid;
        const uint64_t image_bytes = ((uint64_t)nc * chunk_bytes + 7) & ~7ull;       // (chunk_bytes * rpc-of-8 is a multiple of 8; any rpc: + 8 above)
        PZ_TRY(zd::launch_pack(a, image_bytes, h->d_image.p, s));
        PZ_TRY(hipEventRecord(h->zev[1], s));
        zd::Streams r{};
        const char* msg = nullptr;
        if (zd::run(h->zctx.get(), h->d_image.p, chunk_bytes, nc, zd::DEFAULT_SEG, false, true, h->compress_dynamic, h->d_zout.p, s, h->zev[2], &r, &msg))
            return fail(h, -2, "pg_compress_records_device: %s", msg);
        PZ_TRY(hipEventRecord(h->zev[3], s));
        PZ_TRY(hipMemcpyAsync(offsets + c0, r.offs, (size_t)nc * 8, hipMemcpyDeviceToHost, s));
        PZ_TRY(hipMemcpyAsync(sizes + c0, r.sizes, (size_t)nc * 8, hipMemcpyDeviceToHost, s));
        PZ_TRY(hipMemcpyAsync(adlers + c0, r.adlers, (size_t)nc * 4, hipMemcpyDeviceToHost, s));
        PZ_TRY(hipMemcpyAsync(store + c0, r.store, (size_t)nc, hipMemcpyDeviceToHost, s));
        if (r.seg_kind) {
            h->seg_kind.resize((size_t)r.n_segs);
            PZ_TRY(hipMemcpyAsync(h->seg_kind.data(), r.seg_kind, (size_t)r.n_segs, hipMemcpyDeviceToHost, s));
        }
        PZ_TRY(hipStreamSynchronize(s));
        if (r.seg_kind)
            for (const uint8_t kind : h->seg_kind)
                ++*(kind == zd::KIND_DYNAMIC ? &h->st.dynamic_segments : kind == zd::KIND_STORED ? &h->st.stored_segments : &h->st.fixed_segments);
        const uint64_t bytes = offsets[c0 + nc - 1] + sizes[c0 + nc - 1];
        if (bytes > (uint64_t)nc * cbound) return fail(h, -2, "pg_compress_records_device: the streams exceed their bound");
        if (h->h_zout.ensure_keep((size_t)(total + bytes), (size_t)total))   // (a later pass may outgrow it: the earlier passes' bytes stay)
            return fail(h, -2, "pinned allocation of %llu bytes failed", (unsigned long long)(total + bytes));
        PZ_TRY(hipMemcpyAsync(h->h_zout.p + total, h->d_zout.p, bytes, hipMemcpyDeviceToHost, s));
        PZ_TRY(hipEventRecord(h->zev[4], s));
        PZ_TRY(hipStreamSynchronize(s));
        for (int64_t c = c0; c < c0 + nc; ++c) {
            offsets[c] += total;
            h->st.stored_chunks += store[c] != 0;
        }
        total += bytes;
        float ms = 0.f;
        PZ_TRY(hipEventElapsedTime(&ms, h->zev[0], h->zev[1])); h->st.pack_ms += ms;
        PZ_TRY(hipEventElapsedTime(&ms, h->zev[1], h->zev[2])); h->st.deflate_ms += ms;
        PZ_TRY(hipEventElapsedTime(&ms, h->zev[2], h->zev[3])); h->st.gather_ms += ms;
        PZ_TRY(hipEventElapsedTime(&ms, h->zev[3], h->zev[4])); h->st.compress_copy_back_ms += ms;
    }
#undef PZ_TRY
    h->st.chunks = n_chunks;
    h->st.raw_bytes = (int64_t)((uint64_t)n_chunks * chunk_bytes);
    h->st.chunk_bytes_out = (int64_t)total;
    *out = h->h_zout.p;
    return 0;
}

}  // namespace

extern "C" {

const char* pg_last_error(const pg_encoder_t* h) { return h ? h->err.c_str() : pgh::g_err.c_str(); }

int pg_open(const char* bam_path, const char* bai_path, const char* fasta_path, const pe_options* opt, int32_t device, pg_encoder_t** out) {
    return capi::guarded(pgh::g_err, "pg_open", [&] {
        if (!bam_path || !fasta_path || !opt || !out) return fail(nullptr, -1, "pg_open: null argument");
        *out = nullptr;
        if (opt->window_size < 1 || opt->max_reads < 1) return fail(nullptr, -1, "pg_open: window_size and max_reads must be positive");
        std::unique_ptr<pg_encoder> h(new pg_encoder());
        h->bam_path = bam_path; h->fasta_path = fasta_path; h->opt = *opt; h->device = device;
        if (!h->header.open(bam_path)) return fail(nullptr, -3, "%s", h->header.err.c_str());
        std::string err;
        if (!h->fasta.open(fasta_path, err)) return fail(nullptr, -3, "%s", err.c_str());
        std::vector<std::string> cands;
        if (bai_path && *bai_path) cands.push_back(bai_path);
        else {
            cands.push_back(std::string(bam_path) + ".bai");
            const std::string p(bam_path);
            const size_t dot = p.find_last_of('.'), slash = p.find_last_of('/');
            if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) cands.push_back(p.substr(0, dot) + ".bai");
        }
        for (auto& c : cands) if (h->bai.load(c)) { h->have_bai = true; break; }
        *out = h.release();
        return 0;
    });
}

int pg_encode(pg_encoder_t* h, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_out, uint8_t* qual_out,
              uint8_t* strand_out, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out) {
    if (!h) return fail(nullptr, -1, "pg_encode: null handle");
    return capi::guarded(h->err, "pg_encode", [&] {
        return encode_all(h, contigs, positions, n, Outs{reads_out, qual_out, strand_out, ref_out, num_reads_out, status_out, false}, nullptr);
    });
}

int pg_encode_device(pg_encoder_t* h, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_dev,
                     uint8_t* qual_dev, uint8_t* strand_dev, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out,
                     void* stream) {
    if (!h) return fail(nullptr, -1, "pg_encode_device: null handle");
    return capi::guarded(h->err, "pg_encode_device", [&] {
        return encode_all(h, contigs, positions, n, Outs{reads_dev, qual_dev, strand_dev, ref_out, num_reads_out, status_out, true}, stream);
    });
}

int pg_census(pg_encoder_t* h, const char* const* contigs, const int32_t* positions, int64_t n, int8_t* status_out, void* stream) {
    if (!h) return fail(nullptr, -1, "pg_census: null handle");
    return capi::guarded(h->err, "pg_census", [&] {
        return encode_all(h, contigs, positions, n, Outs{nullptr, nullptr, nullptr, nullptr, nullptr, status_out, true}, stream, true);
    });
}

int pg_assemble_device(pg_encoder_t* h, const uint8_t* reads_src, const uint8_t* qual_src, const uint8_t* strand_src, int64_t n_slots,
                       int32_t stored_rows, int32_t window, const int32_t* slots, const int16_t* rows, const uint8_t* first_rows,
                       int64_t m, int32_t reads, const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask,
                       int32_t use_q, int32_t use_strand, uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out,
                       uint8_t* ref_out, uint8_t* ref_mask_out, uint8_t* var_mask_out, void* stream) {
    if (!h) return fail(nullptr, -1, "pg_assemble_device: null handle");
    return capi::guarded(h->err, "pg_assemble_device", [&] {
        const uint8_t* src[3] = {reads_src, qual_src, strand_src};    // [n_slots][stored_rows][window]: a slot is one plane of a site
        return pgh::assemble(h, "pg_assemble_device", src, (int64_t)stored_rows * window, n_slots, stored_rows, window, slots, rows,
                             first_rows, m, reads, ref, ref_mask, var_mask, use_q, use_strand, reads_out, qual_out, strand_out, ref_out,
                             ref_mask_out, var_mask_out, stream);
    });
}

int pg_compress_records_device(pg_encoder_t* h, const uint8_t* reads_dev, const uint8_t* qual_dev, const uint8_t* strand_dev,
                               int64_t n_slots, const int32_t* slots, const uint8_t* blob, int64_t n_records,
                               int32_t records_per_chunk, const uint8_t** out, uint64_t* offsets, uint64_t* sizes, uint32_t* adlers,
                               uint8_t* store, void* stream) {
    if (!h) return fail(nullptr, -1, "pg_compress_records_device: null handle");
    return capi::guarded(h->err, "pg_compress_records_device", [&] {
        return compress_records(h, reads_dev, qual_dev, strand_dev, n_slots, slots, blob, n_records, records_per_chunk, out, offsets, sizes,
                                adlers, store, stream);
    });
}

int pg_set_inflate_device(pg_encoder_t* h, int on, uint64_t max_inflated_bytes) {
    if (!h) return fail(nullptr, -1, "pg_set_inflate_device: null handle");
    return capi::guarded(h->err, "pg_set_inflate_device", [&] {
        if (on && (!h->have_bai || h->bai.bins.empty()))
            return fail(h, -1, "inflate on the device needs the BAI index of %s: its bins give the byte ranges to read", h->bam_path.c_str());
        if (on && !h->inflate.open(h->bam_path)) return fail(h, -3, "cannot open %s", h->bam_path.c_str());
        h->inflate_device = on != 0;
        h->max_inflated = max_inflated_bytes ? max_inflated_bytes : DEFAULT_INFLATED;
        return 0;
    });
}

int pg_set_subsample(pg_encoder_t* h, double fraction, uint32_t seed) {
    if (!h) return fail(nullptr, -1, "pg_set_subsample: null handle");
    return capi::guarded(h->err, "pg_set_subsample", [&] {
        if (const char* why = pg::frame::sample_rule(fraction, seed, h->sample)) return fail(h, -1, "pg_set_subsample: %s", why);
        return 0;
    });
}

int pg_get_subsample_stats(const pg_encoder_t* h, pg_subsample_stats* out) {
    if (!h || !out) return fail(nullptr, -1, "pg_get_subsample_stats: null argument");
    *out = h->sst;
    return 0;
}

int pg_set_read_filter(pg_encoder_t* h, int32_t exclude, int32_t require, int32_t min_mapq) {
    if (!h) return fail(nullptr, -1, "pg_set_read_filter: null handle");
    return capi::guarded(h->err, "pg_set_read_filter", [&] {
        if (const char* why = pg::frame::read_filter(exclude, require, min_mapq, h->filter)) return fail(h, -1, "pg_set_read_filter: %s", why);
        return 0;
    });
}

int pg_set_read_stats(pg_encoder_t* h, int on) {
    if (!h) return fail(nullptr, -1, "pg_set_read_stats: null handle");
    h->read_stats = on != 0;
    return 0;
}

int pg_get_read_stats(const pg_encoder_t* h, dl4vc_read_stats* out) {
    if (!h || !out) return fail(nullptr, -1, "pg_get_read_stats: null argument");
    static_assert(sizeof(dl4vc_read_stats) == sizeof(h->read_census.w), "dl4vc_read_stats is the census's words");
    memcpy(out, h->read_census.w, sizeof(*out));
    return 0;
}

int pg_set_compress_codes(pg_encoder_t* h, int mode) {
    if (!h) return fail(nullptr, -1, "pg_set_compress_codes: null handle");
    if (mode != 0 && mode != 1) return fail(h, -1, "pg_set_compress_codes: mode %d is neither 0 (fixed) nor 1 (dynamic)", mode);
    h->compress_dynamic = mode == 1;
    return 0;
}

int pg_get_stats(const pg_encoder_t* h, pg_stats* out) {
    if (!h || !out) return fail(nullptr, -1, "pg_get_stats: null argument");
    *out = h->st;
    return 0;
}

void pg_close(pg_encoder_t* h) {
    try {
        delete h;
    } catch (...) {
    }
}

}  // extern "C"
