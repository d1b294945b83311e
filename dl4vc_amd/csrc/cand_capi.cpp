// Host side of libdl4vc_cand.so (C ABI: include/dl4vc_candgen.h).  Worker threads, each with its own BAM handle, fetch the
// records of a batch of subregions (BAI linear index, htslib's overlap rule: pos < end and bam_endpos > start, no flag
// filter), frame and validate every record (the frame core of bam_frame.h) and gather them into one pinned buffer; the device
// does the rest (cand_kernels.hip).  A read overlapping two subregions is listed once for each, as the reference's per
// subregion fetch counts it.  Every extern "C" body catches what it throws: a corrupt file is an error code, never an abort.
//
// With cg_set_inflate_device() the host does none of that: run_batch_device() takes the batch's byte ranges from the BAI bins,
// reads their BGZF blocks as they are into pinned memory, and the device inflates them, walks the record chain, frames the
// records and lists them per subregion (bgzf_kernels.hip); the same count / emit / filter kernels follow.
#include "../../include/dl4vc_candgen.h"
#include "bam_frame.h"
#include "bam_native.h"
#include "bgzf_device.h"
#include "cand_device.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const char BASES[] = "=ACMGRSVTWYHKDBN";
constexpr int64_t BATCH_BASES = 4000000;     // subregion length gathered per device batch
constexpr uint32_t MAX_BATCH_SUBS = 1u << 20;

struct Gathered {
    std::vector<uint8_t> bytes;
    std::vector<cand::ReadMeta> meta;   // off relative to bytes
    std::string err;
};

}  // namespace

struct cg_handle {
    std::string bam_path;
    bamn::BamFile header;
    bamn::Bai bai;
    bool have_bai = false;
    cg_options opt{};
    hipStream_t stream = nullptr;
    cand::Workspace* ws = nullptr;
    uint8_t* pinned = nullptr;
    size_t pinned_cap = 0;
    std::vector<cg_candidate> out;
    // the device inflate path (cg_set_inflate_device)
    bool inflate_device = false;
    int fd = -1;
    bz::Framer* framer = nullptr;
    void *d_comp = nullptr, *d_tab = nullptr, *d_infl = nullptr, *d_bstatus = nullptr;
    size_t d_comp_cap = 0, d_tab_cap = 0, d_infl_cap = 0, d_bstatus_cap = 0;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    cg_inflate_stats ist{};
    ~cg_handle() {
        if (fd >= 0) close(fd);
        bz::framer_destroy(framer);
        for (void* p : {d_comp, d_tab, d_infl, d_bstatus}) if (p) (void)hipFree(p);
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (pinned) (void)hipHostFree(pinned);
        cand::workspace_destroy(ws);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace {

// the records of subregion s (one BAM handle per worker)
bool fetch_sub(cg_handle* h, bamn::BamFile& bam, std::vector<uint8_t>& blk, const cg_region& rg, uint32_t s, Gathered& g) {
    namespace F = bamn::frame;
    int64_t at = bam.first_record;
    if (h->have_bai) {
        const uint64_t off = h->bai.linear_offset(rg.tid, rg.start);
        if (off == 0) return true;
        at = (int64_t)off;
    }
    if (!bam.r.seek(at)) { g.err = "BGZF: " + bam.r.err; return false; }
    for (;;) {
        const int64_t voff = bam.r.tell();
        const int got = bam.next_block(blk);
        if (got == 0) return true;
        if (got < 0) { g.err = bam.err + " (record at virtual offset " + std::to_string(voff) + ")"; return false; }
        F::Framed fr;
        if (const uint32_t why = F::frame_record(blk.data(), blk.size(), fr)) {
            g.err = std::string(F::why_text(why)) + " (record at virtual offset " + std::to_string(voff) + ")";
            return false;
        }
        if (fr.tid != rg.tid) {
            if (fr.tid < 0 || fr.tid > rg.tid) return true;
            continue;
        }
        if (fr.pos >= rg.end) return true;
        F::cigar_sums(blk.data(), fr);
        if (F::endpos(fr) <= rg.start) continue;
        cand::ReadMeta m;
        m.off = g.bytes.size();
        m.len = (uint32_t)blk.size();
        m.sub = s;
        m.md_off = fr.md_off;
        m.md_len = fr.md_len;
        g.bytes.insert(g.bytes.end(), blk.begin(), blk.end());
        g.bytes.resize((g.bytes.size() + 3) & ~(size_t)3);
        g.meta.push_back(m);
    }
}

void decode(const cand::DevCand& c, cg_candidate& o) {
    auto base = [&](int i) { return BASES[(c.w[i >> 4] >> (60 - 4 * (i & 15))) & 0xf]; };
    memset(o.ref, 0, sizeof o.ref);
    memset(o.alt, 0, sizeof o.alt);
    if (c.kind == 0) {
        o.ref[0] = BASES[(c.w[0] >> 60) & 0xf];
        o.alt[0] = BASES[(c.w[0] >> 56) & 0xf];
        return;
    }
    const int n = (int)std::min<uint32_t>(c.len, CG_MAX_ALLELE_LEN);
    char* seq = c.kind == cand::KIND_INS ? o.alt : o.ref;
    char* one = c.kind == cand::KIND_INS ? o.ref : o.alt;
    for (int i = 0; i < n; ++i) seq[i] = base(i);
    one[0] = seq[0];
}

// the counting kernels over what upload() / upload_device() left in the workspace, and the batch's results
int finish_batch(cg_handle* h, const cg_region* regions, int64_t b0, uint64_t n_reads, uint32_t n_subs, int64_t cov, cg_stats& st) {
    const char* msg = nullptr;
    const cand::DevCand* dc = nullptr;
    const uint8_t* status = nullptr;
    uint64_t n_out = 0, n_events = 0, n_unique = 0;
    cand::BatchTimes bt{};
    if (cand::run_batch(h->ws, n_reads, n_subs, cov, h->opt.max_len_indel_allele, h->opt.snp_min_freq, h->opt.indel_min_freq,
                        h->stream, &dc, &n_out, &status, &n_events, &n_unique, &bt, &msg))
        return fail(-2, "device: %s", msg);
    st.device_ms += bt.device_ms;
    st.reads += (int64_t)n_reads;
    for (uint64_t r = 0; r < n_reads; ++r) {
        const uint8_t v = status[r];
        switch (v & 0xf) {
            case cand::ST_NO_MD: ++st.reads_no_md; break;
            case cand::ST_NO_PAIRS: ++st.reads_no_pairs; break;
            case cand::ST_UNSUPPORTED: ++st.reads_unsupported; break;
            case cand::ST_MALFORMED: ++st.reads_malformed; break;
            default: break;
        }
        if (v & cand::ST_DEL_DROPPED) ++st.reads_deletions_dropped;
    }
    st.allele_events += (int64_t)n_events;
    st.alleles += (int64_t)n_unique;
    st.candidates += (int64_t)n_out;
    ++st.batches;
    const size_t o = h->out.size();
    h->out.resize(o + n_out);
    for (uint64_t i = 0; i < n_out; ++i) {
        cg_candidate& c = h->out[o + i];
        c.region = (int32_t)(b0 + dc[i].sub);
        c.tid = regions[c.region].tid;
        c.pos0 = dc[i].pos;
        c.depth = dc[i].depth;
        c.count = dc[i].count;
        decode(dc[i], c);
    }
    return 0;
}

int run_batch(cg_handle* h, const cg_region* regions, int64_t b0, int64_t b1, cg_stats& st) {
    const uint32_t n_subs = (uint32_t)(b1 - b0);
    const int nt = std::max(1, std::min<int>(h->opt.threads, (int)n_subs));
    std::vector<Gathered> per(n_subs);
    std::atomic<uint32_t> next{0};
    std::mutex open_mu;
    std::string open_err;
    const auto t0 = std::chrono::steady_clock::now();
    auto worker = [&]() {
        bamn::BamFile bam;
        std::vector<uint8_t> blk;
        if (!bam.open(h->bam_path)) {
            std::lock_guard<std::mutex> lk(open_mu);
            open_err = bam.err;
            return;
        }
        for (;;) {
            const uint32_t s = next.fetch_add(1);
            if (s >= n_subs) return;
            try {
                fetch_sub(h, bam, blk, regions[b0 + s], s, per[s]);
            } catch (const std::exception& e) {
                per[s].err = std::string("host framing: ") + e.what();
            }
        }
    };
    std::vector<std::thread> pool;
    for (int i = 1; i < nt; ++i) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    if (!open_err.empty()) return fail(-3, "%s", open_err.c_str());
    for (uint32_t s = 0; s < n_subs; ++s)
        if (!per[s].err.empty()) return fail(-3, "%s", per[s].err.c_str());
    // the device is set up only now, after the first batch framed cleanly (framing errors need no GPU)
    if (hipSetDevice(h->opt.device) != hipSuccess) return fail(-2, "hipSetDevice(%d) failed", h->opt.device);
    if (!h->stream && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(-2, "hipStreamCreate failed");
    if (!h->ws && !(h->ws = cand::workspace_create())) return fail(-2, "cannot create the device workspace");
    // gather into the pinned buffer, subregion by subregion
    uint64_t bytes = 0, n_reads = 0;
    for (auto& g : per) { bytes += g.bytes.size(); n_reads += g.meta.size(); }
    if (bytes + 1 > h->pinned_cap) {
        if (h->pinned) (void)hipHostFree(h->pinned);
        h->pinned = nullptr; h->pinned_cap = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        if (hipHostMalloc((void**)&h->pinned, want, hipHostMallocDefault) != hipSuccess) return fail(-2, "hipHostMalloc(%zu) failed", want);
        h->pinned_cap = want;
    }
    std::vector<cand::ReadMeta> meta;
    meta.reserve(n_reads);
    std::vector<cand::SubDesc> subs(n_subs);
    uint64_t at = 0;
    int64_t cov = 0;
    for (uint32_t s = 0; s < n_subs; ++s) {
        const cg_region& rg = regions[b0 + s];
        subs[s].start = rg.start;
        subs[s].end = rg.end;
        subs[s].cov_base = cov;
        cov += (int64_t)rg.end - rg.start + 2;
        Gathered& g = per[s];
        if (!g.bytes.empty()) memcpy(h->pinned + at, g.bytes.data(), g.bytes.size());
        for (auto m : g.meta) { m.off += at; meta.push_back(m); }
        at += g.bytes.size();
        std::vector<uint8_t>().swap(g.bytes);
    }
    const auto t1 = std::chrono::steady_clock::now();
    st.host_frame_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    const char* msg = nullptr;
    if (cand::upload(h->ws, h->pinned, bytes, meta.data(), n_reads, subs.data(), n_subs, cov, h->stream, &msg))
        return fail(-2, "device upload: %s", msg);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(-2, "device upload failed");
    const auto t2 = std::chrono::steady_clock::now();
    st.upload_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
    return finish_batch(h, regions, b0, n_reads, n_subs, cov, st);
}

// ---- the device inflate path ---------------------------------------------------------------------------------------------
bool dev_ensure(void*& p, size_t& cap, size_t bytes) {
    if (bytes <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipMalloc(&p, want) != hipSuccess) return false;
    cap = want;
    return true;
}

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

int run_batch_device(cg_handle* h, const cg_region* regions, int64_t b0, int64_t b1, cg_stats& st) {
    const uint32_t n_subs = (uint32_t)(b1 - b0);
    const auto t0 = std::chrono::steady_clock::now();
    bz::BlockPlan pl;
    std::string perr;
    pl.plan(h->bai, regions + b0, b1 - b0);
    struct stat sb;
    if (fstat(h->fd, &sb) != 0) return fail(-3, "BGZF: cannot stat %s", h->bam_path.c_str());
    if (!pl.spans((uint64_t)sb.st_size, perr)) return fail(-3, "%s", perr.c_str());
    const uint64_t comp_bytes = pl.comp_bytes;
    if (hipSetDevice(h->opt.device) != hipSuccess) return fail(-2, "hipSetDevice(%d) failed", h->opt.device);
    if (comp_bytes + 1 > h->pinned_cap) {
        if (h->pinned) (void)hipHostFree(h->pinned);
        h->pinned = nullptr; h->pinned_cap = 0;
        const size_t want = comp_bytes + comp_bytes / 4 + 4096;
        if (hipHostMalloc((void**)&h->pinned, want, hipHostMallocDefault) != hipSuccess) return fail(-2, "hipHostMalloc(%zu) failed", want);
        h->pinned_cap = want;
    }
    if (!pl.read(h->fd, h->bam_path, h->pinned, perr) || !pl.segments(perr)) return fail(-3, "%s", perr.c_str());
    const std::vector<bz::BlockDesc>& tab = pl.tab;
    const std::vector<bz::HostBlock>& blocks = pl.blocks;
    const std::vector<bz::Segment>& segs = pl.segs;
    const uint64_t infl_bytes = pl.infl_bytes, n_slots = pl.n_slots;
    const auto t1 = std::chrono::steady_clock::now();
    st.host_frame_ms += ms_between(t0, t1);
    h->ist.read_ms += ms_between(t0, t1);
    h->ist.blocks += (int64_t)blocks.size();
    h->ist.compressed_bytes += (int64_t)comp_bytes;
    h->ist.inflated_bytes += (int64_t)infl_bytes;
    // the device
    if (!h->stream && hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(-2, "hipStreamCreate failed");
    if (!h->ws && !(h->ws = cand::workspace_create())) return fail(-2, "cannot create the device workspace");
    if (!h->framer) h->framer = bz::framer_create();
    for (hipEvent_t& e : h->ev)
        if (!e && hipEventCreate(&e) != hipSuccess) return fail(-2, "hipEventCreate failed");
    if (!dev_ensure(h->d_comp, h->d_comp_cap, comp_bytes + 16) || !dev_ensure(h->d_tab, h->d_tab_cap, (tab.size() + 1) * sizeof(bz::BlockDesc)) ||
        !dev_ensure(h->d_infl, h->d_infl_cap, infl_bytes + 16) || !dev_ensure(h->d_bstatus, h->d_bstatus_cap, (tab.size() + 1) * sizeof(int32_t)))
        return fail(-2, "hipMalloc failed for a batch of %llu compressed and %llu inflated bytes", (unsigned long long)comp_bytes,
                    (unsigned long long)infl_bytes);
#define CG_TRY(x)                                                                                 \
    do {                                                                                          \
        const hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) return fail(-2, "device inflate: %s: %s", #x, hipGetErrorString(e_)); \
    } while (0)
    if (comp_bytes) CG_TRY(hipMemcpyAsync(h->d_comp, h->pinned, comp_bytes, hipMemcpyHostToDevice, h->stream));
    if (!tab.empty()) CG_TRY(hipMemcpyAsync(h->d_tab, tab.data(), tab.size() * sizeof(bz::BlockDesc), hipMemcpyHostToDevice, h->stream));
    CG_TRY(hipStreamSynchronize(h->stream));
    const auto t2 = std::chrono::steady_clock::now();
    st.upload_ms += ms_between(t1, t2);
    CG_TRY(hipEventRecord(h->ev[0], h->stream));
    CG_TRY(bz::launch_inflate((const uint8_t*)h->d_comp, (const bz::BlockDesc*)h->d_tab, (int64_t)tab.size(), (uint8_t*)h->d_infl,
                              (int32_t*)h->d_bstatus, h->stream));
    CG_TRY(hipEventRecord(h->ev[1], h->stream));
    std::vector<int32_t> bstatus(tab.size());
    if (!tab.empty()) CG_TRY(hipMemcpyAsync(bstatus.data(), h->d_bstatus, tab.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    CG_TRY(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < tab.size(); ++i)
        if (bstatus[i] != BZ_OK)
            return fail(-3, "BGZF block fails its CRC / size check (%s, block at file offset %llu)", bz_status_text(bstatus[i]),
                        (unsigned long long)blocks[i].coff);
    std::vector<bz::SubRange> sr(n_subs);
    for (uint32_t s = 0; s < n_subs; ++s) sr[s] = bz::SubRange{regions[b0 + s].tid, regions[b0 + s].start, regions[b0 + s].end};
    const cand::ReadMeta* meta_dev = nullptr;
    uint64_t n_reads = 0, n_records = 0, err = bz::NO_ERROR;
    const char* msg = nullptr;
    CG_TRY(hipEventRecord(h->ev[2], h->stream));
    if (bz::frame_records(h->framer, (const uint8_t*)h->d_infl, infl_bytes, segs.data(), segs.size(), n_slots, sr.data(), n_subs, h->stream,
                          &meta_dev, &n_reads, &n_records, &err, &msg))
        return fail(-2, "device framing: %s", msg);
    if (err != bz::NO_ERROR)
        return fail(-3, "%s (record at virtual offset %lld)", bamn::frame::why_text((uint32_t)(err & 0xff)), (long long)pl.voff_of(err >> 8));
    CG_TRY(hipEventRecord(h->ev[3], h->stream));
    CG_TRY(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    CG_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ist.inflate_ms += ms;
    CG_TRY(hipEventElapsedTime(&ms, h->ev[2], h->ev[3]));
    h->ist.walk_frame_ms += ms;
    h->ist.records += (int64_t)n_records;
#undef CG_TRY
    std::vector<cand::SubDesc> subs(n_subs);
    int64_t cov = 0;
    for (uint32_t s = 0; s < n_subs; ++s) {
        const cg_region& rg = regions[b0 + s];
        subs[s].start = rg.start;
        subs[s].end = rg.end;
        subs[s].cov_base = cov;
        cov += (int64_t)rg.end - rg.start + 2;
    }
    if (cand::upload_device(h->ws, (const uint8_t*)h->d_infl, meta_dev, subs.data(), n_subs, cov, h->stream, &msg))
        return fail(-2, "device upload: %s", msg);
    return finish_batch(h, regions, b0, n_reads, n_subs, cov, st);
}

}  // namespace

extern "C" {

const char* cg_last_error(void) { return g_err.c_str(); }

int cg_open(const char* bam_path, const char* bai_path, const cg_options* opt, cg_handle_t** out) {
    try {
        if (!out || !bam_path || !opt) return fail(-1, "cg_open: null argument");
        *out = nullptr;
        if (opt->max_len_indel_allele > CG_MAX_ALLELE_LEN)
            return fail(-1, "max_len_indel_allele %d exceeds the allele key's limit of %d bases", opt->max_len_indel_allele,
                        CG_MAX_ALLELE_LEN);
        std::unique_ptr<cg_handle> h(new cg_handle());
        h->bam_path = bam_path;
        h->opt = *opt;
        if (h->opt.threads <= 0) h->opt.threads = 1;
        if (!h->header.open(bam_path)) return fail(-3, "%s", h->header.err.c_str());
        if (bai_path && *bai_path) {
            if (!h->bai.load(bai_path)) return fail(-3, "cannot read the BAI index %s", bai_path);
            h->have_bai = true;
        }
        *out = h.release();
        return 0;
    } catch (const std::exception& e) {
        return fail(-4, "cg_open: %s", e.what());
    } catch (...) {
        return fail(-4, "cg_open: unknown exception");
    }
}

int cg_run(cg_handle_t* h, const cg_region* regions, int64_t n_regions, const cg_candidate** out, int64_t* n_out, cg_stats* stats) {
    try {
        if (!h || !out || !n_out || (n_regions > 0 && !regions)) return fail(-1, "cg_run: null argument");
        const auto t0 = std::chrono::steady_clock::now();
        cg_stats st{};
        h->ist = cg_inflate_stats{};
        h->out.clear();
        for (int64_t i = 0; i < n_regions; ++i) {
            const cg_region& r = regions[i];
            if (r.tid < 0 || r.tid >= (int)h->header.refs.size()) return fail(-1, "region %lld: tid %d not in the BAM header", (long long)i, r.tid);
            if (r.start < 0 || r.end < r.start) return fail(-1, "region %lld: bad interval [%d, %d)", (long long)i, r.start, r.end);
        }
        int64_t b0 = 0;
        while (b0 < n_regions) {
            int64_t b1 = b0, len = 0;
            while (b1 < n_regions && (b1 == b0 || (len + regions[b1].end - regions[b1].start <= BATCH_BASES && b1 - b0 < MAX_BATCH_SUBS))) {
                len += (int64_t)regions[b1].end - regions[b1].start;
                ++b1;
            }
            const int rc = h->inflate_device ? run_batch_device(h, regions, b0, b1, st) : run_batch(h, regions, b0, b1, st);
            if (rc) return rc;
            b0 = b1;
        }
        st.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (stats) *stats = st;
        *out = h->out.data();
        *n_out = (int64_t)h->out.size();
        return 0;
    } catch (const std::exception& e) {
        return fail(-4, "cg_run: %s", e.what());
    } catch (...) {
        return fail(-4, "cg_run: unknown exception");
    }
}

int cg_set_inflate_device(cg_handle_t* h, int on) {
    try {
        if (!h) return fail(-1, "cg_set_inflate_device: null handle");
        if (on && !h->have_bai)
            return fail(-1, "inflate on the device needs the BAI index of %s: its bins give the byte ranges to read", h->bam_path.c_str());
        if (on && h->fd < 0 && (h->fd = open(h->bam_path.c_str(), O_RDONLY)) < 0) return fail(-3, "cannot open %s", h->bam_path.c_str());
        h->inflate_device = on != 0;
        return 0;
    } catch (...) {
        return fail(-4, "cg_set_inflate_device: unknown exception");
    }
}

int cg_get_inflate_stats(const cg_handle_t* h, cg_inflate_stats* out) {
    if (!h || !out) return fail(-1, "cg_get_inflate_stats: null argument");
    *out = h->ist;
    return 0;
}

int cg_debug_ranges(const cg_handle_t* h, int32_t tid, int32_t start, int32_t end, uint64_t* ranges, int64_t cap_ranges, int64_t* n_ranges,
                    uint64_t* bounds, int64_t cap_bounds, int64_t* n_bounds) {
    try {
        if (!h || !n_ranges || !n_bounds) return fail(-1, "cg_debug_ranges: null argument");
        if (!h->have_bai) return fail(-1, "cg_debug_ranges: the handle has no BAI index");
        const cg_region rg{tid, start, end};
        bz::BlockPlan pl;
        pl.plan(h->bai, &rg, 1);
        *n_ranges = (int64_t)pl.ranges.size();
        int64_t nb = 0;
        for (size_t r = 0; r < pl.ranges.size(); ++r) {
            if (ranges && (int64_t)r < cap_ranges) { ranges[2 * r] = pl.ranges[r].first; ranges[2 * r + 1] = pl.ranges[r].second; }
            for (const uint64_t v : pl.bounds[r]) {
                if (bounds && nb < cap_bounds) bounds[nb] = v;
                ++nb;
            }
        }
        *n_bounds = nb;
        return 0;
    } catch (const std::exception& e) {
        return fail(-4, "cg_debug_ranges: %s", e.what());
    } catch (...) {
        return fail(-4, "cg_debug_ranges: unknown exception");
    }
}

int32_t cg_n_refs(const cg_handle_t* h) { return h ? (int32_t)h->header.refs.size() : 0; }
const char* cg_ref_name(const cg_handle_t* h, int32_t tid) {
    return (h && tid >= 0 && tid < (int32_t)h->header.refs.size()) ? h->header.refs[tid].c_str() : nullptr;
}
int64_t cg_ref_length(const cg_handle_t* h, int32_t tid) {
    return (h && tid >= 0 && tid < (int32_t)h->header.lengths.size()) ? h->header.lengths[tid] : -1;
}

void cg_close(cg_handle_t* h) {
    try {
        delete h;
    } catch (...) {
    }
}

}  // extern "C"
