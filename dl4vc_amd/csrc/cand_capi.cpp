// Host side of libdl4vc_cand.so (C ABI: include/dl4vc_candgen.h).  Worker threads, each with its own BAM handle, fetch the
// records of a batch of subregions (BAI linear index, htslib's overlap rule: pos < end and bam_endpos > start, no flag
// filter), frame and validate every record (the frame core of bam_frame.h) and gather them into one pinned buffer; the device
// does the rest (cand_kernels.hip).  A read overlapping two subregions is listed once for each, as the reference's per
// subregion fetch counts it.  Every extern "C" body catches what it throws: a corrupt file is an error code, never an abort.
//
// With cg_set_inflate_device() the host does none of that: run_batch_device() takes the batch's byte ranges from the BAI bins,
// reads their BGZF blocks as they are into pinned memory, and the device inflates them, walks the record chain, frames the
// records and lists them per subregion (bgzf_kernels.hip); the same count / emit / filter kernels follow.
//
// With cg_set_reference() a read without MD is walked against the FASTA's bases of its contig: batch_refs() makes the contigs a
// batch touches resident (load_contig(): the raw byte range read with fasta_native.h's index, uploaded, and turned into one code
// per base by reference_codes_kernel) and hands the kernels one RefDesc per subregion, on either record path.
//
// With cg_set_left_align() (which needs the reference) the kernels move every insertion and deletion to its left-most placement
// on those bases before it is counted (cand_left_align.h); finish_batch() sums the counters of the batches.
#include "../../include/dl4vc_candgen.h"
#include "bam_frame.h"
#include "bam_native.h"
#include "bgzf_device.h"
#include "cand_device.h"
#include "cand_reference.h"
#include "fasta_native.h"

#include <atomic>
#include <chrono>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace cand {
std::string& last_error();     // this thread's error text (cand_reference_capi.cpp, with cg_last_error)
}

namespace {

thread_local std::string& g_err = cand::last_error();

template <class... A>
int fail(int code, const char* fmt, A... a) { return capi::failf(g_err, code, fmt, a...); }

const char BASES[] = "=ACMGRSVTWYHKDBN";
constexpr int64_t BATCH_BASES = 4000000;     // subregion length gathered per device batch
constexpr uint32_t MAX_BATCH_SUBS = 1u << 20;

struct Gathered {
    std::vector<uint8_t> bytes;
    std::vector<cand::ReadMeta> meta;   // off relative to bytes
    std::string err;
    int64_t seen = 0;                   // records that passed the region test and the read filter, in front of the sample rule
    bamn::frame::Census census;         // filled when the handle collects the read census
};

}  // namespace

struct cg_handle {   // (members are destroyed last to first: the stream outlives everything that was used on it)
    std::string bam_path;
    bamn::BamFile header;
    bamn::Bai bai;
    bool have_bai = false;
    cg_options opt{};
    dev::Stream stream;
    std::unique_ptr<cand::Workspace, void (*)(cand::Workspace*)> ws{nullptr, cand::workspace_destroy};
    dev::Pinned pinned;                         // the gathered records of the host framing path
    std::vector<cg_candidate> out;
    // the device inflate path (cg_set_inflate_device)
    bool inflate_device = false;
    bz::InflateStage inflate;
    std::unique_ptr<bz::Framer, void (*)(bz::Framer*)> framer{nullptr, bz::framer_destroy};
    dev::Event ev[2];                           // around walk + frame
    cg_inflate_stats ist{};
    // the reference source (cg_set_reference): whole contigs as codes, loaded at the first batch that touches them
    std::string fasta_path;
    std::unique_ptr<fastan::Fasta> fasta;
    std::map<int32_t, dev::Buffer> contigs;     // tid -> exactly header.lengths[tid] bytes
    cg_reference_stats rst{};
    // left-alignment of indels (cg_set_left_align): needs the reference source
    bool left_align = false;
    cg_left_align_stats lst{};
    // read subsampling (cg_set_subsample)
    bamn::frame::SampleRule sample{0, 0};
    cg_subsample_stats sst{};
    // read filter and census (cg_set_read_filter, cg_set_read_stats): the census is collected with a filter or when asked for
    bamn::frame::ReadFilter filter{0, 0, 0};
    bool read_stats = false;
    bamn::frame::Census census;
    bool collects() const { return read_stats || bamn::frame::filter_on(filter); }
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
        const uint32_t fate = F::fate(h->collects() ? &g.census : nullptr, blk.data(), fr, h->filter, h->sample);
        if (fate == F::FATE_FILTERED) continue;
        ++g.seen;
        if (fate != F::FATE_KEPT) continue;
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

// ---- the reference source ---------------------------------------------------------------------------------------------------
// The contig of tid as codes in `codes` (exactly its length in bytes): its raw byte range, line breaks included, read from the
// FASTA, uploaded and converted by reference_codes_kernel.  The caller has set the device and created the stream.
int load_contig(cg_handle* h, int32_t tid, dev::Buffer& codes) {
    namespace R = cand::refc;
    const int64_t length = h->header.lengths[tid];
    const char* name = h->header.refs[tid].c_str();
    const char* fa = h->fasta_path.c_str();
    const fastan::Fasta::Entry* e = h->fasta->entry(h->header.refs[tid]);
    if (!e) return fail(-3, "reference: contig %s of the BAM header is not in %s", name, fa);
    if (e->length != length)
        return fail(-3, "reference: contig %s has %lld bases in %s and %lld in the BAM header: not the reference these reads were aligned to",
                    name, (long long)e->length, fa, (long long)length);
    if (!R::layout_ok(e->lb, e->lw, length) || e->offset < 0)
        return fail(-3, "reference: contig %s: the index of %s gives lines of %lld bases in %lld bytes", name, fa, (long long)e->lb,
                    (long long)e->lw);
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t span = R::raw_span(e->lb, e->lw, length);
    std::vector<uint8_t> raw(span);
    uint64_t got = 0;
    if (span) {
        if (fseeko(h->fasta->f, (off_t)e->offset, SEEK_SET) != 0) return fail(-3, "reference: cannot seek to contig %s in %s", name, fa);
        got = fread(raw.data(), 1, span, h->fasta->f);       // (a short read leaves base positions past the bytes: refused below)
    }
    const auto t1 = std::chrono::steady_clock::now();
#define CG_TRY(x) DEV_TRY(g_err, "reference: ", x)
    dev::Buffer d_raw;
    dev::Array<unsigned long long> d_counts;
    unsigned long long counts[2] = {0, R::NONE};
    CG_TRY(codes.alloc((size_t)std::max<int64_t>(length, 1)));
    CG_TRY(d_raw.alloc(got + 16));
    CG_TRY(d_counts.alloc(2));
    if (got) CG_TRY(hipMemcpy(d_raw.p, raw.data(), got, hipMemcpyHostToDevice));      // (pageable memory: complete on return)
    CG_TRY(hipMemcpy(d_counts.p, counts, sizeof counts, hipMemcpyHostToDevice));
    CG_TRY(cand::launch_reference_codes(d_raw.p, got, e->lb, e->lw, length, codes.p, d_counts.p, h->stream));
    CG_TRY(hipStreamSynchronize(h->stream));
    CG_TRY(hipMemcpy(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost));
#undef CG_TRY
    if (counts[1] != R::NONE)
        return fail(-3, "reference: contig %s: a line end, '>' or the end of the file at base %llu: the index of %s (lines of %lld bases in "
                    "%lld bytes from offset %lld) does not describe the file", name, counts[1], fa, (long long)e->lb, (long long)e->lw,
                    (long long)e->offset);
    const auto t2 = std::chrono::steady_clock::now();
    ++h->rst.contigs;
    h->rst.bases += length;
    h->rst.other_bytes += (int64_t)counts[0];
    h->rst.read_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->rst.upload_convert_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
    return 0;
}

// one RefDesc per subregion of the batch (none when the reference is off); contigs not yet resident are loaded
int batch_refs(cg_handle* h, const cg_region* regions, int64_t b0, uint32_t n_subs, std::vector<cand::RefDesc>& refs) {
    refs.clear();
    if (!h->fasta) return 0;
    refs.resize(n_subs);
    for (uint32_t s = 0; s < n_subs; ++s) {
        const int32_t tid = regions[b0 + s].tid;
        auto it = h->contigs.find(tid);
        if (it == h->contigs.end()) {
            it = h->contigs.try_emplace(tid).first;
            if (const int rc = load_contig(h, tid, it->second)) { h->contigs.erase(it); return rc; }
        }
        refs[s] = cand::RefDesc{it->second.p, h->header.lengths[tid]};
    }
    return 0;
}

// the counting kernels over what upload() / upload_device() left in the workspace, and the batch's results
int finish_batch(cg_handle* h, const cg_region* regions, int64_t b0, uint64_t n_reads, uint32_t n_subs, int64_t cov, cg_stats& st) {
    const char* msg = nullptr;
    const cand::DevCand* dc = nullptr;
    const uint8_t* status = nullptr;
    uint64_t n_out = 0, n_events = 0, n_unique = 0;
    cand::BatchTimes bt{};
    uint64_t la[cand::LA_COUNTERS];
    if (cand::run_batch(h->ws.get(), n_reads, n_subs, cov, h->opt.max_len_indel_allele, h->opt.snp_min_freq, h->opt.indel_min_freq,
                        h->left_align, h->stream, &dc, &n_out, &status, &n_events, &n_unique, la, &bt, &msg))
        return fail(-2, "device: %s", msg);
    h->lst.observations += (int64_t)la[cand::LA_SEEN];
    h->lst.shifted += (int64_t)la[cand::LA_SHIFTED];
    h->lst.bases_shifted += (int64_t)la[cand::LA_BASES];
    h->lst.clamped += (int64_t)la[cand::LA_CLAMPED];
    h->lst.not_eligible += (int64_t)la[cand::LA_NOT_ELIGIBLE];
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
        if (v & cand::ST_REFERENCE) ++h->rst.reads;
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
    if (h->stream.ensure() != hipSuccess) return fail(-2, "hipStreamCreate failed");
    if (!h->ws) h->ws.reset(cand::workspace_create());
    if (!h->ws) return fail(-2, "cannot create the device workspace");
    std::vector<cand::RefDesc> refs;
    if (const int rc = batch_refs(h, regions, b0, n_subs, refs)) return rc;
    // gather into the pinned buffer, subregion by subregion
    uint64_t bytes = 0, n_reads = 0;
    for (auto& g : per) { bytes += g.bytes.size(); n_reads += g.meta.size(); h->sst.records_seen += g.seen; }
    if (h->collects())
        for (auto& g : per) h->census.add(g.census);
    h->sst.records_kept += (int64_t)n_reads;
    if (h->pinned.ensure(bytes + 1) != hipSuccess) return fail(-2, "pinned allocation of %llu bytes failed", (unsigned long long)bytes);
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
        if (!g.bytes.empty()) memcpy(h->pinned.p + at, g.bytes.data(), g.bytes.size());
        for (auto m : g.meta) { m.off += at; meta.push_back(m); }
        at += g.bytes.size();
        std::vector<uint8_t>().swap(g.bytes);
    }
    const auto t1 = std::chrono::steady_clock::now();
    st.host_frame_ms += std::chrono::duration<double, std::milli>(t1 - t0).count();
    const char* msg = nullptr;
    if (cand::upload(h->ws.get(), h->pinned.p, bytes, meta.data(), n_reads, subs.data(), refs.empty() ? nullptr : refs.data(), n_subs, cov,
                     h->stream, &msg))
        return fail(-2, "device upload: %s", msg);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(-2, "device upload failed");
    const auto t2 = std::chrono::steady_clock::now();
    st.upload_ms += std::chrono::duration<double, std::milli>(t2 - t1).count();
    return finish_batch(h, regions, b0, n_reads, n_subs, cov, st);
}

// ---- the device inflate path ---------------------------------------------------------------------------------------------
double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
}

#define CG_TRY(x) DEV_TRY(g_err, "device inflate: ", x)

int run_batch_device(cg_handle* h, const cg_region* regions, int64_t b0, int64_t b1, cg_stats& st) {
    const uint32_t n_subs = (uint32_t)(b1 - b0);
    const auto t0 = std::chrono::steady_clock::now();
    bz::BlockPlan pl;
    std::string perr;
    pl.plan(h->bai, regions + b0, b1 - b0);
    if (hipSetDevice(h->opt.device) != hipSuccess) return fail(-2, "hipSetDevice(%d) failed", h->opt.device);
    if (const int rc = h->inflate.read(pl, h->bam_path, g_err)) return rc;
    if (!pl.segments(perr)) return fail(-3, "%s", perr.c_str());
    const uint64_t infl_bytes = pl.infl_bytes;
    const auto t1 = std::chrono::steady_clock::now();
    st.host_frame_ms += ms_between(t0, t1);
    h->ist.read_ms += ms_between(t0, t1);
    h->ist.blocks += (int64_t)pl.blocks.size();
    h->ist.compressed_bytes += (int64_t)pl.comp_bytes;
    h->ist.inflated_bytes += (int64_t)infl_bytes;
    // the device
    if (h->stream.ensure() != hipSuccess) return fail(-2, "hipStreamCreate failed");
    if (!h->ws) h->ws.reset(cand::workspace_create());
    if (!h->ws) return fail(-2, "cannot create the device workspace");
    if (!h->framer) h->framer.reset(bz::framer_create());
    for (dev::Event& e : h->ev)
        if (e.ensure() != hipSuccess) return fail(-2, "hipEventCreate failed");
    if (const int rc = h->inflate.upload(pl, h->stream, g_err)) return rc;
    CG_TRY(hipStreamSynchronize(h->stream));
    st.upload_ms += ms_between(t1, std::chrono::steady_clock::now());
    if (const int rc = h->inflate.enqueue(pl, h->stream, g_err)) return rc;
    if (const int rc = h->inflate.finish(pl, h->stream, &h->ist.inflate_ms, g_err)) return rc;
    std::vector<bz::SubRange> sr(n_subs);
    for (uint32_t s = 0; s < n_subs; ++s) sr[s] = bz::SubRange{regions[b0 + s].tid, regions[b0 + s].start, regions[b0 + s].end};
    const cand::ReadMeta* meta_dev = nullptr;
    uint64_t n_reads = 0, n_records = 0, n_seen = 0, err = bz::NO_ERROR;
    const char* msg = nullptr;
    CG_TRY(hipEventRecord(h->ev[0], h->stream));
    if (bz::frame_records(h->framer.get(), h->inflate.d_infl.p, infl_bytes, pl.segs.data(), pl.segs.size(), pl.n_slots, sr.data(), n_subs,
                          h->stream, &meta_dev, &n_reads, &n_records, &err, &msg, h->sample, &n_seen, h->filter,
                          h->collects() ? &h->census : nullptr))
        return fail(-2, "device framing: %s", msg);
    if (err != bz::NO_ERROR)
        return fail(-3, "%s (record at virtual offset %lld)", bamn::frame::why_text((uint32_t)(err & 0xff)), (long long)pl.voff_of(err >> 8));
    CG_TRY(hipEventRecord(h->ev[1], h->stream));
    CG_TRY(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    CG_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ist.walk_frame_ms += ms;
    h->ist.records += (int64_t)n_records;
    h->sst.records_seen += (int64_t)n_seen;
    h->sst.records_kept += (int64_t)n_reads;
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
    std::vector<cand::RefDesc> refs;
    if (const int rc = batch_refs(h, regions, b0, n_subs, refs)) return rc;
    if (cand::upload_device(h->ws.get(), h->inflate.d_infl.p, meta_dev, subs.data(), refs.empty() ? nullptr : refs.data(), n_subs, cov,
                            h->stream, &msg))
        return fail(-2, "device upload: %s", msg);
    return finish_batch(h, regions, b0, n_reads, n_subs, cov, st);
}

}  // namespace

extern "C" {

int cg_open(const char* bam_path, const char* bai_path, const cg_options* opt, cg_handle_t** out) {
    return capi::guarded(g_err, "cg_open", [&] {
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
    });
}

int cg_run(cg_handle_t* h, const cg_region* regions, int64_t n_regions, const cg_candidate** out, int64_t* n_out, cg_stats* stats) {
    return capi::guarded(g_err, "cg_run", [&] {
        if (!h || !out || !n_out || (n_regions > 0 && !regions)) return fail(-1, "cg_run: null argument");
        const auto t0 = std::chrono::steady_clock::now();
        cg_stats st{};
        h->ist = cg_inflate_stats{};
        h->rst.reads = 0;
        h->lst = cg_left_align_stats{};
        h->sst = cg_subsample_stats{};
        h->census = bamn::frame::Census{};
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
    });
}

int cg_set_inflate_device(cg_handle_t* h, int on) {
    return capi::guarded(g_err, "cg_set_inflate_device", [&] {
        if (!h) return fail(-1, "cg_set_inflate_device: null handle");
        if (on && !h->have_bai)
            return fail(-1, "inflate on the device needs the BAI index of %s: its bins give the byte ranges to read", h->bam_path.c_str());
        if (on && !h->inflate.open(h->bam_path)) return fail(-3, "cannot open %s", h->bam_path.c_str());
        h->inflate_device = on != 0;
        return 0;
    });
}

int cg_get_inflate_stats(const cg_handle_t* h, cg_inflate_stats* out) {
    if (!h || !out) return fail(-1, "cg_get_inflate_stats: null argument");
    *out = h->ist;
    return 0;
}

int cg_set_subsample(cg_handle_t* h, double fraction, uint32_t seed) {
    return capi::guarded(g_err, "cg_set_subsample", [&] {
        if (!h) return fail(-1, "cg_set_subsample: null handle");
        if (const char* why = bamn::frame::sample_rule(fraction, seed, h->sample)) return fail(-1, "cg_set_subsample: %s", why);
        return 0;
    });
}

int cg_get_subsample_stats(const cg_handle_t* h, cg_subsample_stats* out) {
    if (!h || !out) return fail(-1, "cg_get_subsample_stats: null argument");
    *out = h->sst;
    return 0;
}

int cg_set_read_filter(cg_handle_t* h, int32_t exclude, int32_t require, int32_t min_mapq) {
    return capi::guarded(g_err, "cg_set_read_filter", [&] {
        if (!h) return fail(-1, "cg_set_read_filter: null handle");
        if (const char* why = bamn::frame::read_filter(exclude, require, min_mapq, h->filter)) return fail(-1, "cg_set_read_filter: %s", why);
        return 0;
    });
}

int cg_set_read_stats(cg_handle_t* h, int on) {
    if (!h) return fail(-1, "cg_set_read_stats: null handle");
    h->read_stats = on != 0;
    return 0;
}

int cg_get_read_stats(const cg_handle_t* h, dl4vc_read_stats* out) {
    if (!h || !out) return fail(-1, "cg_get_read_stats: null argument");
    static_assert(sizeof(dl4vc_read_stats) == sizeof(h->census.w), "dl4vc_read_stats is the census's words");
    memcpy(out, h->census.w, sizeof(*out));
    return 0;
}

int cg_set_reference(cg_handle_t* h, const char* fasta_path) {
    return capi::guarded(g_err, "cg_set_reference", [&] {
        if (!h) return fail(-1, "cg_set_reference: null handle");
        std::unique_ptr<fastan::Fasta> fa;
        if (h->left_align && !(fasta_path && *fasta_path))
            return fail(-1, "cg_set_reference: left-alignment is on and takes its bases from the reference: switch it off first "
                        "(cg_set_left_align(h, 0))");
        if (fasta_path && *fasta_path) {
            std::string err;
            fa.reset(new fastan::Fasta());
            if (!fa->open(fasta_path, err)) return fail(-3, "reference: %s", err.c_str());
        }
        h->contigs.clear();                     // (codes of another file, or of none)
        h->rst = cg_reference_stats{};
        h->fasta = std::move(fa);
        h->fasta_path = h->fasta ? fasta_path : "";
        return 0;
    });
}

int cg_get_reference_stats(const cg_handle_t* h, cg_reference_stats* out) {
    if (!h || !out) return fail(-1, "cg_get_reference_stats: null argument");
    *out = h->rst;
    return 0;
}

int cg_set_left_align(cg_handle_t* h, int on) {
    return capi::guarded(g_err, "cg_set_left_align", [&] {
        if (!h) return fail(-1, "cg_set_left_align: null handle");
        if (on && !h->fasta)
            return fail(-1, "cg_set_left_align: left-alignment is defined by the reference bases and no reference is set: call "
                        "cg_set_reference first");
        h->left_align = on != 0;
        return 0;
    });
}

int cg_get_left_align_stats(const cg_handle_t* h, cg_left_align_stats* out) {
    if (!h || !out) return fail(-1, "cg_get_left_align_stats: null argument");
    *out = h->lst;
    return 0;
}

int cg_debug_ranges(const cg_handle_t* h, int32_t tid, int32_t start, int32_t end, uint64_t* ranges, int64_t cap_ranges, int64_t* n_ranges,
                    uint64_t* bounds, int64_t cap_bounds, int64_t* n_bounds) {
    return capi::guarded(g_err, "cg_debug_ranges", [&] {
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
    });
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
