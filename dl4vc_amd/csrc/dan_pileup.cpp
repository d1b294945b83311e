// Native pileup encoder: BAM + FASTA + candidate locations -> the image planes of the
// candidate records main.py scores.  Part of libdl4vc_loader.so (C ABI: include/dl4vc_loader.h, pe_*).
//
// Restates, for the common case, what dl4vc_amd/pileup_encoder.py::process_tracks + finish_record compute -- themselves the
// read-by-read form of the reference's tools/convert_bam_single_reads.py::process_location (:846-1118) and the crop / centre
// / pad step of process_locations_chunk (:720-838) -- together with the layers under them: BGZF blocks (zlib raw inflate +
// CRC), BAM header / records (SAM specification section 4.2), the BAI linear index (section 5.2), a forward-moving window
// over the alignments (each record inflated and parsed once per run of locations), per-read CIGAR resolution (htslib's
// pileup rules: qpos / is_del / is_refskip / merged indel lengths) and FASTA + .fai access.  A location the read-by-read form
// declines (two reads sharing a name:sequence key, a reference skip, a base outside the token table, > 1000 columns, > 8000
// reads) is reported back as status 2 and takes the Python column-by-column path: results are byte-identical to the Python
// module by construction (tests/test_pileup_native.py).  Status 2 as well, with a ValueError on the Python side: a read inside
// the window whose alignment has no reference position (0M 5I) or whose SEQ is shorter than its CIGAR's query length (SEQ '*');
// tests/test_pileup_edges.py.  Worker threads take contiguous runs of locations, each with its own file handles and window.
#include "../../include/dl4vc_loader.h"
#include "bam_native.h"
#include "capi_shell.h"
#include "fasta_native.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

namespace {

std::string g_pe_error;

// ---- token tables (tools/convert_bam_single_reads.py:38-56; dl4vc_amd/pileup_encoder.py::BASE_ENUM) ---------------------------
constexpr uint8_t PAD = 0, START = 6, END = 7, NOINSERT = 8, STRAND_PAD = 200, STRAND_LOWER = 1, STRAND_UPPER = 2, TOK_GAP = 5;
struct Tables {
    uint8_t token[256];
    bool known[256];
    Tables() {
        memset(token, 0, sizeof token);
        memset(known, 0, sizeof known);
        auto set = [&](const char* cs, uint8_t v) { for (; *cs; ++cs) { token[(uint8_t)*cs] = v; known[(uint8_t)*cs] = true; } };
        set("Aa", 1); set("TtUu", 2); set("Gg", 3); set("Cc", 4); set("-*NnXx.,", 5); set("e", 7);
        set("?MmKkRrYySsWwBbVvHhDd", 9);
    }
};
const Tables T;
const char SEQ_CODES[] = "=ACMGRSVTWYHKDBN";
enum { CMATCH, CINS, CDEL, CREF_SKIP, CSOFT_CLIP, CHARD_CLIP, CPADOP, CEQUAL, CDIFF };
inline bool is_aligned(int op) { return op == CMATCH || op == CEQUAL || op == CDIFF; }
inline bool is_refop(int op) { return is_aligned(op) || op == CDEL || op == CREF_SKIP; }
constexpr int FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400;          // unmapped, secondary, QC fail, duplicate (BAM_DEF_MASK)
constexpr int FREVERSE = 0x10;

using bamn::Bgzf;
using bamn::Bai;

struct Rec {
    int32_t tid = -1, pos = 0, ref_end = 0;
    uint16_t flag = 0;
    bool sampled = true;                                         // false: the read filter or the sample rule dropped it
    uint8_t mapq = 0, verdict = 0;                               // bamn::frame::Verdict of the read filter (0: it passes)
    std::string name, seq;
    std::vector<uint32_t> cigar;                                 // (len << 4) | op
    std::vector<uint8_t> qual;
    // resolved against the reference (pileup.py::ReadTrack), filled on first use
    bool resolved = false, has_ref = false, short_seq = false;     // short_seq: the CIGAR implies query bases SEQ lacks
    int32_t start = 0, end = 0;
    std::vector<int32_t> qpos, indel;
    std::vector<uint8_t> is_del, is_skip;

    void resolve() {
        if (resolved) return;
        resolved = true;
        int n = 0;
        for (uint32_t c : cigar) if (is_refop(c & 0xf)) n += (int)(c >> 4);
        has_ref = false;
        for (uint32_t c : cigar) if (is_refop(c & 0xf)) has_ref = true;
        start = pos; end = pos + n;
        int64_t nq = 0;
        for (uint32_t c : cigar) { const int op = c & 0xf; if (is_aligned(op) || op == CINS || op == CSOFT_CLIP) nq += (int64_t)(c >> 4); }
        short_seq = nq > (int64_t)seq.size();
        qpos.assign(n, 0); indel.assign(n, 0); is_del.assign(n, 0); is_skip.assign(n, 0);
        int x = 0, y = 0;
        const int nc = (int)cigar.size();
        for (int k = 0; k < nc; ++k) {
            const int op = cigar[k] & 0xf, l = (int)(cigar[k] >> 4);
            if (is_aligned(op)) { for (int i = 0; i < l; ++i) qpos[x + i] = y + i; x += l; y += l; }
            else if (op == CDEL || op == CREF_SKIP) {
                for (int i = 0; i < l; ++i) { qpos[x + i] = y; is_del[x + i] = 1; is_skip[x + i] = op == CREF_SKIP; }
                x += l;
            } else if (op == CINS || op == CSOFT_CLIP) y += l;
            if (is_refop(op) && x > 0 && k + 1 < nc) {
                const int op2 = cigar[k + 1] & 0xf, l2 = (int)(cigar[k + 1] >> 4);
                int v = 0;
                if (op2 == CDEL && op != CDEL) {
                    v = -l2;
                    for (int j = k + 2; j < nc; ++j) { if ((int)(cigar[j] & 0xf) != CDEL) break; v -= (int)(cigar[j] >> 4); }
                } else if (op2 == CINS) {
                    v = l2;
                    for (int j = k + 2; j < nc; ++j) {
                        const int op3 = cigar[j] & 0xf;
                        if (op3 == CINS) v += (int)(cigar[j] >> 4);
                        else if (op3 != CPADOP) break;
                    }
                } else if (op2 == CPADOP && k + 2 < nc) {
                    for (int j = k + 2; j < nc; ++j) {
                        const int op3 = cigar[j] & 0xf;
                        if (op3 == CINS) v += (int)(cigar[j] >> 4);
                        else if (is_refop(op3)) break;
                    }
                }
                indel[x - 1] = v;
            }
        }
    }
};

using fastan::Fasta;

struct Bam : bamn::BamFile {
    std::vector<uint8_t> b;
    bamn::frame::SampleRule sample{0, 0};                        // pe_set_subsample
    bamn::frame::ReadFilter filter{0, 0, 0};                     // pe_set_read_filter
    int get_tid(const std::string& name) const {
        auto it = tid_of.find(name);
        if (it != tid_of.end()) return it->second;
        const std::string alt = name.rfind("chr", 0) == 0 ? name.substr(3) : "chr" + name;
        it = tid_of.find(alt);
        return it == tid_of.end() ? -1 : it->second;
    }
    // next record; 0 = end of file, 1 = ok, -1 = error
    int next(std::shared_ptr<Rec>& out) {
        const int g = next_block(b);
        if (g <= 0) return g;
        // framed by the one core (bam_frame.h), aux area not walked; the span is not a reason to refuse a record here
        bamn::frame::Framed fr;
        const uint32_t why = bamn::frame::frame_record(b.data(), b.size(), fr, /*aux=*/false);
        if (why != bamn::frame::W_NONE) { err = bamn::frame::why_text(why); return -1; }
        bamn::frame::cigar_sums(b.data(), fr);
        auto rec = std::make_shared<Rec>();
        rec->tid = fr.tid; rec->pos = fr.pos; rec->flag = (uint16_t)fr.flag;
        rec->ref_end = (int32_t)(fr.pos + (fr.nref > 0 ? fr.nref : 1));
        rec->mapq = (uint8_t)bamn::frame::mapq_of(b.data());
        rec->verdict = (uint8_t)bamn::frame::verdict(fr.flag, rec->mapq, filter);
        rec->sampled = bamn::frame::fate(nullptr, b.data(), fr, filter, sample) == bamn::frame::FATE_KEPT;
        rec->name.assign((const char*)&b[32], (size_t)fr.l_name - 1);
        rec->cigar.resize(fr.n_cig);
        for (uint32_t i = 0; i < fr.n_cig; ++i) rec->cigar[i] = bamn::frame::ld32(&b[fr.cigar_off + 4 * i]);
        rec->seq.resize((size_t)fr.l_seq);
        for (int32_t i = 0; i < fr.l_seq; ++i) {
            const uint8_t p = b[fr.seq_off + i / 2];
            rec->seq[i] = SEQ_CODES[(i & 1) ? (p & 0xf) : (p >> 4)];
        }
        rec->qual.assign(b.begin() + fr.qual_off, b.begin() + fr.qual_off + fr.l_seq);
        out = rec;
        return 1;
    }
};

// dl4vc_amd/bamio.py::WindowReader
struct Window {
    Bam* bam = nullptr;
    const Bai* bai = nullptr;
    int64_t max_gap = 1 << 16;
    int tid = -2;
    int64_t last_start = -1, scanned_to = -1, at = 0;
    std::vector<std::shared_ptr<Rec>> kept;
    std::shared_ptr<Rec> pending;
    bool eof = true;
    // with it, every record of a location's window is counted (a dropped one as well, so those stay in `kept` until it passes)
    bamn::frame::Census* census = nullptr;

    bool reads(int t, int64_t start, int64_t stop, std::vector<std::shared_ptr<Rec>>& out) {
        out.clear();
        if (t < 0) return true;
        if (t != tid || start < last_start || start > scanned_to + max_gap) {
            kept.clear(); pending.reset(); tid = t; scanned_to = -1; eof = false;
            at = bam->first_record;
            if (bai) {
                const uint64_t off = bai->linear_offset(t, start);
                if (off == 0) eof = true; else at = (int64_t)off;
            }
        } else {
            size_t w = 0;
            for (auto& r : kept) if (r->ref_end > start) kept[w++] = r;
            kept.resize(w);
        }
        last_start = start;
        if (stop > scanned_to && !eof) {
            std::shared_ptr<Rec> rec = pending;
            pending.reset();
            if (!rec) { if (!bam->r.seek(at)) return false; }
            for (;;) {
                if (!rec) {
                    const int g = bam->next(rec);
                    if (g < 0) return false;
                    if (g == 0) { eof = true; break; }
                }
                if (rec->tid != t) {
                    if (rec->tid > t || rec->tid < 0) { eof = true; break; }
                } else if (rec->pos >= stop) { pending = rec; break; }
                else if (rec->ref_end > start && (rec->sampled || census)) kept.push_back(rec);
                rec.reset();
            }
            at = bam->r.tell();
            scanned_to = stop;
        }
        for (auto& r : kept)
            if (r->pos < stop && r->ref_end > start) {
                if (census) bamn::frame::census_add(*census, r->flag, r->mapq, r->verdict, r->sampled);
                if (r->sampled) out.push_back(r);
            }
        return true;
    }
};

}  // namespace

struct pe_encoder {
    std::string bam_path, bai_path, fasta_path, err;
    pe_options opt{};
    Bai bai;
    bool have_bai = false;
    bamn::frame::SampleRule sample{0, 0};
    // read filter and census (pe_set_read_filter, pe_set_read_stats): the census of the last pe_encode, every location's window
    bamn::frame::ReadFilter filter{0, 0, 0};
    bool read_stats = false;
    bamn::frame::Census census;
    bool collects() const { return read_stats || bamn::frame::filter_on(filter); }
};

namespace {

template <class... A>
int pe_fail(pe_encoder* e, const char* fmt, A... a) { return capi::failf(e ? e->err : g_pe_error, -1, fmt, a...); }

// one location: status 1 = planes written, 0 = no record (the reference counts an error), 2 = needs the Python column path
int encode_one(const pe_options& opt, Window& win, Bam& bam, Fasta& fasta, const std::string& contig, int32_t pos1,
               uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, int32_t* num_reads, std::string& err) {
    const int w = opt.window_size, W = 2 * w + 1, MR = opt.max_reads;
    const int window = w + 2;
    const int64_t start = (int64_t)pos1 - window, stop = (int64_t)pos1 + window + 1;
    const int tid = bam.get_tid(contig);
    if (tid < 0) return 0;
    const int64_t s0 = std::max<int64_t>(start, 0);
    std::string ref;
    if (!fasta.fetch(contig, s0, stop + 64, ref)) return 2;        // (the Python path raises the reference's KeyError)
    std::vector<std::shared_ptr<Rec>> recs;
    if (!win.reads(tid, s0, stop, recs)) { err = bam.err.empty() ? bam.r.err : bam.err; return -1; }
    if (opt.min_base_quality > 0) return 2;
    // resolve_reads + the window filter of process_tracks
    std::vector<Rec*> tracks;
    size_t n_resolved = 0;
    for (auto& rp : recs) {
        Rec& r = *rp;
        if ((r.flag & FLAG_MASK) || r.tid < 0) continue;
        r.resolve();
        if (!r.has_ref) continue;
        ++n_resolved;
        if (r.end > s0 && r.start < stop) {
            // A track with no reference position (0M 5I: has_ref, end == start) has no first base to draw, and one whose SEQ
            // is shorter than its CIGAR's query length (SEQ '*') has no bases: neither has an answer in the specification.
            if (r.end <= r.start || r.short_seq) return 2;
            tracks.push_back(&r);
        }
    }
    if (n_resolved > 8000) return 2;
    {
        std::unordered_set<std::string> keys;
        for (Rec* t : tracks) if (!keys.insert(t->name + ":" + t->seq).second) return 2;
    }
    const int n_pos = (int)(stop - s0);
    std::vector<int> cover(n_pos + 1, 0), longest(n_pos, 0), cap(n_pos, opt.max_insert_length);
    const int ci = pos1 - 1 - (int)s0;
    if (ci >= 0 && ci < n_pos) cap[ci] = std::max(opt.max_insert_length_variant, opt.max_insert_length);
    std::vector<std::pair<int64_t, int64_t>> spans(tracks.size());
    for (size_t i = 0; i < tracks.size(); ++i) {
        Rec* t = tracks[i];
        const int64_t lo = std::max<int64_t>(t->start, s0), hi = std::min<int64_t>(t->end, stop);
        for (int64_t p = lo; p < hi; ++p) if (t->is_skip[p - t->start]) return 2;
        cover[lo - s0] += 1; cover[hi - s0] -= 1;
        for (int64_t p = lo; p < hi; ++p) {
            const int ins = t->indel[p - t->start];
            if (ins > 0) longest[p - s0] = std::max(longest[p - s0], std::min(ins, cap[p - s0]));
        }
        spans[i] = {lo, hi};
    }
    std::vector<int> pos_idx;
    {
        int run = 0;
        for (int p = 0; p < n_pos; ++p) { run += cover[p]; if (run > 0) pos_idx.push_back(p); }
    }
    auto covered = [&](int p) { return std::binary_search(pos_idx.begin(), pos_idx.end(), p); };
    if (pos_idx.empty() || !(ci >= 0 && ci < n_pos && covered(ci))) return 0;
    if (pos_idx.size() > 1001) return 2;
    std::vector<int64_t> col_of(n_pos, 0), prev_col(n_pos, 0);
    int64_t col = 1, prev = 0;
    for (int p : pos_idx) { col_of[p] = col; prev_col[p] = prev; prev = col; col += 1 + longest[p]; }
    const int64_t end_col = col;                                    // the column the loop would give the next position
    std::vector<size_t> order(tracks.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return spans[a].first < spans[b].first; });
    const int n_rows = (int)tracks.size();
    const int n_cols = (int)end_col + 1;
    std::vector<uint8_t> img((size_t)n_rows * n_cols, 0), qimg((size_t)n_rows * n_cols, 0), simg((size_t)n_rows * n_cols, 0);
    for (int row = 0; row < n_rows; ++row) {
        Rec* t = tracks[order[row]];
        const int64_t lo = spans[order[row]].first, hi = spans[order[row]].second;
        const int a = (int)(lo - t->start), nb = (int)(hi - lo);
        uint8_t* I = &img[(size_t)row * n_cols];
        uint8_t* Q = &qimg[(size_t)row * n_cols];
        uint8_t* S = &simg[(size_t)row * n_cols];
        const uint8_t strand = (t->flag & FREVERSE) ? STRAND_LOWER : STRAND_UPPER;
        const int ls = (int)t->seq.size(), lq = (int)t->qual.size();
        std::vector<uint8_t> quals(nb);
        for (int k = 0; k < nb; ++k) {
            const int qp = t->qpos[a + k];
            const bool del = t->is_del[a + k] != 0;
            const uint8_t ch = qp < ls ? (uint8_t)t->seq[qp] : (uint8_t)'N';
            if (!T.known[ch]) return 2;
            const int64_t c = col_of[lo - s0 + k];
            I[c] = del ? TOK_GAP : T.token[ch];
            quals[k] = qp < lq ? t->qual[qp] : 0;
            Q[c] = quals[k];
            S[c] = del ? STRAND_PAD : strand;
        }
        if (t->start >= s0) {                                       // head column inside the window
            const int64_t pc = prev_col[lo - s0];
            I[pc] = START; Q[pc] = quals[0]; S[pc] = t->is_del[a] ? STRAND_PAD : strand;
        }
        for (int k = 0; k < nb; ++k) {
            const int lg = longest[lo - s0 + k];
            if (lg <= 0) continue;
            const int64_t c0 = col_of[lo - s0 + k] + 1;
            const uint8_t st = t->is_del[a + k] ? STRAND_PAD : strand;
            const int ins = t->indel[a + k];
            if (ins > 0) {
                const int n_ins = std::min(ins, cap[lo - s0 + k]);
                const int q0 = t->qpos[a + k];
                for (int j = 1; j <= n_ins; ++j) {
                    const uint8_t ch = q0 + j < ls ? (uint8_t)t->seq[q0 + j] : (uint8_t)'N';
                    if (!T.known[ch]) return 2;
                    I[c0 + j - 1] = T.token[ch];
                    Q[c0 + j - 1] = quals[k];
                    S[c0 + j - 1] = st;
                }
            }
            for (int j = 0; j < lg; ++j) if (I[c0 + j] == PAD) I[c0 + j] = NOINSERT;
        }
        if (t->end <= stop) {                                       // tail column inside the window
            const int k = nb - 1;
            const int64_t e = col_of[lo - s0 + k] + longest[lo - s0 + k] + 1;
            I[e] = END; Q[e] = quals[k]; S[e] = t->is_del[a + k] ? STRAND_PAD : strand;
        }
        // deletions carry no strand: the row's own strand, forward when it has none (:1063-1078)
        uint8_t best = 0;
        bool any_pad = false;
        for (int c = 0; c < n_cols; ++c) { if (S[c] == STRAND_PAD) any_pad = true; else best = std::max(best, S[c]); }
        if (any_pad) for (int c = 0; c < n_cols; ++c) if (S[c] == STRAND_PAD) S[c] = best ? best : STRAND_UPPER;
    }
    // ---- finish_record (process_locations_chunk :720-838)
    const int64_t center = col_of[ci];
    std::vector<uint8_t> ref_line(n_cols, TOK_GAP);
    for (int p : pos_idx) {
        const int64_t o = p;                                        // s0 + p - ref_start with ref_start = s0
        uint8_t tok = TOK_GAP;                                      // BASE_ENUM[""]
        if (o < (int64_t)ref.size()) {
            const uint8_t ch = (uint8_t)ref[o];
            if (!T.known[ch]) return 2;                              // (the Python path raises the reference's KeyError)
            tok = T.token[ch];
        }
        ref_line[col_of[p]] = tok;
    }
    const int64_t lo = std::max<int64_t>(0, center - w), hi = std::min<int64_t>(center + w + 1, n_cols);
    const int cw = (int)(hi - lo);
    auto first_nonzero_row = [&](const std::vector<uint8_t>& im) {
        for (int r = 0; r < n_rows; ++r) {
            const uint8_t* p = &im[(size_t)r * n_cols + lo];
            for (int c = 0; c < cw; ++c) if (p[c]) return r;
        }
        return 0;                                                    // all rows zero: nothing is trimmed
    };
    const int fb = first_nonzero_row(img), fq = first_nonzero_row(qimg), fs = first_nonzero_row(simg);
    const int nbr = n_rows - fb, nq = n_rows - fq, ns = n_rows - fs;
    const int first = std::max(0, (nbr - MR) / 2);                  // int((n - max_reads) / 2) for n >= max_reads, else 0
    const int last = std::min(first + MR, nbr);
    auto count = [&](int n) { return std::max(0, std::min(last, n) - std::min(first, n)); };
    const int kb = count(nbr), kq = count(nq), ks = count(ns);
    if (kq != kb || ks != kb || kb == 0) return 0;
    const int off = w - (int)(center - lo);
    const int k = std::min(MR, kb);
    memset(reads_out, 0, (size_t)MR * W); memset(qual_out, 0, (size_t)MR * W); memset(strand_out, 0, (size_t)MR * W);
    memset(ref_out, 0, (size_t)W);
    for (int r = 0; r < k; ++r) {
        memcpy(reads_out + (size_t)r * W + off, &img[(size_t)(fb + first + r) * n_cols + lo], cw);
        memcpy(qual_out + (size_t)r * W + off, &qimg[(size_t)(fq + first + r) * n_cols + lo], cw);
        memcpy(strand_out + (size_t)r * W + off, &simg[(size_t)(fs + first + r) * n_cols + lo], cw);
    }
    memcpy(ref_out + off, &ref_line[lo], cw);
    *num_reads = k;
    return 1;
}

int open_encoder(const char* bam_path, const char* bai_path, const char* fasta_path, const pe_options* opt, pe_encoder_t** out) {
    auto e = std::make_unique<pe_encoder>();
    e->bam_path = bam_path; e->fasta_path = fasta_path; e->opt = *opt;
    {   // both files must open (per-thread handles are opened in pe_encode)
        Bam b;
        if (!b.open(bam_path)) return pe_fail(nullptr, "%s", b.err.c_str());
        Fasta f;
        std::string err;
        if (!f.open(fasta_path, err)) return pe_fail(nullptr, "%s", err.c_str());
    }
    std::vector<std::string> cands;
    if (bai_path && *bai_path) cands.push_back(bai_path);
    else {
        cands.push_back(std::string(bam_path) + ".bai");
        const std::string p(bam_path);
        const size_t dot = p.find_last_of('.'), slash = p.find_last_of('/');
        if (dot != std::string::npos && (slash == std::string::npos || dot > slash)) cands.push_back(p.substr(0, dot) + ".bai");
    }
    for (auto& c : cands) if (e->bai.load(c)) { e->have_bai = true; e->bai_path = c; break; }
    *out = e.release();
    return 0;
}

int encode(pe_encoder_t* e, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_out, uint8_t* qual_out,
           uint8_t* strand_out, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out, int32_t threads) {
    const int W = 2 * e->opt.window_size + 1, MR = e->opt.max_reads;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads > 0 ? threads : 1, n));
    std::vector<std::string> errors((size_t)nt);
    std::vector<bamn::frame::Census> census(e->collects() ? (size_t)nt : 0);    // one per thread, added up behind the join
    e->census = bamn::frame::Census{};
    auto work = [&](int ti) {
      try {                                                  // (an exception leaving a std::thread terminates the process)
        const int64_t lo = n * ti / nt, hi = n * (ti + 1) / nt;
        Bam bam;
        Fasta fasta;
        std::string err;
        if (!bam.open(e->bam_path)) { errors[ti] = bam.err; return; }
        if (!fasta.open(e->fasta_path, err)) { errors[ti] = err; return; }
        bam.sample = e->sample;
        bam.filter = e->filter;
        Window win;
        if (e->collects()) win.census = &census[(size_t)ti];
        win.bam = &bam; win.bai = e->have_bai ? &e->bai : nullptr;
        for (int64_t i = lo; i < hi; ++i) {
            const int st = encode_one(e->opt, win, bam, fasta, contigs[i], positions[i], reads_out + (size_t)i * MR * W,
                                      qual_out + (size_t)i * MR * W, strand_out + (size_t)i * MR * W, ref_out + (size_t)i * W,
                                      num_reads_out + i, err);
            if (st < 0) { errors[ti] = err.empty() ? "read error" : err; break; }
            status_out[i] = (int8_t)st;
        }
      } catch (const std::exception& ex) {
        errors[ti] = std::string("pileup encoder: ") + ex.what();
      } catch (...) {
        errors[ti] = "pileup encoder: unknown exception";
      }
    };
    std::vector<std::thread> pool;
    pool.reserve((size_t)nt - 1);
    try {
        for (int ti = 1; ti < nt; ++ti) pool.emplace_back(work, ti);
    } catch (...) {                                          // a thread that did not start: the ones that did still end before this frame
        for (auto& t : pool) t.join();
        throw;
    }
    work(0);
    for (auto& t : pool) t.join();
    for (auto& c : census) e->census.add(c);
    for (auto& s : errors) if (!s.empty()) return pe_fail(e, "%s", s.c_str());
    return 0;
}

}  // namespace

extern "C" {

const char* pe_last_error(const pe_encoder_t* e) { return e ? e->err.c_str() : g_pe_error.c_str(); }

int pe_open(const char* bam_path, const char* bai_path, const char* fasta_path, const pe_options* opt, pe_encoder_t** out) {
    if (!bam_path || !fasta_path || !opt || !out) return pe_fail(nullptr, "pe_open: null argument");
    if (opt->window_size < 1 || opt->max_reads < 1) return pe_fail(nullptr, "pe_open: window_size and max_reads must be positive");
    return capi::guarded(g_pe_error, "pe_open", [&] { return open_encoder(bam_path, bai_path, fasta_path, opt, out); });
}

int pe_encode(pe_encoder_t* e, const char* const* contigs, const int32_t* positions, int64_t n, uint8_t* reads_out, uint8_t* qual_out,
              uint8_t* strand_out, uint8_t* ref_out, int32_t* num_reads_out, int8_t* status_out, int32_t threads) {
    if (!e || (n > 0 && (!contigs || !positions || !reads_out || !qual_out || !strand_out || !ref_out || !num_reads_out || !status_out)))
        return pe_fail(e, "pe_encode: null argument");
    return capi::guarded(e->err, "pe_encode", [&] {
        return encode(e, contigs, positions, n, reads_out, qual_out, strand_out, ref_out, num_reads_out, status_out, threads);
    });
}

int pe_set_subsample(pe_encoder_t* e, double fraction, uint32_t seed) {
    if (!e) return pe_fail(nullptr, "pe_set_subsample: null handle");
    return capi::guarded(e->err, "pe_set_subsample", [&] {
        if (const char* why = bamn::frame::sample_rule(fraction, seed, e->sample)) return pe_fail(e, "pe_set_subsample: %s", why);
        return 0;
    });
}

int pe_subsample_keeps(const uint8_t* name, int32_t l_read_name, double fraction, uint32_t seed) {
    return capi::guarded(g_pe_error, "pe_subsample_keeps", [&] {
        namespace F = bamn::frame;
        if (!name || l_read_name < 1 || l_read_name > 255) return pe_fail(nullptr, "pe_subsample_keeps: a name field of 1..255 bytes");
        F::SampleRule rule{0, 0};
        if (!(fraction > 0.0)) return pe_fail(nullptr, "pe_subsample_keeps: the fraction must lie in (0, 1]");
        if (const char* why = F::sample_rule(fraction, seed, rule)) return pe_fail(nullptr, "pe_subsample_keeps: %s", why);
        // a record of nothing but its fixed fields and the name field, framed by the one core
        std::vector<uint8_t> rec(32 + (size_t)l_read_name, 0);
        rec[8] = (uint8_t)l_read_name;
        memcpy(rec.data() + 32, name, (size_t)l_read_name);
        F::Framed fr;
        if (const uint32_t w = F::frame_record(rec.data(), rec.size(), fr, /*aux=*/false)) return pe_fail(nullptr, "%s", F::why_text(w));
        return F::sampled(rec.data(), fr, rule) ? 1 : 0;
    });
}

int pe_set_read_filter(pe_encoder_t* e, int32_t exclude, int32_t require, int32_t min_mapq) {
    if (!e) return pe_fail(nullptr, "pe_set_read_filter: null handle");
    return capi::guarded(e->err, "pe_set_read_filter", [&] {
        if (const char* why = bamn::frame::read_filter(exclude, require, min_mapq, e->filter)) return pe_fail(e, "pe_set_read_filter: %s", why);
        return 0;
    });
}

int pe_set_read_stats(pe_encoder_t* e, int on) {
    if (!e) return pe_fail(nullptr, "pe_set_read_stats: null handle");
    e->read_stats = on != 0;
    return 0;
}

int pe_get_read_stats(const pe_encoder_t* e, dl4vc_read_stats* out) {
    if (!e || !out) return pe_fail(nullptr, "pe_get_read_stats: null argument");
    static_assert(sizeof(dl4vc_read_stats) == sizeof(e->census.w), "dl4vc_read_stats is the census's words");
    memcpy(out, e->census.w, sizeof(*out));
    return 0;
}

int pe_read_filter_passes(int32_t flag, int32_t mapq, int32_t exclude, int32_t require, int32_t min_mapq) {
    return capi::guarded(g_pe_error, "pe_read_filter_passes", [&] {
        namespace F = bamn::frame;
        if (flag < 0 || flag > 0xffff || mapq < 0 || mapq > 255) return pe_fail(nullptr, "pe_read_filter_passes: a flag in [0, 0xFFFF] and a MAPQ in [0, 255]");
        F::ReadFilter f{0, 0, 0};
        if (const char* why = F::read_filter(exclude, require, min_mapq, f)) return pe_fail(nullptr, "pe_read_filter_passes: %s", why);
        // a record of nothing but its fixed fields and an empty name, framed by the one core
        std::vector<uint8_t> rec(33, 0);
        rec[8] = 1;
        rec[9] = (uint8_t)mapq;
        rec[14] = (uint8_t)(flag & 0xff);
        rec[15] = (uint8_t)(flag >> 8);
        F::Framed fr;
        if (const uint32_t w = F::frame_record(rec.data(), rec.size(), fr, /*aux=*/false)) return pe_fail(nullptr, "%s", F::why_text(w));
        return F::passes(rec.data(), fr, f) ? 1 : 0;
    });
}

void pe_close(pe_encoder_t* e) { delete e; }

}  // extern "C"
