// Candidate generation on the GPU (reference tools/candidate_generator.py::build_allele_stats + filter_alleles_by_frequency):
// one thread per framed read walks its CIGAR and MD, adds two coverage difference events per aligned M/=/X run, and emits one
// fixed-width key per allele; the keys are radix sorted and run-length encoded (rocPRIM), the coverage events scanned into
// depth, and each distinct allele kept when min(count, depth) / depth > the minimum frequency (double precision).  Counting
// by sort + run-length encoding is exact and independent of the order the reads run in; the only atomics are integer adds,
// two per aligned run (not per base), and one per survivor.
//
// Per read, the semantics of the reference's detect_variants on pysam's get_aligned_pairs(with_seq=True):
//   * the pairs before the first and after the last reference-consuming operation are trimmed (which drops insertions next to
//     a clip); a soft clip between them reads as an insertion, as its pairs do;
//   * SNP: an MD mismatch letter in ACGT at an aligned base in ACGT;
//   * insertion: a run of query-only pairs, anchored on the pair before it (a deleted position anchors at that position);
//   * deletion: a run of reference-only pairs, REF = anchor + deleted bases, ALT = anchor; a run at the first pair takes the
//     LAST pair as its anchor (Python's aligned_pairs[-1]); a run anchored on an inserted base raises TypeError in the
//     reference, which drops every deletion of that read;
//   * an allele whose REF or ALT is longer than max_len is dropped; only alleles at start <= pos <= end count.
// A read whose MD does not agree with its CIGAR (runs past it, ends short, a '^' run of the wrong length, a letter outside the
// BAM alphabet) is marked malformed and gives no alleles.  Every byte read is bounded by the read's framed length.
// A read without MD gives coverage and no alleles, unless the batch carries the reference bases of its contig (cg_set_reference):
// then the same walk takes them from there (RefSeq below; reference_codes_kernel makes them of the FASTA's bytes).
// With cg_set_left_align an insertion or deletion is moved to its left-most placement on those bases before its key is made
// (cand_left_align.h has the rule): close_run applies it in both passes, so the count pass's offsets hold in the emit pass.
#include "bam_frame.h"
#include "cand_device.h"
#include "cand_left_align.h"
#include "cand_reference.h"
#include "device_buffer.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

#include <vector>

namespace cand {
namespace {

using bamn::frame::ld16;
using bamn::frame::ld32;

// an MD letter as a BAM nibble code ("=ACMGRSVTWYHKDBN"), -1 outside the alphabet (lower case included)
__device__ inline int letter_code(uint8_t c) {
    switch (c) {
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
        case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
        case 'D': return 13; case 'B': return 14; case 'N': return 15; default: return -1;
    }
}
__device__ inline bool is_acgt(int code) { return code == 1 || code == 2 || code == 4 || code == 8; }
__device__ inline bool is_upper(uint8_t c) { return c >= 'A' && c <= 'Z'; }

enum { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };
__device__ inline bool aligned_op(int op) { return op == OP_M || op == OP_EQ || op == OP_X; }

// The MD string as pysam's build_alignment_sequence reads it, held to a strict grammar: matches are decimal counts, a
// mismatch is one upper-case letter, a deletion '^' plus exactly the deleted letters (ended by a digit or the end).
struct Md {
    const uint8_t* p;
    int n, i;
    uint32_t rem;
    bool in_del, bad;

    // the reference base of an aligned pair whose read base is rc
    __device__ int match(int rc, bool& mism) {
        end_del();
        while (rem == 0) {
            if (bad || i >= n) { bad = true; return 0; }
            const uint8_t c = p[i];
            if (c >= '0' && c <= '9') {
                uint32_t v = 0;
                int digits = 0;
                while (i < n && p[i] >= '0' && p[i] <= '9') {
                    v = v * 10 + (p[i] - '0');
                    ++i;
                    if (++digits > 9) { bad = true; return 0; }
                }
                rem = v;
                continue;
            }
            const int code = letter_code(c);
            if (code < 0) { bad = true; return 0; }    // '^' where a base is aligned, or a letter outside the alphabet
            ++i;
            mism = true;
            return code;
        }
        --rem;
        mism = false;
        return rc;
    }
    // the deleted reference base of a reference-only pair
    __device__ int del() {
        if (rem != 0) { bad = true; return 0; }
        if (!in_del) {
            while (i < n && p[i] == '0') ++i;
            if (i >= n || p[i] != '^') { bad = true; return 0; }
            ++i;
            in_del = true;
        }
        const int code = i < n ? letter_code(p[i]) : -1;
        if (code < 0) { bad = true; return 0; }
        ++i;
        return code;
    }
    // a '^' run ends at a pair that is not a deletion: a letter still waiting means the run was longer than the deletion
    __device__ void end_del() {
        if (in_del) {
            if (i < n && is_upper(p[i])) bad = true;
            in_del = false;
        }
    }
    __device__ void finish() {
        end_del();
        while (i < n && p[i] == '0') ++i;
        if (rem != 0 || i != n) bad = true;
    }
};

// The other source of reference bases, for a read without MD (cg_set_reference): the contig's codes at the walk's own
// reference position.  An aligned base is a mismatch when the codes differ or the read's is N (samtools calmd's rule, so the
// letter an MD tag would carry is the code returned here); a position outside the contig makes the read malformed, as an MD
// that runs past its CIGAR does, and no byte outside codes[0, length) is read.
struct RefSeq {
    const uint8_t* codes;
    int64_t length, at;
    bool bad;

    __device__ int next() {
        if ((uint64_t)at >= (uint64_t)length) { bad = true; return 0; }
        return codes[at++];
    }
    __device__ int match(int rc, bool& mism) {
        const int code = next();
        mism = code != rc || rc == 15;
        return code;
    }
    __device__ int del() { return next(); }
    __device__ void end_del() {}
    __device__ void finish() {}
};

struct Sink {
    // count mode (keys == nullptr) or emit mode
    uint64_t* snp;
    IndelKey* indel;
    uint32_t n_snp, n_indel;
    uint32_t la[LA_COUNTERS];   // left-alignment, of the indels counted (LA_* of cand_device.h)
};

struct Pair {
    int kind;      // -1 none, OP_M, OP_D, OP_I
    int32_t pos;
    int code;
};

struct Walk {
    const uint8_t* cig;
    const uint8_t* seq;
    int n_cig, k0, k1;
    int32_t pos, lo, hi;
    uint32_t sub;
    int max_len;
    bool del_dropped;
    const uint8_t* la_codes;   // the contig's codes when indels are left-aligned, else nullptr
    int64_t la_length;

    __device__ int read_code(int q) const { return (q & 1) ? (seq[q >> 1] & 0xf) : (seq[q >> 1] >> 4); }

    // md: the read's reference source at its start (Md or RefSeq), taken by value: each run walks it from the beginning.
    // dry = true: only the walk of the source, returning the last pair (the anchor of a deletion run at the first pair)
    // LA: indels are left-aligned on la_codes before they are counted (a kernel instantiation of its own, so that the walk
    // without the option is the code it was)
    template <bool LA, class Ref>
    __device__ bool run(Ref md, bool dry, Pair last_pair, Sink& out, Pair* last_out) const {
        int32_t rp = pos;
        int qp = 0;
        Pair prev{-1, 0, 0};
        int run_kind = -1, run_len = 0;
        int32_t run_pos = 0;
        uint64_t run_w[4] = {0, 0, 0, 0};
        bool first = true, run_aligned = false;
        auto close_run = [&]() {
            if (run_kind < 0) return;
            bool keep = run_len <= max_len && !(run_kind == OP_D && del_dropped);
            int la_flags = 0;
            int64_t la_k = 0;
            if (LA && keep) {
                la_k = lal::align(run_kind == OP_I ? lal::INS : lal::DEL, run_aligned, run_w, run_len - 1, la_codes, la_length, run_pos,
                                  pos, &la_flags);
                run_pos -= (int32_t)la_k;
            }
            keep = keep && run_pos >= lo && run_pos <= hi;
            if (keep) {
                if (LA) {
                    ++out.la[LA_SEEN];
                    out.la[LA_SHIFTED] += la_k > 0;
                    out.la[LA_BASES] += (uint32_t)la_k;
                    out.la[LA_CLAMPED] += (la_flags & lal::CLAMPED) != 0;
                    out.la[LA_NOT_ELIGIBLE] += !(la_flags & lal::ELIGIBLE);
                }
                if (out.indel) {
                    IndelKey k;
                    k.w[0] = ((uint64_t)sub << 40) | ((uint64_t)(uint32_t)run_pos << 8) |
                             ((uint64_t)(run_kind == OP_I ? KIND_INS : KIND_DEL) << 6) | (uint64_t)run_len;
                    for (int j = 0; j < 4; ++j) k.w[j + 1] = run_w[j];
                    out.indel[out.n_indel] = k;
                }
                ++out.n_indel;
            }
            run_kind = -1;
        };
        auto push_base = [&](int code) {
            if (run_len < KEY_BASES) run_w[run_len >> 4] |= (uint64_t)code << (60 - 4 * (run_len & 15));
            ++run_len;
        };
        auto start_run = [&](int kind, const Pair& anchor, bool stand_in) {
            run_kind = kind;
            run_aligned = anchor.kind == OP_M && !stand_in;
            run_pos = anchor.pos;
            run_len = 0;
            run_w[0] = run_w[1] = run_w[2] = run_w[3] = 0;
            push_base(anchor.code);
        };
        for (int k = 0; k < n_cig; ++k) {
            const uint32_t c = ld32(cig + 4 * k);
            const int op = c & 0xf;
            const int l = (int)(c >> 4);
            const bool q = aligned_op(op) || op == OP_I || op == OP_S;
            if (k < k0 || k > k1) { if (q) qp += l; continue; }
            if (aligned_op(op)) {
                for (int i = 0; i < l; ++i) {
                    if (!dry && run_kind >= 0) close_run();
                    const int rc = read_code(qp + i);
                    bool mism = false;
                    const int code = md.match(rc, mism);
                    if (md.bad) return false;
                    const int32_t p = rp + i;
                    if (!dry && mism && is_acgt(code) && is_acgt(rc) && p >= lo && p <= hi) {
                        if (out.snp) out.snp[out.n_snp] = ((uint64_t)sub << 40) | ((uint64_t)(uint32_t)p << 8) | ((uint64_t)code << 4) | rc;
                        ++out.n_snp;
                    }
                    prev = Pair{OP_M, p, code};
                    first = false;
                }
                rp += l; qp += l;
            } else if (op == OP_D) {
                for (int i = 0; i < l; ++i) {
                    if (!dry && run_kind == OP_I) close_run();
                    const int code = md.del();
                    if (md.bad) return false;
                    if (!dry && run_kind != OP_D) start_run(OP_D, first ? last_pair : prev, first);
                    if (!dry) push_base(code);
                    prev = Pair{OP_D, rp + i, code};
                    first = false;
                }
                rp += l;
            } else if (op == OP_I || op == OP_S) {
                for (int i = 0; i < l; ++i) {
                    md.end_del();
                    if (md.bad) return false;
                    if (!dry && run_kind == OP_D) close_run();
                    if (!dry && run_kind != OP_I) start_run(OP_I, prev, false);
                    if (!dry) push_base(read_code(qp + i));
                    prev = Pair{OP_I, 0, 0};
                }
                qp += l;
            }
            // H: no pairs
        }
        if (!dry) close_run();
        md.finish();
        if (md.bad) return false;
        if (last_out) *last_out = prev;
        return true;
    }

    // the dry run for a deletion run at the first pair, then the run that counts or emits
    template <bool LA, class Ref>
    __device__ bool run_read(const Ref& src, Sink& out) const {
        Pair last{-1, 0, 0};
        Sink dry{nullptr, nullptr, 0, 0, {}};
        if ((ld32(cig + 4 * k0) & 0xf) == OP_D) {
            if (!run<false>(src, true, last, dry, &last)) return false;
        }
        return run<LA>(src, false, last, out, nullptr);
    }
};

// Shared by both passes: frames the read (again, on the device), adds its coverage events (count pass), and walks it.
template <bool EMIT, bool LA>
__device__ void process_read(const uint8_t* __restrict__ buf, const ReadMeta& m, const SubDesc* __restrict__ subs,
                             const RefDesc* __restrict__ refs, int max_len, int* __restrict__ cov, Sink& out, uint8_t& status) {
    const uint8_t* b = buf + m.off;
    const uint32_t len = m.len;
    status = ST_MALFORMED;
    if (len < 32) return;
    const int32_t pos = (int32_t)ld32(b + 4);
    const uint32_t l_name = b[8];
    const int n_cig = (int)ld16(b + 12);
    const int32_t l_seq = (int32_t)ld32(b + 16);
    if (l_seq < 0) return;
    const uint64_t cig_off = 32 + (uint64_t)l_name, seq_off = cig_off + 4 * (uint64_t)n_cig;
    if (seq_off + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > len) return;
    const uint8_t* cig = b + cig_off;
    const SubDesc sd = subs[m.sub];
    // coverage: every fetched read, whatever else is wrong with it (get_reference_positions runs first in the reference)
    if (!EMIT) {
        int32_t rp = pos;
        for (int k = 0; k < n_cig; ++k) {
            const uint32_t c = ld32(cig + 4 * k);
            const int op = c & 0xf;
            const int32_t l = (int32_t)(c >> 4);
            if (aligned_op(op)) {
                const int64_t a = max((int64_t)rp, (int64_t)sd.start), e = min((int64_t)rp + l, (int64_t)sd.end + 1);
                if (a < e) {
                    atomicAdd(cov + sd.cov_base + (a - sd.start), 1);
                    atomicAdd(cov + sd.cov_base + (e - sd.start), -1);
                }
            }
            if (aligned_op(op) || op == OP_D || op == OP_N) rp += l;
        }
    }
    // the reference source: the read's MD when it has one (whatever it says), else the contig's bases when the batch has them
    const bool from_ref = m.md_off < 0;
    if (from_ref && !refs) { status = ST_NO_MD; return; }
    if (!from_ref && (uint64_t)m.md_off + (uint64_t)(m.md_len < 0 ? 0 : m.md_len) > len) return;
    const uint8_t flag = from_ref ? ST_REFERENCE : 0;
    status = ST_MALFORMED | flag;
    int k0 = -1, k1 = -1;
    int64_t qlen = 0;
    bool unsupported = l_seq == 0, bad_op = false, dd = false;
    int prev_kind = -1;
    for (int k = 0; k < n_cig; ++k) {
        const uint32_t c = ld32(cig + 4 * k);
        const int op = c & 0xf;
        if (op > OP_X) bad_op = true;
        if (op == OP_N || op == OP_P) unsupported = true;
        if (aligned_op(op) || op == OP_I || op == OP_S) qlen += c >> 4;
        if ((aligned_op(op) || op == OP_D) && (c >> 4) > 0) { if (k0 < 0) k0 = k; k1 = k; }
    }
    if (bad_op) return;
    if (k0 < 0) { status = ST_NO_PAIRS | flag; return; }
    if (unsupported) { status = ST_UNSUPPORTED | flag; return; }
    if (qlen != l_seq) return;
    for (int k = k0; k <= k1; ++k) {
        const uint32_t c = ld32(cig + 4 * k);
        const int op = c & 0xf;
        if ((c >> 4) == 0) continue;
        if (op == OP_D && prev_kind == OP_I) dd = true;
        if (aligned_op(op)) prev_kind = OP_M;
        else if (op == OP_D) prev_kind = OP_D;
        else if (op == OP_I || op == OP_S) prev_kind = OP_I;
    }
    Walk w;
    w.cig = cig; w.seq = b + seq_off; w.n_cig = n_cig; w.k0 = k0; w.k1 = k1; w.pos = pos;
    w.lo = sd.start; w.hi = sd.end; w.sub = m.sub; w.max_len = max_len; w.del_dropped = dd;
    w.la_codes = nullptr; w.la_length = 0;
    if (LA) {                      // (run_batch launches this instantiation only with refs)
        const RefDesc rd = refs[m.sub];
        w.la_codes = rd.codes; w.la_length = rd.length;
    }
    bool ok;
    if (from_ref) {
        const RefDesc rd = refs[m.sub];
        ok = w.run_read<LA>(RefSeq{rd.codes, rd.length, (int64_t)pos, false}, out);
    } else {
        ok = w.run_read<LA>(Md{b + m.md_off, m.md_len, 0, 0, false, false}, out);
    }
    if (!ok) { out = Sink{out.snp, out.indel, 0, 0, {}}; return; }
    status = (uint8_t)((dd ? ST_OK | ST_DEL_DROPPED : ST_OK) | flag);
}

template <bool LA>
__global__ void count_kernel(const uint8_t* __restrict__ buf, const ReadMeta* __restrict__ meta, uint64_t n,
                             const SubDesc* __restrict__ subs, const RefDesc* __restrict__ refs, int max_len,
                             int* __restrict__ cov, uint32_t* __restrict__ n_snp, uint32_t* __restrict__ n_indel,
                             uint8_t* __restrict__ status, unsigned long long* __restrict__ la_counts) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    Sink s{nullptr, nullptr, 0, 0, {}};
    uint8_t st;
    process_read<false, LA>(buf, meta[r], subs, refs, max_len, cov, s, st);
    n_snp[r] = s.n_snp;
    n_indel[r] = s.n_indel;
    status[r] = st;
    // (integer adds: exact in any order; only reads with a counted indel get here, and only with the option on)
    if (LA && s.la[LA_SEEN])
        for (int j = 0; j < LA_COUNTERS; ++j)
            if (s.la[j]) atomicAdd(la_counts + j, (unsigned long long)s.la[j]);
}

template <bool LA>
__global__ void emit_kernel(const uint8_t* __restrict__ buf, const ReadMeta* __restrict__ meta, uint64_t n,
                            const SubDesc* __restrict__ subs, const RefDesc* __restrict__ refs, int max_len,
                            const uint32_t* __restrict__ snp_off, const uint32_t* __restrict__ indel_off,
                            const uint32_t* __restrict__ n_snp, const uint32_t* __restrict__ n_indel, uint64_t* __restrict__ snp_keys,
                            IndelKey* __restrict__ indel_keys) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || (n_snp[r] == 0 && n_indel[r] == 0)) return;
    Sink s{snp_keys + snp_off[r], indel_keys + indel_off[r], 0, 0, {}};
    uint8_t st;
    process_read<true, LA>(buf, meta[r], subs, refs, max_len, nullptr, s, st);
}

__device__ inline void keep_if(const SubDesc* subs, const int* depth, uint32_t sub, int32_t pos, uint32_t count, bool snp,
                               double snp_min, double indel_min, DevCand& c, bool& keep) {
    const SubDesc sd = subs[sub];
    const int d = depth[sd.cov_base + (pos - sd.start)];
    keep = false;
    if (d <= 0) return;
    const double af = (double)min((int64_t)count, (int64_t)d) / (double)d;
    keep = af > (snp ? snp_min : indel_min);
    c.sub = (int32_t)sub; c.pos = pos; c.depth = d; c.count = (int32_t)count;
}

__global__ void filter_snp_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ n_runs,
                                  const SubDesc* __restrict__ subs, const int* __restrict__ depth, double snp_min,
                                  DevCand* __restrict__ out, uint32_t* __restrict__ n_out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *n_runs) return;
    const uint64_t k = keys[r];
    DevCand c;
    bool keep;
    keep_if(subs, depth, (uint32_t)(k >> 40), (int32_t)(uint32_t)(k >> 8), counts[r], true, snp_min, 0.0, c, keep);
    if (!keep) return;
    c.kind = 0; c.len = 1;
    c.w[0] = (k & 0xff) << 56; c.w[1] = c.w[2] = c.w[3] = 0;
    out[atomicAdd(n_out, 1u)] = c;
}

__global__ void filter_indel_kernel(const IndelKey* __restrict__ keys, const uint32_t* __restrict__ counts,
                                    const uint32_t* __restrict__ n_runs, const SubDesc* __restrict__ subs,
                                    const int* __restrict__ depth, double indel_min, DevCand* __restrict__ out,
                                    uint32_t* __restrict__ n_out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *n_runs) return;
    const IndelKey k = keys[r];
    DevCand c;
    bool keep;
    keep_if(subs, depth, (uint32_t)(k.w[0] >> 40), (int32_t)(uint32_t)(k.w[0] >> 8), counts[r], false, 0.0, indel_min, c, keep);
    if (!keep) return;
    c.kind = (uint32_t)((k.w[0] >> 6) & 3); c.len = (uint32_t)(k.w[0] & 63);
    for (int j = 0; j < 4; ++j) c.w[j] = k.w[j + 1];
    out[atomicAdd(n_out, 1u)] = c;
}

// Reference bases: four bases per lane, one 32-bit store where all four exist (out is a device allocation, p a multiple of 4).
__global__ void reference_codes_kernel(const uint8_t* __restrict__ raw, uint64_t raw_len, int64_t lb, int64_t lw, int64_t length,
                                       uint8_t* __restrict__ out, unsigned long long* __restrict__ counts) {
    const int64_t p0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (p0 >= length) return;
    uint32_t word = 0, other = 0;
    int64_t broken = -1;
    const int n = (int)min((int64_t)4, length - p0);
    for (int j = 0; j < n; ++j) {
        const int c = refc::base_code(raw, raw_len, lb, lw, p0 + j);
        if (c == refc::BROKEN && broken < 0) broken = p0 + j;
        if (c == refc::OTHER) ++other;
        word |= (uint32_t)(c >= refc::OTHER ? 15 : c) << (8 * j);
    }
    if (n == 4) *(uint32_t*)(out + p0) = word;
    else for (int j = 0; j < n; ++j) out[p0 + j] = (uint8_t)(word >> (8 * j));
    if (other) atomicAdd(counts + 0, (unsigned long long)other);
    if (broken >= 0) atomicMin(counts + 1, (unsigned long long)broken);
}

struct IndelDecomposer {
    __host__ __device__ ::rocprim::tuple<uint64_t&, uint64_t&, uint64_t&, uint64_t&, uint64_t&> operator()(IndelKey& k) const {
        return ::rocprim::tuple<uint64_t&, uint64_t&, uint64_t&, uint64_t&, uint64_t&>(k.w[0], k.w[1], k.w[2], k.w[3], k.w[4]);
    }
};

}  // namespace

struct Workspace {
    dev::Buffer recs, meta, subs, refs, cov, depth, n_snp, n_indel, snp_off, indel_off, status, snp_keys, snp_sorted, indel_keys, indel_sorted,
        snp_unique, snp_counts, indel_unique, indel_counts, scalars, la_counts, cands, temp;
    std::vector<uint8_t> h_status;
    std::vector<DevCand> h_cands;
    const uint8_t* recs_p = nullptr;      // the batch's records and their meta: ws->recs / ws->meta after upload(), the
    const ReadMeta* meta_p = nullptr;     // caller's device buffers after upload_device()
    const RefDesc* refs_p = nullptr;      // the batch's reference bases per subregion (ws->refs), nullptr without a reference
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

Workspace* workspace_create() {
    Workspace* ws = new Workspace();
    if (hipEventCreate(&ws->ev0) != hipSuccess || hipEventCreate(&ws->ev1) != hipSuccess) { delete ws; return nullptr; }
    return ws;
}
void workspace_destroy(Workspace* ws) {
    if (!ws) return;
    if (ws->ev0) (void)hipEventDestroy(ws->ev0);
    if (ws->ev1) (void)hipEventDestroy(ws->ev1);
    delete ws;
}

// the batch's subregions, their reference bases (or none) and an empty coverage array
static int upload_subs(Workspace* ws, const SubDesc* subs, const RefDesc* refs, uint32_t n_subs, int64_t cov_len, hipStream_t stream,
                       const char** msg) {
    HIP_CHECK_MSG(ws->subs.ensure((n_subs + 1) * sizeof(SubDesc)));
    HIP_CHECK_MSG(ws->cov.ensure((size_t)(cov_len + 1) * sizeof(int)));
    HIP_CHECK_MSG(hipMemcpyAsync(ws->subs.p, subs, n_subs * sizeof(SubDesc), hipMemcpyHostToDevice, stream));
    HIP_CHECK_MSG(hipMemsetAsync(ws->cov.p, 0, (size_t)cov_len * sizeof(int), stream));
    ws->refs_p = nullptr;
    if (refs) {
        HIP_CHECK_MSG(ws->refs.ensure((n_subs + 1) * sizeof(RefDesc)));
        HIP_CHECK_MSG(hipMemcpyAsync(ws->refs.p, refs, n_subs * sizeof(RefDesc), hipMemcpyHostToDevice, stream));
        ws->refs_p = ws->refs.as<const RefDesc>();
    }
    return 0;
}

int upload(Workspace* ws, const uint8_t* recs, uint64_t rec_bytes, const ReadMeta* meta, uint64_t n_reads, const SubDesc* subs,
           const RefDesc* refs, uint32_t n_subs, int64_t cov_len, hipStream_t stream, const char** msg) {
    HIP_CHECK_MSG(ws->recs.ensure(rec_bytes + 1));
    HIP_CHECK_MSG(ws->meta.ensure((n_reads + 1) * sizeof(ReadMeta)));
    if (rec_bytes) HIP_CHECK_MSG(hipMemcpyAsync(ws->recs.p, recs, rec_bytes, hipMemcpyHostToDevice, stream));
    if (n_reads) HIP_CHECK_MSG(hipMemcpyAsync(ws->meta.p, meta, n_reads * sizeof(ReadMeta), hipMemcpyHostToDevice, stream));
    if (const int rc = upload_subs(ws, subs, refs, n_subs, cov_len, stream, msg)) return rc;
    ws->recs_p = ws->recs.as<const uint8_t>();
    ws->meta_p = ws->meta.as<const ReadMeta>();
    return 0;
}

int upload_device(Workspace* ws, const uint8_t* recs_dev, const ReadMeta* meta_dev, const SubDesc* subs, const RefDesc* refs,
                  uint32_t n_subs, int64_t cov_len, hipStream_t stream, const char** msg) {
    if (const int rc = upload_subs(ws, subs, refs, n_subs, cov_len, stream, msg)) return rc;
    ws->recs_p = recs_dev;
    ws->meta_p = meta_dev;
    return 0;
}

int run_batch(Workspace* ws, uint64_t n_reads, uint32_t n_subs, int64_t cov_len, int max_len, double snp_min, double indel_min,
              bool left_align, hipStream_t stream, const DevCand** out, uint64_t* n_out, const uint8_t** status, uint64_t* n_events,
              uint64_t* n_unique, uint64_t* la_counts, BatchTimes* t, const char** msg) {
    (void)n_subs;
    *n_out = 0; *n_events = 0; *n_unique = 0;
    for (int j = 0; j < LA_COUNTERS; ++j) la_counts[j] = 0;
    if (left_align && !ws->refs_p) { *msg = "left-alignment needs the batch's reference bases"; return -1; }
    ws->h_status.assign(n_reads, 0);
    *status = ws->h_status.data();
    HIP_CHECK_MSG(hipEventRecord(ws->ev0, stream));
    const uint64_t nr1 = n_reads + 1;
    HIP_CHECK_MSG(ws->n_snp.ensure(nr1 * 4));
    HIP_CHECK_MSG(ws->n_indel.ensure(nr1 * 4));
    HIP_CHECK_MSG(ws->snp_off.ensure(nr1 * 4));
    HIP_CHECK_MSG(ws->indel_off.ensure(nr1 * 4));
    HIP_CHECK_MSG(ws->status.ensure(nr1));
    HIP_CHECK_MSG(ws->depth.ensure((size_t)(cov_len + 1) * sizeof(int)));
    HIP_CHECK_MSG(ws->scalars.ensure(16 * sizeof(uint32_t)));
    uint32_t* sc = ws->scalars.as<uint32_t>();     // [0] snp runs, [1] indel runs, [2] survivors
    HIP_CHECK_MSG(hipMemsetAsync(sc, 0, 16 * sizeof(uint32_t), stream));
    HIP_CHECK_MSG(ws->la_counts.ensure(LA_COUNTERS * sizeof(unsigned long long)));
    if (left_align) HIP_CHECK_MSG(hipMemsetAsync(ws->la_counts.p, 0, LA_COUNTERS * sizeof(unsigned long long), stream));
    const int TB = 256;
    const unsigned grid = (unsigned)((n_reads + TB - 1) / TB);
    if (n_reads) {
        hipLaunchKernelGGL(left_align ? count_kernel<true> : count_kernel<false>, dim3(grid), dim3(TB), 0, stream, ws->recs_p, ws->meta_p,
                           n_reads, ws->subs.as<const SubDesc>(), ws->refs_p, max_len, ws->cov.as<int>(),
                           ws->n_snp.as<uint32_t>(), ws->n_indel.as<uint32_t>(), ws->status.as<uint8_t>(),
                           ws->la_counts.as<unsigned long long>());
        HIP_CHECK_MSG(hipGetLastError());
    }
    // per-read output offsets (exclusive scans; the element past the last read carries the total)
    HIP_CHECK_MSG(hipMemsetAsync(ws->n_snp.as<uint32_t>() + n_reads, 0, 4, stream));
    HIP_CHECK_MSG(hipMemsetAsync(ws->n_indel.as<uint32_t>() + n_reads, 0, 4, stream));
    size_t tb = 0, tb2 = 0;
    HIP_CHECK_MSG(rocprim::exclusive_scan(nullptr, tb, ws->n_snp.as<uint32_t>(), ws->snp_off.as<uint32_t>(), 0u, nr1,
                                          rocprim::plus<uint32_t>(), stream));
    HIP_CHECK_MSG(rocprim::inclusive_scan(nullptr, tb2, ws->cov.as<int>(), ws->depth.as<int>(), (size_t)cov_len, rocprim::plus<int>(), stream));
    tb = std::max(tb, tb2);
    HIP_CHECK_MSG(ws->temp.ensure(tb));
    tb = ws->temp.cap;
    HIP_CHECK_MSG(rocprim::exclusive_scan(ws->temp.p, tb, ws->n_snp.as<uint32_t>(), ws->snp_off.as<uint32_t>(), 0u, nr1,
                                          rocprim::plus<uint32_t>(), stream));
    tb = ws->temp.cap;
    HIP_CHECK_MSG(rocprim::exclusive_scan(ws->temp.p, tb, ws->n_indel.as<uint32_t>(), ws->indel_off.as<uint32_t>(), 0u, nr1,
                                          rocprim::plus<uint32_t>(), stream));
    tb = ws->temp.cap;
    if (cov_len > 0)
        HIP_CHECK_MSG(rocprim::inclusive_scan(ws->temp.p, tb, ws->cov.as<int>(), ws->depth.as<int>(), (size_t)cov_len, rocprim::plus<int>(), stream));
    uint32_t tot[2];
    HIP_CHECK_MSG(hipMemcpyAsync(&tot[0], ws->snp_off.as<uint32_t>() + n_reads, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipMemcpyAsync(&tot[1], ws->indel_off.as<uint32_t>() + n_reads, 4, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipStreamSynchronize(stream));
    const uint64_t ns = tot[0], ni = tot[1];
    *n_events = ns + ni;
    HIP_CHECK_MSG(ws->snp_keys.ensure((ns + 1) * 8));
    HIP_CHECK_MSG(ws->snp_sorted.ensure((ns + 1) * 8));
    HIP_CHECK_MSG(ws->snp_unique.ensure((ns + 1) * 8));
    HIP_CHECK_MSG(ws->snp_counts.ensure((ns + 1) * 4));
    HIP_CHECK_MSG(ws->indel_keys.ensure((ni + 1) * sizeof(IndelKey)));
    HIP_CHECK_MSG(ws->indel_sorted.ensure((ni + 1) * sizeof(IndelKey)));
    HIP_CHECK_MSG(ws->indel_unique.ensure((ni + 1) * sizeof(IndelKey)));
    HIP_CHECK_MSG(ws->indel_counts.ensure((ni + 1) * 4));
    HIP_CHECK_MSG(ws->cands.ensure((ns + ni + 1) * sizeof(DevCand)));
    if (ns + ni > 0) {
        hipLaunchKernelGGL(left_align ? emit_kernel<true> : emit_kernel<false>, dim3(grid), dim3(TB), 0, stream, ws->recs_p, ws->meta_p,
                           n_reads, ws->subs.as<const SubDesc>(), ws->refs_p, max_len, ws->snp_off.as<const uint32_t>(),
                           ws->indel_off.as<const uint32_t>(), ws->n_snp.as<const uint32_t>(), ws->n_indel.as<const uint32_t>(),
                           ws->snp_keys.as<uint64_t>(), ws->indel_keys.as<IndelKey>());
        HIP_CHECK_MSG(hipGetLastError());
    }
    if (ns > 0) {
        size_t a = 0, b = 0;
        HIP_CHECK_MSG(rocprim::radix_sort_keys(nullptr, a, ws->snp_keys.as<uint64_t>(), ws->snp_sorted.as<uint64_t>(), (size_t)ns, 0u, 64u, stream));
        HIP_CHECK_MSG(rocprim::run_length_encode(nullptr, b, ws->snp_sorted.as<uint64_t>(), (unsigned)ns, ws->snp_unique.as<uint64_t>(),
                                                 ws->snp_counts.as<uint32_t>(), sc + 0, stream));
        HIP_CHECK_MSG(ws->temp.ensure(std::max(a, b)));
        a = b = ws->temp.cap;
        HIP_CHECK_MSG(rocprim::radix_sort_keys(ws->temp.p, a, ws->snp_keys.as<uint64_t>(), ws->snp_sorted.as<uint64_t>(), (size_t)ns, 0u, 64u, stream));
        HIP_CHECK_MSG(rocprim::run_length_encode(ws->temp.p, b, ws->snp_sorted.as<uint64_t>(), (unsigned)ns, ws->snp_unique.as<uint64_t>(),
                                                 ws->snp_counts.as<uint32_t>(), sc + 0, stream));
        hipLaunchKernelGGL(filter_snp_kernel, dim3((unsigned)((ns + TB - 1) / TB)), dim3(TB), 0, stream, ws->snp_unique.as<const uint64_t>(),
                           ws->snp_counts.as<const uint32_t>(), sc + 0, ws->subs.as<const SubDesc>(), ws->depth.as<const int>(), snp_min,
                           ws->cands.as<DevCand>(), sc + 2);
        HIP_CHECK_MSG(hipGetLastError());
    }
    if (ni > 0) {
        size_t a = 0, b = 0;
        HIP_CHECK_MSG(rocprim::radix_sort_keys(nullptr, a, ws->indel_keys.as<IndelKey>(), ws->indel_sorted.as<IndelKey>(), (size_t)ni,
                                               IndelDecomposer(), stream));
        HIP_CHECK_MSG(rocprim::run_length_encode(nullptr, b, ws->indel_sorted.as<IndelKey>(), (unsigned)ni, ws->indel_unique.as<IndelKey>(),
                                                 ws->indel_counts.as<uint32_t>(), sc + 1, stream));
        HIP_CHECK_MSG(ws->temp.ensure(std::max(a, b)));
        a = b = ws->temp.cap;
        HIP_CHECK_MSG(rocprim::radix_sort_keys(ws->temp.p, a, ws->indel_keys.as<IndelKey>(), ws->indel_sorted.as<IndelKey>(), (size_t)ni,
                                               IndelDecomposer(), stream));
        HIP_CHECK_MSG(rocprim::run_length_encode(ws->temp.p, b, ws->indel_sorted.as<IndelKey>(), (unsigned)ni, ws->indel_unique.as<IndelKey>(),
                                                 ws->indel_counts.as<uint32_t>(), sc + 1, stream));
        hipLaunchKernelGGL(filter_indel_kernel, dim3((unsigned)((ni + TB - 1) / TB)), dim3(TB), 0, stream, ws->indel_unique.as<const IndelKey>(),
                           ws->indel_counts.as<const uint32_t>(), sc + 1, ws->subs.as<const SubDesc>(), ws->depth.as<const int>(), indel_min,
                           ws->cands.as<DevCand>(), sc + 2);
        HIP_CHECK_MSG(hipGetLastError());
    }
    HIP_CHECK_MSG(hipEventRecord(ws->ev1, stream));
    uint32_t hs[3];
    HIP_CHECK_MSG(hipMemcpyAsync(hs, sc, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (n_reads) HIP_CHECK_MSG(hipMemcpyAsync(ws->h_status.data(), ws->status.p, n_reads, hipMemcpyDeviceToHost, stream));
    unsigned long long la[LA_COUNTERS] = {};
    if (left_align) HIP_CHECK_MSG(hipMemcpyAsync(la, ws->la_counts.p, sizeof la, hipMemcpyDeviceToHost, stream));
    HIP_CHECK_MSG(hipStreamSynchronize(stream));
    for (int j = 0; j < LA_COUNTERS; ++j) la_counts[j] = la[j];
    *n_unique = (uint64_t)hs[0] + hs[1];
    ws->h_cands.resize(hs[2]);
    if (hs[2]) {
        HIP_CHECK_MSG(hipMemcpyAsync(ws->h_cands.data(), ws->cands.p, hs[2] * sizeof(DevCand), hipMemcpyDeviceToHost, stream));
        HIP_CHECK_MSG(hipStreamSynchronize(stream));
    }
    *out = ws->h_cands.data();
    *n_out = hs[2];
    float ms = 0.f;
    HIP_CHECK_MSG(hipEventElapsedTime(&ms, ws->ev0, ws->ev1));
    t->device_ms = ms;
    return 0;
}

hipError_t launch_reference_codes(const uint8_t* raw_dev, uint64_t raw_len, int64_t lb, int64_t lw, int64_t length, uint8_t* out_dev,
                                  unsigned long long* counts_dev, hipStream_t stream) {
    if (length <= 0) return hipSuccess;
    const int TB = 256;
    const int64_t lanes = (length + 3) / 4;
    hipLaunchKernelGGL(reference_codes_kernel, dim3((unsigned)((lanes + TB - 1) / TB)), dim3(TB), 0, stream, raw_dev, raw_len, lb, lw, length,
                       out_dev, counts_dev);
    return hipGetLastError();
}

}  // namespace cand
