// One definition of how a BAM record is framed (SAM specification section 4.2): the checks of its fixed fields and aux area, why
// a record is refused and the text for it, the CIGAR sums, bam_endpos and one step of the record chain.  Plain C++ that compiles
// for the host and the device and needs no HIP header under a plain compiler: the host paths of the candidate generator
// (cand_capi.cpp) and the pileup encoder (pileup_fetch.h), the CPU twin of the device path and the kernels (bgzf_kernels.hip,
// pileup_frame_kernels.hip) all call it, and tools/asan_bam_frame.sh runs it under sanitizers.  Every length comes from the
// file and is checked before anything is indexed by it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BAMF_HD __host__ __device__
#else
#define BAMF_HD
#endif

namespace bamn {
namespace frame {

constexpr int64_t MAX_NREF = 1 << 29;    // a longer reference span is a corrupt record (no contig is longer)
constexpr uint64_t NO_RECORD = ~0ull;    // a record slot the walk left empty

// Why a record is refused.  The device reports (offset of the record's block_size field) << 8 | Why: the values are fixed.
enum Why : uint32_t {
    W_NONE = 0, W_BLOCK_SIZE, W_TRUNCATED, W_OVER_STOP, W_L_NAME, W_L_SEQ, W_NAME_EXCEEDS, W_CIGAR_EXCEEDS, W_SEQ_EXCEEDS,
    W_AUX_TAG, W_AUX_NUL, W_AUX_ARRAY, W_AUX_ARRAY_TYPE, W_AUX_TYPE, W_AUX_VALUE, W_CIGAR_REF, W_COUNT
};

inline const char* why_text(uint32_t w) {
    static const char* const TEXT[W_COUNT] = {
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
        "corrupt BAM record (CIGAR reference length)",
    };
    return w < W_COUNT ? TEXT[w] : "corrupt BAM record";
}

BAMF_HD inline uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
BAMF_HD inline uint32_t ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
BAMF_HD inline int aux_size(uint8_t type) {
    switch (type) {
        case 'A': case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return -1;
    }
}

struct Framed {
    int32_t tid, pos, l_seq;
    uint32_t n_cig, flag, l_name;
    uint32_t cigar_off, seq_off, qual_off, aux_off;
    int32_t md_off, md_len;        // the first MD:Z value (without its NUL), -1 if absent or the aux area was not walked
    int64_t nref, nquery;          // filled by cigar_sums
    bool has_ref, skip;
};

// The fixed fields of the record b[0, size) and the offsets of its variable parts, each checked to lie inside it; with
// `aux`, the aux area is walked tag by tag as well and the MD:Z value located.
BAMF_HD inline uint32_t frame_record(const uint8_t* b, uint64_t size, Framed& fr, bool aux = true) {
    if (size < 32) return W_BLOCK_SIZE;
    fr.tid = (int32_t)ld32(b);
    fr.pos = (int32_t)ld32(b + 4);
    fr.l_name = b[8];
    fr.n_cig = ld16(b + 12);
    fr.flag = ld16(b + 14);
    fr.l_seq = (int32_t)ld32(b + 16);
    fr.md_off = fr.md_len = -1;
    fr.nref = fr.nquery = 0;
    fr.has_ref = fr.skip = false;
    if (fr.l_name < 1) return W_L_NAME;
    if (fr.l_seq < 0) return W_L_SEQ;
    const uint64_t cig = 32 + (uint64_t)fr.l_name;
    if (cig > size) return W_NAME_EXCEEDS;
    const uint64_t seq = cig + 4 * (uint64_t)fr.n_cig;
    if (seq > size) return W_CIGAR_EXCEEDS;
    const uint64_t qual = seq + ((uint64_t)fr.l_seq + 1) / 2;
    const uint64_t ax = qual + (uint64_t)fr.l_seq;
    if (ax > size) return W_SEQ_EXCEEDS;
    fr.cigar_off = (uint32_t)cig; fr.seq_off = (uint32_t)seq; fr.qual_off = (uint32_t)qual; fr.aux_off = (uint32_t)ax;
    if (!aux) return W_NONE;
    uint64_t o = ax;
    while (o < size) {                                      // (each turn advances o by at least 3)
        if (o + 3 > size) return W_AUX_TAG;
        const bool md = b[o] == 'M' && b[o + 1] == 'D';
        const uint8_t t = b[o + 2];
        o += 3;
        if (t == 'Z' || t == 'H') {
            uint64_t z = o;
            while (z < size && b[z] != 0) ++z;
            if (z >= size) return W_AUX_NUL;
            if (md && t == 'Z' && fr.md_off < 0) { fr.md_off = (int32_t)o; fr.md_len = (int32_t)(z - o); }
            o = z + 1;
        } else if (t == 'B') {
            if (o + 5 > size) return W_AUX_ARRAY;
            const int es = aux_size(b[o]);
            const uint32_t n = ld32(b + o + 1);
            if (es < 0) return W_AUX_ARRAY_TYPE;
            if ((uint64_t)n * (uint64_t)es > size - (o + 5)) return W_AUX_ARRAY;
            o += 5 + (uint64_t)n * (uint64_t)es;
        } else {
            const int vs = aux_size(t);
            if (vs < 0) return W_AUX_TYPE;
            if (o + (uint64_t)vs > size) return W_AUX_VALUE;
            o += (uint64_t)vs;
        }
    }
    return W_NONE;
}

// ---- read subsampling by name hash (samtools view --subsample F --subsample-seed S) ------------------------------------------
// X31 over the read name of a framed record: the bytes behind the fixed fields up to the first NUL, at most l_read_name - 1 of
// them (frame_record has checked that 32 + l_read_name lies inside the record), each widened as a signed char as htslib's
// __ac_X31_hash_string does on x86-64.  An empty name hashes to 0.
BAMF_HD inline uint32_t name_hash(const uint8_t* b, const Framed& fr) {
    const uint8_t* s = b + 32;
    const uint32_t n = fr.l_name - 1;
    if (n == 0 || s[0] == 0) return 0;
    uint32_t h = (uint32_t)(int32_t)(int8_t)s[0];
    for (uint32_t i = 1; i < n && s[i] != 0; ++i) h = h * 31u + (uint32_t)(int32_t)(int8_t)s[i];
    return h;
}

// Wang's integer mix (htslib's __ac_Wang_hash)
BAMF_HD inline uint32_t wang(uint32_t k) {
    k += ~(k << 15);
    k ^= k >> 10;
    k += k << 3;
    k ^= k >> 6;
    k += ~(k << 11);
    k ^= k >> 16;
    return k;
}

// threshold = ceil(F * 2^24) for a fraction F in (0, 1], formed once on the host (sample_threshold); 0 = off, every read kept
struct SampleRule {
    uint32_t seed, threshold;
};

// keep iff (wang(name_hash ^ seed) & 0xffffff) / 2^24 < F; the name is not read when the rule is off
BAMF_HD inline bool sampled(const uint8_t* b, const Framed& fr, const SampleRule& rule) {
    if (rule.threshold == 0) return true;
    return (wang(name_hash(b, fr) ^ rule.seed) & 0xffffffu) < rule.threshold;
}

// ceil(F * 2^24) in double (exact: F * 2^24 only moves the exponent); F is in (0, 1]
inline uint32_t sample_threshold(double fraction) {
    const double v = fraction * 16777216.0;
    uint32_t t = (uint32_t)v;
    if ((double)t < v) ++t;
    return t;
}

// The rule of a setter's arguments: fraction 0 turns it off, a fraction outside [0, 1] or NaN is refused (the reason, else NULL).
inline const char* sample_rule(double fraction, uint32_t seed, SampleRule& out) {
    if (!(fraction >= 0.0 && fraction <= 1.0)) return "the subsample fraction must lie in [0, 1] (0 turns it off)";
    out = SampleRule{seed, fraction > 0.0 ? sample_threshold(fraction) : 0u};
    return nullptr;
}

// ---- read filter by flags and mapping quality (samtools view -F exclude -f require -q min_mapq) -------------------------------
// keep iff (flag & exclude) == 0 && (flag & require) == require && mapq >= min_mapq; all zero = off, every read kept
struct ReadFilter {
    uint16_t exclude, require;
    uint8_t min_mapq;
};

BAMF_HD inline bool filter_on(const ReadFilter& f) { return (f.exclude | f.require | f.min_mapq) != 0; }

// the MAPQ of a framed record: byte 9 of its fixed fields (frame_record has checked that they lie inside the record)
BAMF_HD inline uint32_t mapq_of(const uint8_t* b) { return b[9]; }

enum Verdict : uint32_t { V_KEPT = 0, V_FLAGS, V_MAPQ };    // the flags are tested first: a record counts in one

BAMF_HD inline uint32_t verdict(uint32_t flag, uint32_t mapq, const ReadFilter& f) {
    if ((flag & f.exclude) != 0 || (flag & f.require) != f.require) return V_FLAGS;
    return mapq < f.min_mapq ? V_MAPQ : V_KEPT;
}

// the record is not read when the filter is off
BAMF_HD inline bool passes(const uint8_t* b, const Framed& fr, const ReadFilter& f) {
    if (!filter_on(f)) return true;
    return verdict(fr.flag, mapq_of(b), f) == V_KEPT;
}

// The filter of a setter's arguments, or why not (else NULL).
inline const char* read_filter(int64_t exclude, int64_t require, int64_t min_mapq, ReadFilter& out) {
    if (exclude < 0 || exclude > 0xffff) return "the excluded flags must lie in [0, 0xFFFF]";
    if (require < 0 || require > 0xffff) return "the required flags must lie in [0, 0xFFFF]";
    if (min_mapq < 0 || min_mapq > 255) return "the minimum mapping quality must lie in [0, 255]";
    if (exclude & require) return "a flag bit both excluded and required lets no read pass";
    out = ReadFilter{(uint16_t)exclude, (uint16_t)require, (uint8_t)min_mapq};
    return nullptr;
}

// The read census: the records that passed the region test, counted in front of the filter and the sample rule, once per
// region they belong to.  One layout for the host threads, the device array and the C ABI's struct (include/dl4vc_loader.h).
constexpr int CENSUS_MAPQ = 0, CENSUS_FLAG = 256, CENSUS_SEEN = 272, CENSUS_DROP_FLAGS = 273, CENSUS_DROP_MAPQ = 274,
              CENSUS_KEPT = 275, CENSUS_WORDS = 276;
struct Census {
    uint64_t w[CENSUS_WORDS] = {};
    void add(const Census& o) { for (int i = 0; i < CENSUS_WORDS; ++i) w[i] += o.w[i]; }
};

// One record of these flags and MAPQ into the census, `times` over (the regions it belongs to): v is the filter's verdict on it,
// kept whether it is left behind the sample rule as well.  The one place the host paths count.
inline void census_add(Census& c, uint32_t flag, uint32_t mapq, uint32_t v, bool kept, uint64_t times = 1) {
    c.w[CENSUS_MAPQ + (mapq & 0xff)] += times;
    for (int k = 0; k < 16; ++k)
        if (flag >> k & 1) c.w[CENSUS_FLAG + k] += times;
    c.w[CENSUS_SEEN] += times;
    if (v != V_KEPT) c.w[v == V_FLAGS ? CENSUS_DROP_FLAGS : CENSUS_DROP_MAPQ] += times;
    else if (kept) c.w[CENSUS_KEPT] += times;
}

// What becomes of one record that passed the region test: the filter first, then the sample rule (the name hash of a filtered
// record is not computed).  With `c`, the record is counted in it; the answer is the same without.
enum Fate : uint32_t { FATE_FILTERED = 0, FATE_UNSAMPLED, FATE_KEPT };
inline uint32_t fate(Census* c, const uint8_t* b, const Framed& fr, const ReadFilter& f, const SampleRule& rule, uint64_t times = 1) {
    if (!c && !filter_on(f)) return sampled(b, fr, rule) ? FATE_KEPT : FATE_UNSAMPLED;
    const uint32_t q = mapq_of(b), v = verdict(fr.flag, q, f);
    const bool kept = v == V_KEPT && sampled(b, fr, rule);
    if (c) census_add(*c, fr.flag, q, v, kept, times);
    return v != V_KEPT ? FATE_FILTERED : kept ? FATE_KEPT : FATE_UNSAMPLED;
}

#if defined(__HIPCC__)
// The device side of the census, shared by the two frame kernels: a workgroup counts in s[CENSUS_WORDS] (LDS, uint32: a workgroup
// of 256 threads times a record's memberships stays far below 2^32) and adds what is not zero to the call's array g[CENSUS_WORDS]
// with integer atomics, so the sums are exact whatever the order.  A workgroup that saw nothing flushes nothing.
__device__ inline void census_clear(uint32_t* s) {
    for (uint32_t k = threadIdx.x; k < (uint32_t)CENSUS_WORDS; k += blockDim.x) s[k] = 0;
}
// a record with c > 0 memberships: returns whether the filter keeps it (CENSUS_KEPT is added by the caller, behind the sample rule)
__device__ inline bool census_count(uint32_t* s, const uint8_t* b, const Framed& fr, const ReadFilter& f, uint32_t c) {
    const uint32_t q = mapq_of(b), v = verdict(fr.flag, q, f);
    atomicAdd(&s[CENSUS_MAPQ + q], c);
    for (uint32_t m = fr.flag & 0xffffu; m; m &= m - 1) atomicAdd(&s[CENSUS_FLAG + __ffs((int)m) - 1], c);
    atomicAdd(&s[CENSUS_SEEN], c);
    if (v != V_KEPT) atomicAdd(&s[v == V_FLAGS ? CENSUS_DROP_FLAGS : CENSUS_DROP_MAPQ], c);
    return v == V_KEPT;
}
// (behind a __syncthreads)
__device__ inline void census_flush(const uint32_t* s, unsigned long long* g) {
    if (s[CENSUS_SEEN] == 0) return;
    for (uint32_t k = threadIdx.x; k < (uint32_t)CENSUS_WORDS; k += blockDim.x)
        if (s[k]) atomicAdd(g + k, (unsigned long long)s[k]);
}
#endif

// the reference and query lengths of a framed record's CIGAR, and whether it holds a reference-consuming operation or an N
BAMF_HD inline void cigar_sums(const uint8_t* b, Framed& fr) {
    fr.nref = fr.nquery = 0;
    fr.has_ref = fr.skip = false;
    for (uint32_t i = 0; i < fr.n_cig; ++i) {
        const uint32_t v = ld32(b + fr.cigar_off + 4 * i);
        const int op = v & 0xf;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) { fr.nref += (int64_t)(v >> 4); fr.has_ref = true; }
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) fr.nquery += (int64_t)(v >> 4);
        if (op == 3) fr.skip = true;
    }
}

// The sums, then the pileup encoder's own check: W_CIGAR_REF when the reference span cannot be trusted (it sizes the device's
// resolution arrays).  The candidate generator takes the sums alone: it refuses no record for its span.
BAMF_HD inline uint32_t walk_cigar(const uint8_t* b, Framed& fr) {
    cigar_sums(b, fr);
    if (fr.nref > MAX_NREF || (int64_t)fr.pos + fr.nref > INT32_MAX) return W_CIGAR_REF;
    return W_NONE;
}

// htslib's bam_endpos from the sums: an unmapped read, or one without reference-consuming operations, covers one position
BAMF_HD inline int64_t endpos(const Framed& fr) {
    if (fr.flag & 0x4) return (int64_t)fr.pos + 1;
    return (int64_t)fr.pos + (fr.nref > 0 ? fr.nref : 1);
}

// One step of the record chain in infl[0, total): the record whose block_size field is at `at` must lie before `stop`, the
// next known record boundary (at < stop <= total).  W_NONE with `size`, the bytes behind the field, or why not.
BAMF_HD inline uint32_t next_record(const uint8_t* infl, uint64_t total, uint64_t stop, uint64_t at, uint32_t& size) {
    size = 0;
    if (stop - at < 4) return W_OVER_STOP;
    size = ld32(infl + at);
    if (size < 32 || size > (1u << 28)) return W_BLOCK_SIZE;
    if ((uint64_t)size + 4 > total - at) return W_TRUNCATED;
    if ((uint64_t)size + 4 > stop - at) return W_OVER_STOP;
    return W_NONE;
}

}  // namespace frame
}  // namespace bamn
