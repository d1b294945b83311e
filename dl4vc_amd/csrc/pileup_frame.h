// One definition of a framed record of the GPU pileup encoder: the checks of bamn::frame_record, the CIGAR walk, the rule that
// keeps a record for a run and the fields of pg::Rec.  Plain C++ that compiles for the host and the device: fetch_records()
// (pileup_fetch.h, the host path), its CPU twin and pileup_frame_kernels.hip all call it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PGF_HD __host__ __device__
#else
#define PGF_HD
#endif

namespace pg {

enum : uint32_t { R_FLAG_OK = 1, R_HAS_REF = 2, R_SKIP = 4, R_REVERSE = 8, R_EQ = 16, R_SHORT_SEQ = 32 };

// One framed record of a batch (the framing fills all but hash and R_EQ, which the resolve kernel adds;
// R_SHORT_SEQ: SEQ holds fewer bases than the CIGAR's query length, e.g. SEQ '*').
struct Rec {
    uint64_t off;          // first byte of the record (after block_size) in the batch buffer
    uint64_t hash;         // FNV-1a 64 of name ':' sequence, never 0
    int32_t pos, end;      // end = pos + reference-consuming length (nref)
    int32_t res;           // first of the record's nref entries in the resolution arrays
    int32_t l_seq;
    uint32_t cigar_off, seq_off, qual_off;
    uint32_t n_cig, l_name;
    uint32_t bits;
};

namespace frame {

constexpr uint32_t FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400;   // unmapped, secondary, QC fail, duplicate (dan_pileup.cpp)
constexpr uint32_t FREVERSE = 0x10;
constexpr int64_t MAX_NREF = 1 << 29;                         // a longer reference span is a corrupt record (no contig is longer)

// Why a record is refused: the values and order of bz::Reason (bgzf_device.h), then the CIGAR's own.
enum Why : uint32_t {
    W_NONE = 0, W_BLOCK_SIZE, W_TRUNCATED, W_OVER_STOP, W_L_NAME, W_L_SEQ, W_NAME_EXCEEDS, W_CIGAR_EXCEEDS, W_SEQ_EXCEEDS,
    W_AUX_TAG, W_AUX_NUL, W_AUX_ARRAY, W_AUX_ARRAY_TYPE, W_AUX_TYPE, W_AUX_VALUE, W_CIGAR_REF, W_COUNT
};

// the texts of bamn::frame_record, BamFile::next_block and walk_cigar
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

PGF_HD inline uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
PGF_HD inline uint32_t ld32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
PGF_HD inline int aux_size(uint8_t type) {
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
    int64_t nref, nquery;          // filled by walk_cigar
    bool has_ref, skip;
};

// The fixed fields of the record b[0, size) and the offsets of its variable parts, each checked to lie inside it; with
// `aux`, the aux area is walked tag by tag as well (bamn::frame_record's checks, in its order).
PGF_HD inline uint32_t frame_record(const uint8_t* b, uint64_t size, Framed& fr, bool aux = true) {
    if (size < 32) return W_BLOCK_SIZE;
    fr.tid = (int32_t)ld32(b);
    fr.pos = (int32_t)ld32(b + 4);
    fr.l_name = b[8];
    fr.n_cig = ld16(b + 12);
    fr.flag = ld16(b + 14);
    fr.l_seq = (int32_t)ld32(b + 16);
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
        const uint8_t t = b[o + 2];
        o += 3;
        if (t == 'Z' || t == 'H') {
            uint64_t z = o;
            while (z < size && b[z] != 0) ++z;
            if (z >= size) return W_AUX_NUL;
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

// The record's reference and query lengths; W_CIGAR_REF when its reference span cannot be trusted (it sizes the device's
// resolution arrays).
PGF_HD inline uint32_t walk_cigar(const uint8_t* b, Framed& fr) {
    fr.nref = fr.nquery = 0;
    fr.has_ref = fr.skip = false;
    for (uint32_t i = 0; i < fr.n_cig; ++i) {
        const uint32_t v = ld32(b + fr.cigar_off + 4 * i);
        const int op = v & 0xf;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) { fr.nref += (int64_t)(v >> 4); fr.has_ref = true; }
        if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) fr.nquery += (int64_t)(v >> 4);
        if (op == 3) fr.skip = true;
    }
    if (fr.nref > MAX_NREF || (int64_t)fr.pos + fr.nref > INT32_MAX) return W_CIGAR_REF;
    return W_NONE;
}

// the window reader's rule (dan_pileup.cpp): a record of the run's contig that starts before stop and reaches past s0
PGF_HD inline bool keeps(const Framed& fr, int32_t tid, int64_t s0, int64_t stop) {
    return fr.tid == tid && (int64_t)fr.pos < stop && (int64_t)fr.pos + (fr.nref > 1 ? fr.nref : 1) > s0;
}

// every field of the Rec but hash; res: the records' nref before this one (a batch past INT32_MAX positions is refused later)
PGF_HD inline void fill_rec(const Framed& fr, uint64_t off, int64_t res, Rec& m) {
    m.off = off;
    m.hash = 0;
    m.pos = fr.pos;
    m.end = (int32_t)(fr.pos + fr.nref);
    m.res = (int32_t)(res < INT32_MAX ? res : INT32_MAX);
    m.l_seq = fr.l_seq;
    m.cigar_off = fr.cigar_off; m.seq_off = fr.seq_off; m.qual_off = fr.qual_off;
    m.n_cig = fr.n_cig; m.l_name = fr.l_name;
    m.bits = ((fr.flag & FLAG_MASK) ? 0u : (uint32_t)R_FLAG_OK) | (fr.has_ref ? (uint32_t)R_HAS_REF : 0u) | (fr.skip ? (uint32_t)R_SKIP : 0u) |
             ((fr.flag & FREVERSE) ? (uint32_t)R_REVERSE : 0u) | (fr.nquery > (int64_t)fr.l_seq ? (uint32_t)R_SHORT_SEQ : 0u);
}

}  // namespace frame
}  // namespace pg
