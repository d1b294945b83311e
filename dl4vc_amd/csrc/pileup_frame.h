// The pileup encoder's own part of a framed record: the rule that keeps a record for a run and the fields of pg::Rec.  The
// framing itself (the checks, the reasons, the CIGAR walk) is the shared core of bam_frame.h, which pg::frame takes in whole:
// fetch_records() (pileup_fetch.h, the host path), its CPU twin and pileup_frame_kernels.hip call both through one name.
#pragma once

#include "bam_frame.h"

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

using namespace bamn::frame;

constexpr uint32_t FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400;   // unmapped, secondary, QC fail, duplicate (dan_pileup.cpp)
constexpr uint32_t FREVERSE = 0x10;

// the window reader's rule (dan_pileup.cpp): a record of the run's contig that starts before stop and reaches past s0
BAMF_HD inline bool keeps(const Framed& fr, int32_t tid, int64_t s0, int64_t stop) {
    return fr.tid == tid && (int64_t)fr.pos < stop && (int64_t)fr.pos + (fr.nref > 1 ? fr.nref : 1) > s0;
}

// every field of the Rec but hash; res: the records' nref before this one (a batch past INT32_MAX positions is refused later)
BAMF_HD inline void fill_rec(const Framed& fr, uint64_t off, int64_t res, Rec& m) {
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
