// Shared between the host side (pileup_capi.cpp) and the kernels (pileup_kernels.hip) of libdl4vc_pileup.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pg {

constexpr int BLOCK = 256;                   // threads per location workgroup (four wave64)
constexpr int MAX_TRACKS = 1024;             // PG_MAX_TRACKS
constexpr int MAX_WINDOW = 100;              // PG_MAX_WINDOW
constexpr int MAX_POS = 2 * MAX_WINDOW + 5;  // reference positions of one location's fetch window [s0, stop)
constexpr int HASH_SLOTS = 2 * MAX_TRACKS;   // LDS open-addressing table of name:sequence hashes
constexpr uint8_t REF_UNKNOWN = 0xff;        // a reference base outside the token table

enum : uint32_t { R_FLAG_OK = 1, R_HAS_REF = 2, R_SKIP = 4, R_REVERSE = 8, R_EQ = 16, R_SHORT_SEQ = 32 };

// One framed record of a batch (the host fills all but hash and R_EQ, which the resolve kernel adds;
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

// One location of a batch.
struct Loc {
    int32_t s0, stop, ci;  // fetch window [s0, stop) and the 0-based offset of the candidate position in it
    int32_t first, last;   // candidate records [first, last) of the batch
    int32_t pre;           // -1: encode; 0 or 2: status decided on the host
    int64_t ref;           // index of position s0 in the batch's reference token array
    int64_t slot;          // plane slot the location writes (every slot is written, zeros unless status 1)
};

struct Params {
    int32_t w, W, max_reads, max_insert_length, max_insert_length_variant;
};

hipError_t launch_resolve(const uint8_t* buf, Rec* recs, int32_t n_recs, int32_t* qpos, int32_t* indel, uint8_t* isdel,
                          hipStream_t s);
hipError_t launch_encode(const uint8_t* buf, const Rec* recs, const Loc* locs, int32_t n_locs, const uint8_t* reftok,
                         const int32_t* qpos, const int32_t* indel, const uint8_t* isdel, Params p, uint8_t* reads,
                         uint8_t* qual, uint8_t* strand, uint8_t* ref_small, int32_t* num_small, int8_t* status_small,
                         hipStream_t s);

// ---- site assembly (assemble_kernels.hip) ----
constexpr int ASSEMBLE_BLOCK = 256;          // threads per (site, plane) workgroup

// Where one output site comes from.
struct SiteSrc {
    int32_t slot;          // location slot of the stored planes
    int32_t first_rows;    // != 0: stored rows 0..R-1, one contiguous span; 0: the site's R entries of `rows`
};

struct AssembleArgs {
    const uint8_t* src[3];  // stored reads / qual / strand [n][S][L]
    uint8_t* dst[3];        // assembled reads / qual / strand [m][R][L]
    const SiteSrc* sites;   // [m], device
    const int16_t* rows;    // [m][R], device; read only where first_rows == 0
    int32_t S, R, L;
    int32_t use[3];         // 0: the plane is zero-filled (a model without q-scores / strands)
};

hipError_t launch_assemble(const AssembleArgs& a, int32_t m, hipStream_t s);

}  // namespace pg
