// Shared between the host side (pileup_capi.cpp) and the kernels (pileup_kernels.hip) of libdl4vc_pileup.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pileup_frame.h"

namespace pg {

constexpr int BLOCK = 256;                   // threads per location workgroup (four wave64)
constexpr int MAX_TRACKS = 1024;             // PG_MAX_TRACKS
constexpr int MAX_WINDOW = 100;              // PG_MAX_WINDOW
constexpr int MAX_POS = 2 * MAX_WINDOW + 5;  // reference positions of one location's fetch window [s0, stop)
constexpr int HASH_SLOTS = 2 * MAX_TRACKS;   // LDS open-addressing table of name:sequence hashes
constexpr uint8_t REF_UNKNOWN = 0xff;        // a reference base outside the token table

// (pg::Rec, one framed record of a batch, and its bits: pileup_frame.h)

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
// The statuses launch_encode would leave in status_small, and nothing else (census_locations).
hipError_t launch_census(const uint8_t* buf, const Rec* recs, const Loc* locs, int32_t n_locs, const uint8_t* reftok,
                         const int32_t* qpos, const int32_t* indel, const uint8_t* isdel, Params p, int8_t* status_small,
                         hipStream_t s);

// ---- framing on the device (pileup_frame_kernels.hip; pg_set_inflate_device) ----
// One run of locations, in the order of the call: sorted by (tid, s0), and stop rises with s0 inside a contig.
struct RunDesc {
    int32_t tid, pad;
    int64_t s0, stop;
};
// What the framing found for a run: its records [rec0, rec1) of the group, its longest reference span, positions never decreasing.
struct RunOut {
    int32_t rec0, rec1;
    int64_t max_nref;
    int32_t sorted, pad;
};
constexpr uint64_t FRAME_NO_ERROR = ~0ull;   // else (offset of the record's block_size field) << 8 | frame::Why, the lowest offset wins

struct Framing;   // device buffers of the framing passes, grown on demand
Framing* framing_create();
void framing_destroy(Framing* f);
// rec_off: the n_slots record slots bz::walk_records left over infl (device).  Frames every record, lists it once for each of
// the n_runs runs (host) it belongs to, run-major and in file order inside a run: *recs (device, the framing's own, *n_recs
// entries with off into infl and res from the exclusive scan of their reference lengths, *n_res in all) and *run_out (device).
// *err = FRAME_NO_ERROR or the first refused record.  0 or -2 with msg.  With a sample rule (threshold != 0) a record it drops
// is listed in no run; *n_seen (if given) = the entries in front of the rule (= *n_recs without one).  A record the read filter
// drops is listed in no run either, in front of the rule; with a filter, or with `census` (the entries in front of the filter are
// added to it), the frame kernel counts in LDS and flushes with integer atomics.
int frame_runs(Framing* f, const uint8_t* infl, const uint64_t* rec_off, uint64_t n_slots, const RunDesc* runs, int32_t n_runs,
               hipStream_t stream, Rec** recs, int64_t* n_recs, int64_t* n_res, const RunOut** run_out, uint64_t* err, const char** msg,
               frame::SampleRule rule = frame::SampleRule{0, 0}, int64_t* n_seen = nullptr,
               frame::ReadFilter filter = frame::ReadFilter{0, 0, 0}, frame::Census* census = nullptr);
// Fills first / last (or pre = 2 in a run that is not sorted) of the device locations whose pre is -1; loc_run (host): each
// location's run, -1 for none.  `uploaded` (may be null) is recorded between the copy of loc_run and the kernel.
int locate(Framing* f, const Rec* recs, const RunOut* run_out, int32_t n_runs, const int32_t* loc_run, Loc* locs, int32_t n_locs,
           hipStream_t stream, const char** msg, hipEvent_t uploaded = nullptr);

// ---- site assembly (assemble_kernels.hip) ----
constexpr int ASSEMBLE_BLOCK = 256;          // threads per (site, plane) workgroup

// Where one output site comes from.
struct SiteSrc {
    int32_t slot;          // location slot of the stored planes
    int32_t first_rows;    // != 0: stored rows 0..R-1, one contiguous span; 0: the site's R entries of `rows`
};

struct AssembleArgs {
    const uint8_t* src[3];  // stored reads / qual / strand: slot i's [S][L] plane at src[plane] + i * slot_stride
    uint8_t* dst[3];        // assembled reads / qual / strand [m][R][L]
    const SiteSrc* sites;   // [m], device
    const int16_t* rows;    // [m][R], device; read only where first_rows == 0
    int64_t slot_stride;    // bytes; S * L for planes [n][S][L], the record size for planes inside records
    int32_t S, R, L;
    int32_t use[3];         // 0: the plane is zero-filled (a model without q-scores / strands)
};

hipError_t launch_assemble(const AssembleArgs& a, int32_t m, hipStream_t s);

constexpr int COUNTS_BLOCK = 64;             // one wave per site
constexpr int COUNT_TOKENS = 16;             // tokens 0..15 are counted, larger bytes are not

// counts[site][k][t] = rows of reads[site] ([R][L]) whose byte at column col + k is t (k = 0, 1; t < COUNT_TOKENS).  The caller
// has checked 0 <= col, col + 1 < L and 0 < m <= INT32_MAX.
hipError_t launch_center_counts(const uint8_t* reads, int64_t m, int32_t R, int32_t L, int32_t col, int32_t* counts, hipStream_t s);

}  // namespace pg
