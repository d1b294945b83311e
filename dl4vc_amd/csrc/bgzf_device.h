// Device side of the BGZF path (bgzf_kernels.hip) as its hosts see it (bgzf_capi.cpp, cand_capi.cpp): inflate a run of BGZF
// blocks into one contiguous buffer, walk the BAM record chain in it, frame the records and hand them to the candidate
// kernels as cand::ReadMeta without leaving the device.
#pragma once

#include "bam_frame.h"
#include "bgzf_inflate.h"
#include "bgzf_plan.h"
#include "cand_device.h"

namespace bz {

struct SubRange {
    int32_t tid, start, end;
};

constexpr uint64_t NO_ERROR = ~0ull;   // else (offset of the record's block_size field) << 8 | bamn::frame::Why, the lowest offset wins

// inflates n blocks of comp (device) into out (device); status[i] per block.  Blocks whose desc.status is set are skipped.
hipError_t launch_inflate(const uint8_t* comp, const BlockDesc* tab, int64_t n, uint8_t* out, int32_t* status, hipStream_t stream);

struct Framer;   // device buffers of the walk / frame / emit passes, grown on demand
Framer* framer_create();
void framer_destroy(Framer* f);
using bamn::frame::NO_RECORD;           // a record slot the walk left empty
// Walks segs (bgzf_plan.h) over infl[0, infl_bytes): *rec_off (device, owned by the framer, n_slots entries) holds the offset of
// every record's block_size field, NO_RECORD in the slots left over; *n_records = records walked; *err = NO_ERROR or the first
// refused record.  0 or -2 with msg.  The first pass of frame_records(), and of the pileup encoder's framing.
int walk_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs /* host */, uint64_t n_segs, uint64_t n_slots,
                 hipStream_t stream, const uint64_t** rec_off, uint64_t* n_records, uint64_t* err, const char** msg);
// Walks segs over infl[0, infl_bytes), frames every record and lists it once for each subregion it overlaps (same tid,
// pos < end, endpos > start).  *meta (device, owned by the framer) then holds *n_reads entries with off into infl; *n_records
// = records walked; *err = NO_ERROR or the first refused record.  0 or -2 with msg.
int frame_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs, uint64_t n_segs, uint64_t n_slots,
                  const SubRange* subs /* host */, uint32_t n_subs, hipStream_t stream,
                  const cand::ReadMeta** meta, uint64_t* n_reads, uint64_t* n_records, uint64_t* err, const char** msg);

}  // namespace bz
