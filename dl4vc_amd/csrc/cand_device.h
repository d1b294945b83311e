// Types shared by the candidate generator's kernels (cand_kernels.hip) and its host side (cand_capi.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cand {

// one framed record of one subregion: its bytes are buf[off, off + len) (the bytes behind block_size)
struct ReadMeta {
    uint64_t off;
    uint32_t len;
    uint32_t sub;        // subregion index within the batch
    int32_t md_off;      // MD:Z value within the record, -1 when absent
    int32_t md_len;
};

struct SubDesc {
    int32_t start, end;  // fetch [start, end), alleles at start <= pos <= end
    int64_t cov_base;    // first element of this subregion's coverage slot (end - start + 2 ints)
};

// the reference bases under one subregion (cg_set_reference): its contig's codes, one BAM nibble code per base, resident on the
// device; a batch with a reference carries one per subregion, beside SubDesc
struct RefDesc {
    const uint8_t* codes;
    int64_t length;
};

// per-read status (the low bits) and flags
enum : uint8_t { ST_OK = 0, ST_NO_MD = 1, ST_NO_PAIRS = 2, ST_UNSUPPORTED = 3, ST_MALFORMED = 4 };
constexpr uint8_t ST_DEL_DROPPED = 0x10;
constexpr uint8_t ST_REFERENCE = 0x20;   // a read without MD, taken against the reference bases

// Allele keys.  SNP: sub(24) | pos(32) | ref(4) | alt(4).  Indel: w[0] = sub(24) | pos(32) | kind(2) | len(6), then the bases
// (anchor first: ALT of an insertion, REF of a deletion) as BAM nibble codes, 16 per word from the top.
constexpr int KIND_INS = 1, KIND_DEL = 2;
constexpr int KEY_BASES = 64;
struct IndelKey {
    uint64_t w[5];
};
__host__ __device__ inline bool operator==(const IndelKey& a, const IndelKey& b) {
    return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3] && a.w[4] == b.w[4];
}
__host__ __device__ inline bool operator!=(const IndelKey& a, const IndelKey& b) { return !(a == b); }

struct DevCand {
    int32_t sub, pos, depth, count;
    uint32_t kind, len;  // kind 0 = SNP (w[0] top byte = ref << 4 | alt)
    uint64_t w[4];
};

// left-alignment (cg_set_left_align): what run_batch counts over the indel observations that were counted as alleles
enum { LA_SEEN = 0, LA_SHIFTED, LA_BASES, LA_CLAMPED, LA_NOT_ELIGIBLE, LA_COUNTERS };

struct Workspace;     // device buffers, grown on demand (cand_kernels.hip)

struct BatchTimes {
    float device_ms;
};

Workspace* workspace_create();
void workspace_destroy(Workspace* ws);
// Runs one batch whose framed records are already on the device (ws buffers from upload()).  Returns 0 or a negative code
// with msg set.  out / n_out: survivors in a host array owned by the workspace; status: one byte per read, host.
// refs: one RefDesc per subregion (reads without MD are walked against them), or nullptr (such reads are ST_NO_MD).
// left_align (needs refs): insertions and deletions are moved to their left-most placement on those bases before they are
// counted (cand_left_align.h); la_counts[LA_COUNTERS] receives the batch's counters (zero with the option off).
int upload(Workspace* ws, const uint8_t* recs, uint64_t rec_bytes, const ReadMeta* meta, uint64_t n_reads,
           const SubDesc* subs, const RefDesc* refs, uint32_t n_subs, int64_t cov_len, hipStream_t stream, const char** msg);
// The same for records and meta that are already on the device (the BGZF path, bgzf_device.h): they are used in place and must
// stay valid until run_batch() returns.
int upload_device(Workspace* ws, const uint8_t* recs_dev, const ReadMeta* meta_dev, const SubDesc* subs, const RefDesc* refs,
                  uint32_t n_subs, int64_t cov_len, hipStream_t stream, const char** msg);
int run_batch(Workspace* ws, uint64_t n_reads, uint32_t n_subs, int64_t cov_len, int max_len, double snp_min, double indel_min,
              bool left_align, hipStream_t stream, const DevCand** out, uint64_t* n_out, const uint8_t** status, uint64_t* n_events,
              uint64_t* n_unique, uint64_t* la_counts, BatchTimes* t, const char** msg);

// Reference bases (cand_reference.h has the rule): raw_dev[0, raw_len) -> out_dev[0, length), on the stream.  counts_dev[0]
// gains the bytes outside the alphabet, counts_dev[1] takes the minimum with the first base that is a line end, '>' or past
// raw_len (the caller sets them to 0 and refc::NONE first).  Needs refc::layout_ok(lb, lw, length).
hipError_t launch_reference_codes(const uint8_t* raw_dev, uint64_t raw_len, int64_t lb, int64_t lw, int64_t length, uint8_t* out_dev,
                                  unsigned long long* counts_dev, hipStream_t stream);

}  // namespace cand
