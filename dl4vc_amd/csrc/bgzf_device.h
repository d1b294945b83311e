// Device side of the BGZF path (bgzf_kernels.hip) as its hosts see it (bgzf_capi.cpp, cand_capi.cpp, pileup_capi.cpp): inflate a
// run of BGZF blocks into one contiguous buffer, walk the BAM record chain in it, frame the records and hand them to the candidate
// kernels as cand::ReadMeta without leaving the device.  InflateStage is the host side of the inflate for both BAM paths.
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "bam_frame.h"
#include "bgzf_inflate.h"
#include "bgzf_plan.h"
#include "cand_device.h"
#include "device_buffer.h"

namespace bz {

struct SubRange {
    int32_t tid, start, end;
};

constexpr uint64_t NO_ERROR = ~0ull;   // else (offset of the record's block_size field) << 8 | bamn::frame::Why, the lowest offset wins

// inflates n blocks of comp (device) into out (device); status[i] per block.  Blocks whose desc.status is set are skipped.
hipError_t launch_inflate(const uint8_t* comp, const BlockDesc* tab, int64_t n, uint8_t* out, int32_t* status, hipStream_t stream);

// The inflate of --inflate-device gpu: the file, the blocks of a plan as they are in pinned memory, their copy on the device and
// the inflated bytes.  read, upload, then enqueue / finish once per plan that lies in what was read (BlockPlan::adopt); the caller
// sets the device, times its upload its own way and does its own host work between enqueue and finish.  Every step: 0, or a code
// with its text in err.
struct InflateStage {
    int fd = -1;
    dev::Pinned h_comp;
    dev::Buffer d_comp, d_infl;
    dev::Array<BlockDesc> d_tab;
    dev::Array<int32_t> d_bstatus;
    dev::Event ev[2];
    std::vector<int32_t> bstatus;

    bool open(const std::string& path) { return fd >= 0 || (fd = ::open(path.c_str(), O_RDONLY)) >= 0; }
    // plan's spans, read from the file
    int read(BlockPlan& plan, const std::string& path, std::string& err) {
        struct stat sb;
        std::string perr;
        if (fstat(fd, &sb) != 0) return capi::failf(err, -3, "BGZF: cannot stat %s", path.c_str());
        if (!plan.spans((uint64_t)sb.st_size, perr)) return capi::failf(err, -3, "%s", perr.c_str());
        if (h_comp.ensure(plan.comp_bytes + 4)) return capi::failf(err, -2, "pinned allocation of %llu bytes failed", (unsigned long long)plan.comp_bytes);
        if (!plan.read(fd, path, h_comp.p, perr)) return capi::failf(err, -3, "%s", perr.c_str());
        return 0;
    }
    // (begin, if given, is recorded once the buffer is there, in front of the copy: the caller's upload time)
    int upload(const BlockPlan& plan, hipStream_t s, std::string& err, hipEvent_t begin = nullptr) {
        if (d_comp.ensure((size_t)plan.comp_bytes + 16))
            return capi::failf(err, -2, "hipMalloc failed for %llu compressed bytes", (unsigned long long)plan.comp_bytes);
        if (begin) DEV_TRY(err, "device inflate: ", hipEventRecord(begin, s));
        if (plan.comp_bytes) DEV_TRY(err, "device inflate: ", hipMemcpyAsync(d_comp.p, h_comp.p, plan.comp_bytes, hipMemcpyHostToDevice, s));
        return 0;
    }
    int enqueue(const BlockPlan& plan, hipStream_t s, std::string& err) {
        const size_t nblk = plan.tab.size();
        if (d_tab.ensure(nblk + 1) || d_infl.ensure((size_t)plan.infl_bytes + 16) || d_bstatus.ensure(nblk + 1))
            return capi::failf(err, -2, "hipMalloc failed for %llu inflated bytes", (unsigned long long)plan.infl_bytes);
        for (dev::Event& e : ev) DEV_TRY(err, "device inflate: ", e.ensure());
        if (nblk) DEV_TRY(err, "device inflate: ", hipMemcpyAsync(d_tab.p, plan.tab.data(), nblk * sizeof(BlockDesc), hipMemcpyHostToDevice, s));
        DEV_TRY(err, "device inflate: ", hipEventRecord(ev[0], s));
        DEV_TRY(err, "device inflate: ", launch_inflate(d_comp.p, d_tab.p, (int64_t)nblk, d_infl.p, d_bstatus.p, s));
        DEV_TRY(err, "device inflate: ", hipEventRecord(ev[1], s));
        bstatus.resize(nblk);
        if (nblk) DEV_TRY(err, "device inflate: ", hipMemcpyAsync(bstatus.data(), d_bstatus.p, nblk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        return 0;
    }
    // waits for the stream; *inflate_ms += the kernel's time; the first block that is not BZ_OK is the error
    int finish(const BlockPlan& plan, hipStream_t s, double* inflate_ms, std::string& err) {
        DEV_TRY(err, "device inflate: ", hipStreamSynchronize(s));
        float ms = 0.f;
        DEV_TRY(err, "device inflate: ", hipEventElapsedTime(&ms, ev[0], ev[1]));
        *inflate_ms += ms;
        for (size_t i = 0; i < bstatus.size(); ++i)
            if (bstatus[i] != BZ_OK) return capi::failf(err, -3, "%s", plan.bad_block(i, bstatus[i]).c_str());
        return 0;
    }
    InflateStage() = default;
    InflateStage(const InflateStage&) = delete;
    InflateStage& operator=(const InflateStage&) = delete;
    ~InflateStage() { if (fd >= 0) close(fd); }
};

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
// = records walked; *err = NO_ERROR or the first refused record.  0 or -2 with msg.  With a sample rule (threshold != 0) a record
// it drops is listed nowhere; *n_seen (if given) = the entries in front of the rule (= *n_reads without one).  A record the read
// filter drops is listed nowhere either, in front of the rule; with a filter, or with `census` (the entries in front of the filter
// are added to it), the frame kernel counts in LDS and flushes with integer atomics; with neither it runs as without the option.
int frame_records(Framer* f, const uint8_t* infl, uint64_t infl_bytes, const Segment* segs, uint64_t n_segs, uint64_t n_slots,
                  const SubRange* subs /* host */, uint32_t n_subs, hipStream_t stream,
                  const cand::ReadMeta** meta, uint64_t* n_reads, uint64_t* n_records, uint64_t* err, const char** msg,
                  bamn::frame::SampleRule rule = bamn::frame::SampleRule{0, 0}, uint64_t* n_seen = nullptr,
                  bamn::frame::ReadFilter filter = bamn::frame::ReadFilter{0, 0, 0}, bamn::frame::Census* census = nullptr);

}  // namespace bz
