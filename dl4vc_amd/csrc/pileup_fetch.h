// The records of one run of locations, framed on the host (libdl4vc_pileup.so without pg_set_inflate_device), and the CPU twin of
// the device path: the index ranges and block table of bgzf_plan.h, the decode core of bgzf_inflate.h and the frame core of
// bam_frame.h, run serially.  No device call: tools/asan_pileup_frame.sh builds this under sanitizers.
#pragma once

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "bam_native.h"
#include "bgzf_plan.h"
#include "pileup_frame.h"

namespace pgh {

// what pg_last_error(NULL) returns: the error of the last failed pg_open or pg_debug_run_records (defined in pileup_debug.cpp)
extern std::string g_err __attribute__((visibility("hidden")));

struct RunRecs {
    std::vector<uint8_t> bytes;
    std::vector<pg::Rec> recs;   // off relative to bytes, res relative to the run
    int64_t max_nref = 0;
    int64_t nres = 0;
    bool sorted = true;
    std::string err;
    int64_t seen = 0;            // records that passed the region test and the read filter, in front of the sample rule
};

struct Region { int32_t tid; int64_t start, end; };

inline std::string at_voff(const char* why, int64_t voff) {
    return std::string(why) + " (record at virtual offset " + std::to_string(voff) + ")";
}

// a kept record joins the run
inline void append(RunRecs& run, const pg::frame::Framed& fr, uint64_t off, int32_t& last_pos) {
    if (fr.pos < last_pos) run.sorted = false;
    last_pos = fr.pos;
    pg::Rec m;
    pg::frame::fill_rec(fr, off, run.nres, m);
    run.nres += fr.nref;
    run.max_nref = std::max(run.max_nref, fr.nref);
    run.recs.push_back(m);
}

// The records of one run: tid == run's, pos < stop and pos + max(nref, 1) > s0 (the window reader of dan_pileup.cpp), read
// forward from the linear index's offset for s0.  A record the sample rule drops (bam_frame.h) is framed and checked like every
// other and then joins no run; so is a record the read filter drops, in front of the rule.  `census` (the calling thread's own, may
// be null): every record that passed the region test is counted in it, in front of the filter.
inline void fetch_records(const bamn::Bai& bai, bamn::BamFile& bam, std::vector<uint8_t>& blk, int32_t tid, int64_t s0, int64_t stop,
                          RunRecs& run, pg::frame::SampleRule rule = pg::frame::SampleRule{0, 0},
                          pg::frame::ReadFilter filter = pg::frame::ReadFilter{0, 0, 0}, pg::frame::Census* census = nullptr) {
    namespace F = pg::frame;
    const uint64_t at = bai.linear_offset(tid, s0);
    if (at == 0) return;
    if (!bam.r.seek((int64_t)at)) { run.err = "BGZF: " + bam.r.err; return; }
    int32_t last_pos = -1;
    for (;;) {
        const int64_t voff = bam.r.tell();
        const int got = bam.next_block(blk);
        if (got == 0) return;
        if (got < 0) { run.err = at_voff(bam.err.c_str(), voff); return; }
        F::Framed fr;
        if (const uint32_t why = F::frame_record(blk.data(), blk.size(), fr)) { run.err = at_voff(F::why_text(why), voff); return; }
        if (fr.tid != tid) {
            if (fr.tid < 0 || fr.tid > tid) return;
            continue;
        }
        if (fr.pos >= stop) return;
        if (const uint32_t why = F::walk_cigar(blk.data(), fr)) { run.err = at_voff(F::why_text(why), voff); return; }
        if (!F::keeps(fr, tid, s0, stop)) continue;
        const uint32_t fate = F::fate(census, blk.data(), fr, filter, rule);
        if (fate == F::FATE_FILTERED) continue;
        ++run.seen;
        if (fate != F::FATE_KEPT) continue;
        append(run, fr, run.bytes.size(), last_pos);
        run.bytes.insert(run.bytes.end(), blk.begin(), blk.end());
        run.bytes.resize((run.bytes.size() + 3) & ~(size_t)3);
    }
}

// The same records the way the device path finds them, on the CPU: the BAI bins' byte ranges, every touched block inflated by
// the decode core into one buffer (run.bytes; Rec::off points into it), the record chain walked segment by segment, and each
// record framed and kept by the shared core.
// `others` (n_others of them): further regions of the same call.  With any, the blocks are read once for the call's plan over
// all the regions and the run's own plan takes them from it (BlockPlan::adopt), as a group of runs does in the encoder.
inline void twin_records(const bamn::Bai& bai, const std::string& path, int32_t tid, int64_t s0, int64_t stop, RunRecs& run,
                         const Region* others = nullptr, int64_t n_others = 0, pg::frame::SampleRule rule = pg::frame::SampleRule{0, 0}) {
    namespace F = pg::frame;
    const Region rg{tid, s0, stop};
    bz::BlockPlan pl, all;
    pl.plan(bai, &rg, 1);
    if (pl.ranges.empty()) return;
    std::vector<Region> call(others, others + n_others);
    call.push_back(rg);
    std::sort(call.begin(), call.end(), [](const Region& a, const Region& b) { return a.tid != b.tid ? a.tid < b.tid : a.start < b.start; });
    if (n_others > 0) all.plan(bai, call.data(), (int64_t)call.size());
    bz::BlockPlan& rd = n_others > 0 ? all : pl;            // the plan whose spans are read from the file
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) { run.err = "cannot open " + path; return; }
    struct stat sb;
    std::vector<uint8_t> comp;
    bool ok = fstat(fd, &sb) == 0 && rd.spans((uint64_t)sb.st_size, run.err);
    if (ok) {
        comp.resize(rd.comp_bytes + 1);
        ok = rd.read(fd, path, comp.data(), run.err) && (n_others == 0 || pl.adopt(all, run.err)) && pl.segments(run.err);
    }
    close(fd);
    if (!ok) { if (run.err.empty()) run.err = "BGZF: cannot stat " + path; return; }
    run.bytes.assign(pl.infl_bytes + 1, 0);
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = bz::crc_table_entry(i);
    std::vector<bz::Tables> t(1);
    for (size_t i = 0; i < pl.tab.size(); ++i) {
        const int st = bz::inflate_block_host(comp.data(), pl.tab[i], run.bytes.data(), t[0], table);
        if (st != BZ_OK) { run.err = pl.bad_block(i, st); return; }
    }
    const uint8_t* infl = run.bytes.data();
    const uint64_t total = pl.infl_bytes;
    int32_t last_pos = -1;
    for (const bz::Segment& sg : pl.segs) {                 // (bam_walk_kernel's checks, then the frame kernel's, record by record)
        uint64_t at = sg.start;
        while (at < sg.stop) {
            uint32_t size = 0;
            uint32_t why = F::next_record(infl, total, sg.stop, at, size);
            F::Framed fr;
            if (!why) why = F::frame_record(infl + at + 4, size, fr);
            if (!why && fr.tid == tid) why = F::walk_cigar(infl + at + 4, fr);
            if (why) { run.err = at_voff(F::why_text(why), pl.voff_of(at)); return; }
            if (F::keeps(fr, tid, s0, stop)) {
                ++run.seen;
                if (F::sampled(infl + at + 4, fr, rule)) append(run, fr, at + 4, last_pos);
            }
            at += (uint64_t)size + 4;
        }
    }
}

}  // namespace pgh
