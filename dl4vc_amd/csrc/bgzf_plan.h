// Host planning of the device BGZF path, shared by its hosts (cand_capi.cpp, pileup_capi.cpp and the CPU twin of
// pileup_fetch.h): from a list of regions to the byte ranges the BAI bins give, the BGZF blocks those ranges touch (read as they
// are), the block table of the inflate and the segments of the record walk.  Plain C++: no device call, so the same text runs
// under a sanitizer.
#pragma once

#include <unistd.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "bam_native.h"
#include "bgzf_inflate.h"

namespace bz {

typedef bamn::Bai::Chunk Chunk;

// a stretch of the inflated buffer whose two ends are known record boundaries; slot_base: first of its bytes / 36 + 1 slots
struct Segment {
    uint64_t start, stop, slot_base;
};

struct HostBlock {
    uint64_t coff;       // file offset of the block
    uint64_t out_off;
    uint32_t isize;
};

struct BlockPlan {
    std::vector<Chunk> ranges;                  // merged, sorted (virtual offsets)
    std::vector<std::vector<uint64_t>> bounds;  // per range: walk boundaries inside it (virtual offsets), ends included
    std::vector<uint64_t> span_at, span_lo, span_hi;   // per range: where its file span [lo, hi) lies in the compressed buffer
    uint64_t comp_bytes = 0, infl_bytes = 0, n_slots = 0;
    std::vector<BlockDesc> tab;                 // body_off relative to the compressed buffer
    std::vector<HostBlock> blocks;              // in out_off order
    std::vector<size_t> first_block;            // per range, one past the end included
    std::vector<Segment> segs;

    // The byte ranges of regions [0, n) (the union of the chunks of every overlapping bin, merged) and where a walk may start
    // inside them: every chunk begin and every distinct linear-index offset of the regions' windows.  R has tid, start, end.
    template <class R>
    void plan(const bamn::Bai& bai, const R* regions, int64_t n) {
        std::vector<Chunk> chunks;
        std::vector<uint64_t> starts;
        for (int64_t i = 0; i < n; ++i) {
            const R& rg = regions[i];
            const size_t before = chunks.size();
            bai.region_chunks(rg.tid, rg.start, rg.end, chunks);
            if (chunks.size() == before) continue;
            const auto& lin = bai.linear[rg.tid];
            for (int64_t w = (int64_t)rg.start >> 14; w <= ((int64_t)rg.end - 1) >> 14 && w < (int64_t)lin.size(); ++w)
                if (lin[w]) starts.push_back(lin[w]);
        }
        for (const Chunk& c : chunks) starts.push_back(c.first);
        std::sort(starts.begin(), starts.end());
        starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
        ranges = chunks;
        bamn::Bai::merge_chunks(ranges);
        bounds.assign(ranges.size(), {});
        for (size_t r = 0; r < ranges.size(); ++r) {
            std::vector<uint64_t>& b = bounds[r];
            b.push_back(ranges[r].first);
            for (auto it = std::upper_bound(starts.begin(), starts.end(), ranges[r].first); it != starts.end() && *it < ranges[r].second; ++it)
                b.push_back(*it);
            b.push_back(ranges[r].second);
        }
    }

    // The file spans: from the block a range begins in to the end of the block it ends in (read 64 KiB past that block's start,
    // which holds it whole).  false with err when the index points past the file.
    bool spans(uint64_t file_size, std::string& err) {
        const size_t n = ranges.size();
        span_at.assign(n + 1, 0); span_lo.assign(n, 0); span_hi.assign(n, 0);
        for (size_t r = 0; r < n; ++r) {
            const uint64_t cb = ranges[r].first >> 16, ce = ranges[r].second >> 16, ue = ranges[r].second & 0xffff;
            if (cb >= file_size || ce > file_size || (ue > 0 && ce >= file_size)) {
                err = "BGZF: truncated file (the index points at offset " + std::to_string(std::max(cb, ce)) + ", past its end at " +
                      std::to_string(file_size) + ")";
                return false;
            }
            span_lo[r] = cb;
            span_hi[r] = ue > 0 ? std::min<uint64_t>(file_size, ce + 65536) : ce;
            span_at[r + 1] = span_at[r] + (span_hi[r] - span_lo[r]);
        }
        comp_bytes = span_at[n];
        return true;
    }

    // Reads the spans into buf (comp_bytes of room) and parses the blocks of every range: the block table, slot after slot in
    // the inflated buffer.
    bool read(int fd, const std::string& path, uint8_t* buf, std::string& err) {
        const size_t n = ranges.size();
        tab.clear(); blocks.clear();
        first_block.assign(n + 1, 0);
        infl_bytes = 0;
        for (size_t r = 0; r < n; ++r) {
            uint64_t got = 0;
            const uint64_t want = span_hi[r] - span_lo[r];
            while (got < want) {
                const ssize_t g = pread(fd, buf + span_at[r] + got, want - got, (off_t)(span_lo[r] + got));
                if (g <= 0) {
                    err = "BGZF: cannot read " + path + " at offset " + std::to_string(span_lo[r] + got);
                    return false;
                }
                got += (uint64_t)g;
            }
            const uint64_t ce = ranges[r].second >> 16, ue = ranges[r].second & 0xffff;
            uint64_t c = span_lo[r];
            first_block[r] = blocks.size();
            while (c < ce || (c == ce && ue > 0)) {
                BlockDesc d;
                uint32_t bsize = 0;
                if (parse_block(buf, span_at[r + 1], span_at[r] + (c - span_lo[r]), d, &bsize) != BZ_OK) {
                    err = "BGZF: not a BGZF block, or a truncated BGZF block (block at file offset " + std::to_string(c) + ")";
                    return false;
                }
                d.out_off = infl_bytes;
                tab.push_back(d);
                blocks.push_back(HostBlock{c, infl_bytes, d.isize});
                infl_bytes += d.isize;
                c += bsize;
            }
        }
        first_block[n] = blocks.size();
        return true;
    }

    // Instead of read(): the blocks of this plan's ranges out of `all`, a plan already read whose ranges cover these (its
    // compressed buffer is the one the table refers to); the slots are this plan's own.  `all` lists a block once for every
    // range of its own that touches it, so a range's blocks are looked up only among those of the one range of `all` that
    // contains it: there they are unique and in file order.
    bool adopt(const BlockPlan& all, std::string& err) {
        const size_t n = ranges.size();
        tab.clear(); blocks.clear();
        first_block.assign(n + 1, 0);
        infl_bytes = 0;
        for (size_t r = 0; r < n; ++r) {
            const uint64_t cb = ranges[r].first >> 16, ce = ranges[r].second >> 16, ue = ranges[r].second & 0xffff;
            first_block[r] = blocks.size();
            // the range of `all` that contains this one: the last that begins at or before it
            const size_t ar = (size_t)(std::upper_bound(all.ranges.begin(), all.ranges.end(), ranges[r].first,
                                                        [](uint64_t v, const Chunk& c) { return v < c.first; }) - all.ranges.begin());
            if (ar == 0 || all.ranges[ar - 1].second < ranges[r].second) {
                err = "BGZF: the index range at offset " + std::to_string(ranges[r].first) + " lies outside the ranges that were read";
                return false;
            }
            const size_t lo = all.first_block[ar - 1], hi = all.first_block[ar];
            size_t k = (size_t)(std::lower_bound(all.blocks.begin() + lo, all.blocks.begin() + hi, cb,
                                                 [](const HostBlock& b, uint64_t c) { return b.coff < c; }) - all.blocks.begin());
            if (k >= hi || all.blocks[k].coff != cb) {
                err = "BGZF: the index offset " + std::to_string(ranges[r].first) + " does not point at a block that was read";
                return false;
            }
            for (; k < hi && (all.blocks[k].coff < ce || (all.blocks[k].coff == ce && ue > 0)); ++k) {
                BlockDesc d = all.tab[k];
                d.out_off = infl_bytes;
                tab.push_back(d);
                blocks.push_back(HostBlock{all.blocks[k].coff, infl_bytes, d.isize});
                infl_bytes += d.isize;
            }
        }
        first_block[n] = blocks.size();
        return true;
    }

    // virtual offset -> offset in the inflated buffer, within range r's run of blocks
    bool locate(size_t r, uint64_t voff, uint64_t& at) const {
        const uint64_t coff = voff >> 16, u = voff & 0xffff;
        const auto lo = blocks.begin() + first_block[r], hi = blocks.begin() + first_block[r + 1];
        const auto it = std::lower_bound(lo, hi, coff, [](const HostBlock& b, uint64_t c) { return b.coff < c; });
        if (it != hi && it->coff == coff) {
            if (u > it->isize) return false;
            at = it->out_off + u;
            return true;
        }
        if (it == hi && u == 0 && lo != hi) {                 // the offset just past the run's last block
            at = (hi - 1)->out_off + (hi - 1)->isize;
            return true;
        }
        return false;
    }

    // The walk segments between the boundaries of every range, and the record slots they need.
    bool segments(std::string& err) {
        segs.clear();
        n_slots = 0;
        for (size_t r = 0; r < ranges.size(); ++r) {
            std::vector<uint64_t> at;
            for (const uint64_t v : bounds[r]) {
                uint64_t a;
                if (!locate(r, v, a)) {
                    err = "BGZF: the index offset " + std::to_string(v) + " does not point into a block of its chunk";
                    return false;
                }
                at.push_back(a);
            }
            const uint64_t lo = at.front(), hi = at.back();
            std::sort(at.begin(), at.end());
            at.erase(std::unique(at.begin(), at.end()), at.end());
            for (size_t k = 0; k + 1 < at.size(); ++k) {
                if (at[k] < lo || at[k + 1] > hi) continue;
                segs.push_back(Segment{at[k], at[k + 1], n_slots});
                n_slots += (at[k + 1] - at[k]) / 36 + 1;
            }
        }
        return true;
    }

    // offset in the inflated buffer -> virtual offset (blocks of no bytes share an out_off: the last block at or before off holds it)
    int64_t voff_of(uint64_t off) const {
        auto it = std::upper_bound(blocks.begin(), blocks.end(), off, [](uint64_t o, const HostBlock& b) { return o < b.out_off; });
        const HostBlock& b = *(it == blocks.begin() ? it : it - 1);
        return (int64_t)((b.coff << 16) | std::min<uint64_t>(off - b.out_off, 0xffff));
    }

    // what every path says of block i of tab when its inflate ends with a status other than BZ_OK
    std::string bad_block(size_t i, int status) const {
        return std::string(bamn::BAD_BLOCK) + " (" + bz_status_text(status) + ", block at file offset " +
               std::to_string(blocks[i].coff) + ")";
    }
};

}  // namespace bz
