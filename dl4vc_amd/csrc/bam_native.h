// BGZF blocks, the BAM header / record framing and the BAI linear index (SAM specification sections 4.1, 4.2 and 5.2), shared
// by the pileup encoder (dan_pileup.cpp, libdl4vc_loader.so) and the candidate generator (cand_capi.cpp, libdl4vc_cand.so).
// Every length below comes from the file and is checked before anything is sized or indexed by it; errors are reported in
// ``err`` strings, never by aborting.
#pragma once

#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "bam_frame.h"

namespace bamn {

// ---- BGZF -------------------------------------------------------------------------------------------------------------------------
constexpr const char* BAD_BLOCK = "BGZF block fails its CRC / size check";   // the host reader's refusal; the device path adds the status

struct Bgzf {
    FILE* f = nullptr;                                           // owned: closed with the reader (also when an exception unwinds past it)
    Bgzf() = default;
    Bgzf(const Bgzf&) = delete;
    Bgzf& operator=(const Bgzf&) = delete;
    ~Bgzf() { if (f) fclose(f); }
    int64_t block_start = 0, next_block = 0;
    std::vector<uint8_t> data, raw;
    size_t off = 0;
    std::string err;

    bool load(int64_t file_off) {
        if (fseeko(f, file_off, SEEK_SET) != 0) { err = "seek failed"; return false; }
        uint8_t head[18];
        const size_t got = fread(head, 1, 18, f);
        if (got == 0) { block_start = next_block = file_off; data.clear(); off = 0; return false; }
        if (got < 18 || head[0] != 0x1f || head[1] != 0x8b || head[2] != 8 || head[3] != 4) { err = "not a BGZF block"; return false; }
        const int xlen = head[10] | (head[11] << 8);
        std::vector<uint8_t> extra(xlen);
        memcpy(extra.data(), head + 12, std::min(6, xlen));
        if (xlen > 6 && fread(extra.data() + 6, 1, xlen - 6, f) != (size_t)(xlen - 6)) { err = "truncated BGZF header"; return false; }
        int bsize = -1;
        for (int i = 0; i + 4 <= xlen;) {
            const int slen = extra[i + 2] | (extra[i + 3] << 8);
            if (extra[i] == 'B' && extra[i + 1] == 'C' && i + 6 <= xlen) bsize = extra[i + 4] | (extra[i + 5] << 8);
            i += 4 + slen;
        }
        if (bsize < 0) { err = "BGZF block without a BC field"; return false; }
        const int body = bsize + 1 - 12 - xlen;
        if (body < 8) { err = "truncated BGZF block"; return false; }
        raw.resize(body);
        if (fread(raw.data(), 1, body, f) != (size_t)body) { err = "truncated BGZF block"; return false; }
        uint32_t crc, isize;
        memcpy(&crc, raw.data() + body - 8, 4);
        memcpy(&isize, raw.data() + body - 4, 4);
        if (isize > 65536) { err = "BGZF block claims more than 64 KiB of data"; return false; }   // (the format's limit; not a size to trust)
        data.resize(isize);
        uint8_t scratch[8];
        z_stream zs{};
        if (inflateInit2(&zs, -15) != Z_OK) { err = "inflateInit2 failed"; return false; }
        zs.next_in = raw.data(); zs.avail_in = body - 8;
        zs.next_out = isize ? data.data() : scratch; zs.avail_out = isize ? isize : (unsigned)sizeof scratch;   // (the empty end-of-file block)
        const int rc = inflate(&zs, Z_FINISH);
        const bool ok = rc == Z_STREAM_END && zs.total_out == isize;
        inflateEnd(&zs);
        if (!ok || (uint32_t)crc32(0L, isize ? data.data() : scratch, isize) != crc) { err = BAD_BLOCK; return false; }
        block_start = file_off; next_block = file_off + bsize + 1; off = 0;
        return true;
    }
    int64_t tell() const { return (block_start << 16) | (int64_t)off; }
    bool seek(int64_t voff) {
        const int64_t blk = voff >> 16;
        if (blk != block_start || data.empty()) { err.clear(); load(blk); if (!err.empty()) return false; }
        off = (size_t)(voff & 0xffff);
        return true;
    }
    // reads up to n bytes; returns the count (short at end of file); err set on a corrupt block
    size_t read(void* dst, size_t n) {
        size_t done = 0;
        while (n > 0) {
            if (off >= data.size()) {
                err.clear();
                if (!load(next_block)) { if (!err.empty()) return done; break; }
                continue;
            }
            const size_t take = std::min(n, data.size() - off);
            memcpy((uint8_t*)dst + done, data.data() + off, take);
            off += take; done += take; n -= take;
        }
        return done;
    }
};

// ---- BAM header and record chain (a record itself is framed by bam_frame.h) -------------------------------------------------------
struct BamFile {
    Bgzf r;
    std::vector<std::string> refs;
    std::vector<int64_t> lengths;
    std::map<std::string, int> tid_of;
    int64_t first_record = 0;
    std::string err;

    bool open(const std::string& path) {
        r.f = fopen(path.c_str(), "rb");
        if (!r.f) { err = "cannot open " + path; return false; }
        char magic[4];
        if (r.read(magic, 4) != 4 || memcmp(magic, "BAM\1", 4) != 0) { err = path + " is not a BAM file"; return false; }
        int32_t l_text = 0, n_ref = 0;
        if (r.read(&l_text, 4) != 4) { err = "truncated BAM header"; return false; }
        if (l_text < 0 || l_text > (1 << 30)) { err = "corrupt BAM header (text length)"; return false; }
        std::vector<char> text((size_t)l_text);
        if (r.read(text.data(), text.size()) != text.size() || r.read(&n_ref, 4) != 4) { err = "truncated BAM header"; return false; }
        if (n_ref < 0) { err = "corrupt BAM header (reference count)"; return false; }
        for (int i = 0; i < n_ref; ++i) {
            int32_t ln = 0, len = 0;
            if (r.read(&ln, 4) != 4) { err = "truncated BAM header"; return false; }
            if (ln < 1 || ln > 65536) { err = "corrupt BAM header (reference name length)"; return false; }
            std::vector<char> nm((size_t)ln);
            if (r.read(nm.data(), nm.size()) != nm.size() || r.read(&len, 4) != 4) { err = "truncated BAM header"; return false; }
            refs.emplace_back(nm.data(), ln > 0 ? (size_t)ln - 1 : 0);
            lengths.push_back(len);
            tid_of[refs.back()] = i;
        }
        first_record = r.tell();
        return true;
    }
    // the bytes behind the next record's block_size into b; 0 = end of file, 1 = ok, -1 = error (err set)
    int next_block(std::vector<uint8_t>& b) {
        int32_t size = 0;
        const size_t g = r.read(&size, 4);
        if (g < 4) { if (!r.err.empty()) err = r.err; return r.err.empty() ? 0 : -1; }
        if (size < 32 || size > (1 << 28)) { err = frame::why_text(frame::W_BLOCK_SIZE); return -1; }
        b.resize((size_t)size);
        if (r.read(b.data(), b.size()) != b.size()) { err = r.err.empty() ? frame::why_text(frame::W_TRUNCATED) : r.err; return -1; }
        return 1;
    }
};

// ---- BAI: the linear index, and the chunks of every bin ------------------------------------------------------------------------
struct Bai {
    std::vector<std::vector<uint64_t>> linear;
    typedef std::pair<uint64_t, uint64_t> Chunk;                 // [begin, end) as virtual offsets
    std::vector<std::map<uint32_t, std::vector<Chunk>>> bins;    // per reference: bin -> chunks (the pseudo-bin 37450 left out)
    // false when the file is absent, not a BAI or shorter than its own counts say
    bool load(const std::string& path) {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return false;
        std::vector<uint8_t> raw;
        uint8_t buf[65536];
        size_t g;
        while ((g = fread(buf, 1, sizeof buf, f)) > 0) raw.insert(raw.end(), buf, buf + g);
        fclose(f);
        if (raw.size() < 8 || memcmp(raw.data(), "BAI\1", 4) != 0) return false;
        size_t o = 4;
        auto take32 = [&](int32_t& v) { if (o + 4 > raw.size()) return false; memcpy(&v, &raw[o], 4); o += 4; return true; };
        int32_t n_ref;
        if (!take32(n_ref) || n_ref < 0) return false;
        for (int r = 0; r < n_ref; ++r) {
            int32_t n_bin;
            if (!take32(n_bin) || n_bin < 0) return false;
            bins.emplace_back();
            for (int b = 0; b < n_bin; ++b) {
                int32_t bin, n_chunk;
                if (!take32(bin) || !take32(n_chunk) || n_chunk < 0) return false;
                if ((uint64_t)16 * (uint64_t)n_chunk > raw.size() - o) return false;
                if ((uint32_t)bin != 37450u) {
                    std::vector<Chunk>& ch = bins.back()[(uint32_t)bin];
                    for (int32_t c = 0; c < n_chunk; ++c) {
                        Chunk k;
                        memcpy(&k.first, &raw[o + 16 * (size_t)c], 8);
                        memcpy(&k.second, &raw[o + 16 * (size_t)c + 8], 8);
                        ch.push_back(k);
                    }
                }
                o += 16 * (size_t)n_chunk;
            }
            int32_t n_intv;
            if (!take32(n_intv) || n_intv < 0) return false;
            if ((uint64_t)8 * (uint64_t)n_intv > raw.size() - o) return false;
            std::vector<uint64_t> lin((size_t)n_intv);
            if (n_intv > 0) memcpy(lin.data(), &raw[o], 8 * (size_t)n_intv);
            o += 8 * (size_t)n_intv;
            linear.push_back(std::move(lin));
        }
        return true;
    }
    // 0 = "no alignment at or after the window" (BaiIndex.linear_offset returning None)
    uint64_t linear_offset(int tid, int64_t start) const {
        if (tid < 0 || tid >= (int)linear.size()) return 0;
        const auto& lin = linear[tid];
        for (size_t w = (size_t)(std::max<int64_t>(start, 0) >> 14); w < lin.size(); ++w) if (lin[w]) return lin[w];
        return 0;
    }
    // The chunks of every bin that overlaps [start, end) (reg2bins), without those that end at or before the linear index's
    // offset for start (htslib's pruning: no alignment that reaches start begins there); appended to out, unmerged.
    void region_chunks(int tid, int64_t start, int64_t end, std::vector<Chunk>& out) const {
        if (tid < 0 || tid >= (int)bins.size() || end <= start) return;
        const uint64_t min_off = linear_offset(tid, start);
        if (min_off == 0) return;
        const int64_t b = std::max<int64_t>(start, 0), e = std::min<int64_t>(end, (int64_t)1 << 29) - 1;
        if (e < b) return;
        const auto& m = bins[tid];
        auto take = [&](uint32_t bin) {
            const auto it = m.find(bin);
            if (it == m.end()) return;
            for (const Chunk& c : it->second) if (c.second > min_off && c.second > c.first) out.push_back(c);
        };
        take(0);
        const int shift[5] = {26, 23, 20, 17, 14};
        const uint32_t base[5] = {1, 9, 73, 585, 4681};
        for (int l = 0; l < 5; ++l)
            for (int64_t k = b >> shift[l]; k <= (e >> shift[l]); ++k) take(base[l] + (uint32_t)k);
    }
    // sorted, with overlapping and adjacent chunks merged
    static void merge_chunks(std::vector<Chunk>& v) {
        std::sort(v.begin(), v.end());
        size_t n = 0;
        for (const Chunk& c : v) {
            if (n > 0 && c.first <= v[n - 1].second) v[n - 1].second = std::max(v[n - 1].second, c.second);
            else v[n++] = c;
        }
        v.resize(n);
    }
};

}  // namespace bamn
