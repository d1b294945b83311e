// Stand-alone driver of tools/asan_read_filter.sh and tests/test_read_filter_host.py: runs frame_record + passes + fate (the
// read filter and the host census of dl4vc_amd/csrc/bam_frame.h, the text the host paths and the GPU kernels run) over records in
// heap buffers of exactly their size, so the sanitizer sees any byte read past one: the smallest record there is (33 bytes, an
// empty name), every single flag bit, 0 and 0xFFFF, MAPQ 0 / Q - 1 / Q / Q + 1 / 255, and a record cut to 31 bytes (refused by
// frame_record before the filter looks at it).  The verdicts are compared with the rule written out here, the census with counts
// kept here, and the setter's refusals are tried.  Exit status 0 when every case holds.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../dl4vc_amd/csrc/bam_frame.h"

namespace F = bamn::frame;

static int g_bad = 0, g_cases = 0;

static void expect(const char* what, long long got, long long want) {
    ++g_cases;
    if (got != want) { printf("FAIL %s = %lld, expected %lld\n", what, got, want); ++g_bad; }
}

struct Rec {
    std::unique_ptr<uint8_t[]> b;
    size_t size;
};
static Rec build(uint32_t flag, uint32_t mapq, size_t size = 33) {
    Rec r;
    r.size = size;
    r.b.reset(new uint8_t[size]);
    memset(r.b.get(), 0, size);
    if (size > 15) {
        r.b[8] = 1;
        r.b[9] = (uint8_t)mapq;
        r.b[14] = (uint8_t)(flag & 0xff);
        r.b[15] = (uint8_t)(flag >> 8);
    }
    return r;
}

int main() {
    std::vector<uint32_t> flags{0, 0xffff};
    for (int k = 0; k < 16; ++k) flags.push_back(1u << k);
    const int64_t filters[][3] = {{0, 0, 0}, {0, 0, 20}, {0x704, 0, 0}, {0x900, 0x1, 1}, {0xfffe, 0x1, 255}, {0, 0xffff, 0}};
    for (const auto& a : filters) {
        F::ReadFilter f{0, 0, 0};
        expect("read_filter accepts", F::read_filter(a[0], a[1], a[2], f) == nullptr, 1);
        const F::SampleRule off{0, 0};
        F::Census census;
        long long seen = 0, by_flags = 0, by_mapq = 0, kept = 0, hist[256] = {0}, bits[16] = {0};
        const uint32_t q = (uint32_t)a[2];
        for (const uint32_t mapq : {0u, q ? q - 1 : 0u, q, q < 255 ? q + 1 : 255u, 254u, 255u})
            for (const uint32_t flag : flags) {
                Rec r = build(flag, mapq);
                F::Framed fr;
                expect("frame_record", F::frame_record(r.b.get(), r.size, fr, false), F::W_NONE);
                const bool flags_ok = (flag & (uint32_t)a[0]) == 0 && (flag & (uint32_t)a[1]) == (uint32_t)a[1];
                const bool want = flags_ok && mapq >= q;
                expect("passes", F::passes(r.b.get(), fr, f), want);
                expect("fate without a census", F::fate(nullptr, r.b.get(), fr, f, off), want ? F::FATE_KEPT : F::FATE_FILTERED);
                expect("fate", F::fate(&census, r.b.get(), fr, f, off, 2), want ? F::FATE_KEPT : F::FATE_FILTERED);
                seen += 2; hist[mapq] += 2;
                for (int k = 0; k < 16; ++k) if (flag >> k & 1) bits[k] += 2;
                if (!flags_ok) by_flags += 2; else if (!want) by_mapq += 2; else kept += 2;
            }
        expect("census seen", (long long)census.w[F::CENSUS_SEEN], seen);
        expect("census dropped_flags", (long long)census.w[F::CENSUS_DROP_FLAGS], by_flags);
        expect("census dropped_mapq", (long long)census.w[F::CENSUS_DROP_MAPQ], by_mapq);
        expect("census kept", (long long)census.w[F::CENSUS_KEPT], kept);
        for (int m = 0; m < 256; ++m) expect("census mapq_hist", (long long)census.w[F::CENSUS_MAPQ + m], hist[m]);
        for (int k = 0; k < 16; ++k) expect("census flag_bits", (long long)census.w[F::CENSUS_FLAG + k], bits[k]);
        F::Census sum;
        sum.add(census);
        sum.add(census);
        expect("census add", (long long)sum.w[F::CENSUS_SEEN], 2 * seen);
    }
    // the sample rule comes behind the filter: a read the rule drops counts as seen and not as kept
    {
        F::ReadFilter f{0, 0, 0};
        F::read_filter(0x400, 0, 0, f);
        F::SampleRule rule{0, 0};
        F::sample_rule(1e-9, 0, rule);                              // (keeps next to nothing)
        F::Census c;
        Rec r = build(0, 60);
        F::Framed fr;
        F::frame_record(r.b.get(), r.size, fr, false);
        expect("fate behind the rule", F::fate(&c, r.b.get(), fr, f, rule), F::FATE_UNSAMPLED);
        expect("seen behind the rule", (long long)c.w[F::CENSUS_SEEN], 1);
        expect("kept behind the rule", (long long)c.w[F::CENSUS_KEPT], 0);
    }
    // a record of 31 bytes carrying an excluded flag is refused by the frame core: the filter never sees it
    {
        Rec r = build(0x400, 0, 31);
        F::Framed fr;
        expect("a cut record", F::frame_record(r.b.get(), r.size, fr, false), F::W_BLOCK_SIZE);
    }
    F::ReadFilter f{1, 2, 3};
    expect("refuses exclude", F::read_filter(0x10000, 0, 0, f) != nullptr, 1);
    expect("refuses exclude < 0", F::read_filter(-1, 0, 0, f) != nullptr, 1);
    expect("refuses require", F::read_filter(0, 0x10000, 0, f) != nullptr, 1);
    expect("refuses min_mapq", F::read_filter(0, 0, 256, f) != nullptr, 1);
    expect("refuses min_mapq < 0", F::read_filter(0, 0, -1, f) != nullptr, 1);
    expect("refuses a shared bit", F::read_filter(0x5, 0x4, 0, f) != nullptr, 1);
    expect("a refusal leaves the filter", f.exclude == 1 && f.require == 2 && f.min_mapq == 3, 1);
    if (g_bad) { printf("asan_read_filter: %d of %d checks FAILED\n", g_bad, g_cases); return 1; }
    printf("asan_read_filter: OK (%d checks)\n", g_cases);
    return 0;
}
