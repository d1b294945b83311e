// Stand-alone driver of tools/asan_subsample.sh and tests/test_subsample_host.py: runs frame_record + sampled (the read
// subsampling rule of dl4vc_amd/csrc/bam_frame.h, the text the host paths and the GPU kernels run) over records whose name field
// is the edge of what the format allows.  Every record is copied into a heap buffer of exactly its size, so the sanitizer sees
// any byte read past it: l_read_name of 1, 2 and 255, a name with no NUL inside l_read_name, bytes >= 0x80 (widened as signed
// chars: no signed overflow, the arithmetic is uint32), and a record cut right behind the name.  The hashes are compared with
// values worked out independently here.  Exit status 0 when every case holds.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../dl4vc_amd/csrc/bam_frame.h"

namespace F = bamn::frame;

static int g_bad = 0, g_cases = 0;

static void expect(const char* name, const char* what, long long got, long long want) {
    if (got != want) { printf("FAIL %s: %s = %lld, expected %lld\n", name, what, got, want); ++g_bad; }
}

// X31 as the issue states it, on int64 with an explicit reduction: the independent restatement
static uint32_t x31(const std::string& s) {
    int64_t h = 0;
    bool first = true;
    for (const char ch : s) {
        if (ch == 0) break;
        const int64_t v = (int64_t)(signed char)ch;
        h = first ? v : h * 31 + v;
        h = ((h % 4294967296ll) + 4294967296ll) % 4294967296ll;
        first = false;
    }
    return (uint32_t)h;
}

// A record of the fixed fields, the name field `field` (its bytes as given: l_read_name = field.size()) and `tail` bytes behind
// it (n_cigar_op = l_seq = 0: the tail is aux area, not walked here), in a heap buffer of exactly its size.
struct Rec {
    std::unique_ptr<uint8_t[]> b;
    size_t size;
};
static Rec build(const std::string& field, size_t tail, size_t cut = 0) {
    Rec r;
    r.size = 32 + field.size() + tail - cut;
    r.b.reset(new uint8_t[r.size]);
    memset(r.b.get(), 0, r.size < 32 ? r.size : 32);
    if (r.size >= 32) {
        r.b[8] = (uint8_t)field.size();
        r.b[9] = 60;
        memcpy(r.b.get() + 32, field.data(), r.size - 32 < field.size() ? r.size - 32 : field.size());
    }
    return r;
}

static void keeps_case(const char* name, const std::string& field, const std::string& hashed) {
    ++g_cases;
    const Rec r = build(field, 0);                          // cut right behind the name: the record ends with the field
    F::Framed fr;
    expect(name, "frame_record", F::frame_record(r.b.get(), r.size, fr, false), F::W_NONE);
    expect(name, "l_name", fr.l_name, (long long)field.size());
    const uint32_t h = F::name_hash(r.b.get(), fr);
    expect(name, "name_hash", h, x31(hashed));
    for (const uint32_t seed : {0u, 7u, 0xffffffffu}) {
        const uint32_t v = F::wang(h ^ seed) & 0xffffffu;
        for (const double f : {1e-9, 0.3, 0.5, 1.0}) {
            F::SampleRule rule{0, 0};
            expect(name, "sample_rule", F::sample_rule(f, seed, rule) == nullptr, 1);
            expect(name, "sampled", F::sampled(r.b.get(), fr, rule), v < rule.threshold);
        }
        expect(name, "off keeps", F::sampled(r.b.get(), fr, F::SampleRule{seed, 0}), 1);
        expect(name, "F = 1 keeps", F::sampled(r.b.get(), fr, F::SampleRule{seed, 1u << 24}), 1);
    }
}

int main() {
    // the worked values
    {
        const char* name = "worked values";
        ++g_cases;
        expect(name, "X31(r1)", x31("r1"), 0x00000dff);
        expect(name, "X31(read/1)", x31("read/1"), 0xc84551f8u);
        expect(name, "wang", F::wang(0xc84551f8u ^ 42u), 0x1f4e6d53u);
        expect(name, "wang", F::wang(0x52e1ffc8u ^ 11u) & 0xffffffu, 7479631);
        expect(name, "threshold 0.3", F::sample_threshold(0.3), 5033165);
        expect(name, "threshold 0.5", F::sample_threshold(0.5), 8388608);
        expect(name, "threshold 0.6", F::sample_threshold(0.6), 10066330);
        expect(name, "threshold 1e-9", F::sample_threshold(1e-9), 1);
        expect(name, "threshold 1", F::sample_threshold(1.0), 16777216);
        F::SampleRule rule{1, 1};
        const double nan = std::nan("");
        expect(name, "NaN refused", F::sample_rule(nan, 0, rule) != nullptr, 1);
        expect(name, "-0.1 refused", F::sample_rule(-0.1, 0, rule) != nullptr, 1);
        expect(name, "1.5 refused", F::sample_rule(1.5, 0, rule) != nullptr, 1);
        expect(name, "a refusal leaves the rule", rule.threshold, 1);
        expect(name, "0 is off", F::sample_rule(0.0, 9, rule) == nullptr && rule.threshold == 0, 1);
    }
    keeps_case("l_read_name 1 (the NUL alone: an empty name)", std::string(1, '\0'), "");
    keeps_case("l_read_name 2", std::string("r\0", 2), "r");
    keeps_case("l_read_name 255", std::string(254, 'q') + std::string(1, '\0'), std::string(254, 'q'));
    keeps_case("no NUL inside l_read_name: l_read_name - 1 bytes are hashed, the last is never read as a name byte",
               std::string("abcd"), "abc");
    keeps_case("no NUL inside 255 bytes", std::string(255, 'z'), std::string(254, 'z'));
    keeps_case("a NUL in the middle", std::string("ab\0cd\0", 6), "ab");
    keeps_case("bytes >= 0x80", std::string("\x80\xff\xc3\xa9\x7f\x81", 6) + std::string(1, '\0'), std::string("\x80\xff\xc3\xa9\x7f\x81", 6));
    keeps_case("254 bytes of 0xff", std::string(254, '\xff') + std::string(1, '\0'), std::string(254, '\xff'));
    {
        // cut inside the name and right in front of it: frame_record refuses, and sampled is never reached
        const char* name = "cut inside the name";
        ++g_cases;
        F::Framed fr;
        const Rec in = build(std::string("abcdef\0", 7), 0, 3);
        expect(name, "frame_record", F::frame_record(in.b.get(), in.size, fr, false), F::W_NAME_EXCEEDS);
        const Rec front = build(std::string("abcdef\0", 7), 0, 7);
        expect(name, "frame_record (no name byte)", F::frame_record(front.b.get(), front.size, fr, false), F::W_NAME_EXCEEDS);
        const Rec behind = build(std::string("abcdef\0", 7), 5);
        expect(name, "frame_record (aux walk of zeros behind the name)", F::frame_record(behind.b.get(), behind.size, fr, true) != F::W_NONE, 1);
        expect(name, "frame_record (not walked)", F::frame_record(behind.b.get(), behind.size, fr, false), F::W_NONE);
        expect(name, "name_hash", F::name_hash(behind.b.get(), fr), x31("abcdef"));
    }
    if (g_bad) { printf("asan_subsample: %d of %d cases FAILED\n", g_bad, g_cases); return 1; }
    printf("asan_subsample: OK (%d cases)\n", g_cases);
    return 0;
}
