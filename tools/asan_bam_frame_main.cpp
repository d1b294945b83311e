// Stand-alone driver of tools/asan_bam_frame.sh and tests/test_bam_frame_host.py: runs the BAM frame core
// (dl4vc_amd/csrc/bam_frame.h, the text the host paths and the GPU kernels run) over a grid of well-formed and damaged records.
// Every record is copied into a heap buffer of exactly its size, so the sanitizer sees any byte read past it, and the reason
// and every field of the Framed are compared with what the record was built from.  Exit status 0 when every case holds.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../dl4vc_amd/csrc/bam_frame.h"

namespace F = bamn::frame;

static int g_bad = 0, g_cases = 0;

#define EXPECT_EQ(what, got, want)                                                                                   \
    do {                                                                                                             \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                               \
        if (g_ != w_) { printf("FAIL %s: %s = %lld, expected %lld\n", name, what, g_, w_); ++g_bad; }                \
    } while (0)

static void put32(std::vector<uint8_t>& v, size_t o, uint32_t x) { for (int i = 0; i < 4; ++i) v[o + i] = (uint8_t)(x >> (8 * i)); }
static void put16(std::vector<uint8_t>& v, size_t o, uint32_t x) { v[o] = (uint8_t)x; v[o + 1] = (uint8_t)(x >> 8); }

struct Ops { std::vector<uint32_t> v; };
static Ops cigar(std::initializer_list<std::pair<uint32_t, char>> ops) {
    Ops c;
    for (const auto& o : ops) c.v.push_back((o.first << 4) | (uint32_t)(strchr("MIDNSHP=X", o.second) - "MIDNSHP=X"));
    return c;
}

// one record (the bytes behind block_size): name "r\0", the CIGAR, l_seq bases and qualities, the aux area as given
struct Built {
    std::vector<uint8_t> b;
    uint32_t cigar_off, seq_off, qual_off, aux_off;
};
static Built build(int32_t tid, int32_t pos, uint32_t flag, const Ops& cg, int32_t l_seq, const std::string& aux) {
    Built r;
    const uint32_t l_name = 2;
    r.cigar_off = 32 + l_name;
    r.seq_off = r.cigar_off + 4 * (uint32_t)cg.v.size();
    r.qual_off = r.seq_off + ((uint32_t)l_seq + 1) / 2;
    r.aux_off = r.qual_off + (uint32_t)l_seq;
    r.b.assign(r.aux_off, 0);
    put32(r.b, 0, (uint32_t)tid);
    put32(r.b, 4, (uint32_t)pos);
    r.b[8] = (uint8_t)l_name;
    r.b[9] = 60;
    put16(r.b, 12, (uint32_t)cg.v.size());
    put16(r.b, 14, flag);
    put32(r.b, 16, (uint32_t)l_seq);
    put32(r.b, 20, 0xffffffffu);
    put32(r.b, 24, 0xffffffffu);
    r.b[32] = 'r';
    for (size_t i = 0; i < cg.v.size(); ++i) put32(r.b, r.cigar_off + 4 * i, cg.v[i]);
    for (uint32_t i = r.seq_off; i < r.qual_off; ++i) r.b[i] = 0x12;
    for (uint32_t i = r.qual_off; i < r.aux_off; ++i) r.b[i] = 30;
    r.b.insert(r.b.end(), aux.begin(), aux.end());
    return r;
}

// frame_record over a heap copy of exactly `size` bytes; the copy stays alive in `heap` for the CIGAR calls that follow
static uint8_t* g_heap = nullptr;
static uint32_t frame(const std::vector<uint8_t>& b, size_t size, F::Framed& fr, bool aux) {
    free(g_heap);
    g_heap = (uint8_t*)malloc(size ? size : 1);
    memcpy(g_heap, b.data(), size);
    memset(&fr, 0x5a, sizeof fr);
    return F::frame_record(g_heap, size, fr, aux);
}

static void expect_fields(const char* name, const F::Framed& fr, const Built& r, int32_t tid, int32_t pos, uint32_t flag, uint32_t n_cig,
                          int32_t l_seq, int32_t md_off, int32_t md_len) {
    EXPECT_EQ("tid", fr.tid, tid); EXPECT_EQ("pos", fr.pos, pos); EXPECT_EQ("flag", fr.flag, flag);
    EXPECT_EQ("n_cig", fr.n_cig, n_cig); EXPECT_EQ("l_seq", fr.l_seq, l_seq); EXPECT_EQ("l_name", fr.l_name, 2);
    EXPECT_EQ("cigar_off", fr.cigar_off, r.cigar_off); EXPECT_EQ("seq_off", fr.seq_off, r.seq_off);
    EXPECT_EQ("qual_off", fr.qual_off, r.qual_off); EXPECT_EQ("aux_off", fr.aux_off, r.aux_off);
    EXPECT_EQ("md_off", fr.md_off, md_off); EXPECT_EQ("md_len", fr.md_len, md_len);
    EXPECT_EQ("nref", fr.nref, 0); EXPECT_EQ("nquery", fr.nquery, 0); EXPECT_EQ("has_ref", fr.has_ref, 0); EXPECT_EQ("skip", fr.skip, 0);
}

// an aux area: accepted with the MD it holds (md_at: offset of the value inside the area, -1 for none), or refused with `why`;
// without the aux walk it is accepted either way, MD -1
static void aux_case(const char* name, const std::string& aux, uint32_t why, int md_at, int md_len) {
    const Ops cg = cigar({{10, 'M'}});
    const Built r = build(3, 1000, 16, cg, 10, aux);
    F::Framed fr;
    ++g_cases;
    EXPECT_EQ("why", frame(r.b, r.b.size(), fr, true), why);
    if (why == F::W_NONE) expect_fields(name, fr, r, 3, 1000, 16, 1, 10, md_at < 0 ? -1 : (int32_t)r.aux_off + md_at, md_at < 0 ? -1 : md_len);
    ++g_cases;
    EXPECT_EQ("why without the aux walk", frame(r.b, r.b.size(), fr, false), F::W_NONE);
    expect_fields(name, fr, r, 3, 1000, 16, 1, 10, -1, -1);
}

// a record cut to `size` bytes, or with one fixed field overwritten, that the fixed-field checks refuse (with and without aux)
static void fixed_case(const char* name, std::vector<uint8_t> b, size_t size, uint32_t why) {
    F::Framed fr;
    for (const bool aux : {true, false}) {
        ++g_cases;
        EXPECT_EQ(aux ? "why" : "why without the aux walk", frame(b, size, fr, aux), why);
    }
}

static void cigar_case(const char* name, int32_t pos, uint32_t flag, const Ops& cg, int64_t nref, int64_t nquery, bool has_ref, bool skip,
                       int64_t end, uint32_t walk_why) {
    const Built r = build(0, pos, flag, cg, 4, std::string("MDZ4\0", 5));
    F::Framed fr;
    ++g_cases;
    EXPECT_EQ("why", frame(r.b, r.b.size(), fr, true), F::W_NONE);
    expect_fields(name, fr, r, 0, pos, flag, (uint32_t)cg.v.size(), 4, (int32_t)r.aux_off + 3, 1);
    for (const bool checked : {false, true}) {
        uint32_t why = F::W_NONE;
        if (checked) why = F::walk_cigar(g_heap, fr); else F::cigar_sums(g_heap, fr);
        EXPECT_EQ(checked ? "walk_cigar" : "cigar_sums", why, checked ? walk_why : (uint32_t)F::W_NONE);
        EXPECT_EQ("nref", fr.nref, nref); EXPECT_EQ("nquery", fr.nquery, nquery);
        EXPECT_EQ("has_ref", fr.has_ref, has_ref); EXPECT_EQ("skip", fr.skip, skip);
        EXPECT_EQ("endpos", F::endpos(fr), end);
    }
}

// one chain step over a heap buffer of exactly `total` bytes whose block_size field at `at` holds `field`
static void chain_case(const char* name, uint64_t total, uint64_t stop, uint64_t at, uint32_t field, uint32_t why) {
    uint8_t* infl = (uint8_t*)malloc(total);
    memset(infl, 0, total);
    for (int i = 0; i < 4 && at + i < total; ++i) infl[at + i] = (uint8_t)(field >> (8 * i));
    uint32_t size = 77;
    ++g_cases;
    EXPECT_EQ("why", F::next_record(infl, total, stop, at, size), why);
    if (why == F::W_NONE) EXPECT_EQ("size", size, field);
    free(infl);
}

int main() {
    const std::string nm("NMC\x01", 4);
    auto z = [](const char* tag, const char* v) { return std::string(tag) + std::string(v) + std::string(1, '\0'); };
    // ---- the aux area ----
    aux_case("plain MD:Z", nm + z("MDZ", "10A5"), F::W_NONE, 7, 4);
    aux_case("no MD", nm, F::W_NONE, -1, 0);
    aux_case("no aux area", "", F::W_NONE, -1, 0);
    aux_case("MD:H before MD:Z", z("MDH", "1AE3") + z("MDZ", "7"), F::W_NONE, 8 + 3, 1);
    aux_case("two MD:Z, the first wins", z("MDZ", "3") + z("MDZ", "10A5"), F::W_NONE, 3, 1);
    aux_case("empty MD:Z", z("MDZ", ""), F::W_NONE, 3, 0);
    aux_case("B array before MD:Z", std::string("XBBs\x02\0\0\0abcd", 12) + z("MDZ", "9"), F::W_NONE, 12 + 3, 1);
    aux_case("every fixed-size type", std::string("aaAx" "bbcx" "ccCx" "ddsxx" "eeSxx" "ffixxxx" "ggIxxxx" "hhfxxxx", 43) + z("MDZ", "2"), F::W_NONE, 43 + 3, 1);
    aux_case("tag cut after 1 byte", nm + "M", F::W_AUX_TAG, -1, 0);
    aux_case("tag cut after 2 bytes", nm + "MD", F::W_AUX_TAG, -1, 0);
    aux_case("Z without NUL", nm + "MDZ10A5", F::W_AUX_NUL, -1, 0);
    aux_case("Z with nothing behind the type", nm + "MDZ", F::W_AUX_NUL, -1, 0);
    aux_case("B with 4 header bytes", std::string("XBBc\x01\0\0", 7), F::W_AUX_ARRAY, -1, 0);
    aux_case("B of element type x", std::string("XBBx\0\0\0\0", 8), F::W_AUX_ARRAY_TYPE, -1, 0);
    aux_case("B one element short", std::string("XBBs\x02\0\0\0abc", 11), F::W_AUX_ARRAY, -1, 0);
    aux_case("B whose n x size overflows 32 bits", std::string("XBBi\x01\0\0\x40" "abcd", 12), F::W_AUX_ARRAY, -1, 0);
    aux_case("value type x", nm + "XYx", F::W_AUX_TYPE, -1, 0);
    aux_case("i value cut by one byte", std::string("NMi\x01\0\0", 6), F::W_AUX_VALUE, -1, 0);
    // ---- the fixed fields ----
    {
        const Built r = build(0, 5, 0, cigar({{8, 'M'}}), 8, "");
        const char* name;
        std::vector<uint8_t> b = r.b;
        name = "size 31"; fixed_case(name, b, 31, F::W_BLOCK_SIZE);
        name = "size 32"; fixed_case(name, b, 32, F::W_NAME_EXCEEDS);
        name = "name one byte past the record"; fixed_case(name, b, r.cigar_off - 1, F::W_NAME_EXCEEDS);
        name = "CIGAR one byte past the record"; fixed_case(name, b, r.seq_off - 1, F::W_CIGAR_EXCEEDS);
        name = "SEQ one byte past the record"; fixed_case(name, b, r.aux_off - 1, F::W_SEQ_EXCEEDS);
        b[8] = 0;
        name = "l_read_name 0"; fixed_case(name, b, b.size(), F::W_L_NAME);
        b = r.b; put32(b, 16, 0xffffffffu);
        name = "l_seq -1"; fixed_case(name, b, b.size(), F::W_L_SEQ);
        b = r.b; put32(b, 16, 0x7fffffffu);
        name = "l_seq INT32_MAX"; fixed_case(name, b, b.size(), F::W_SEQ_EXCEEDS);
        b = r.b; put16(b, 12, 0xffff);
        name = "n_cigar_op 65535"; fixed_case(name, b, b.size(), F::W_CIGAR_EXCEEDS);
    }
    // ---- the CIGAR ----
    cigar_case("10M2I3D4N5S6H7=8X", 100, 0, cigar({{10, 'M'}, {2, 'I'}, {3, 'D'}, {4, 'N'}, {5, 'S'}, {6, 'H'}, {7, '='}, {8, 'X'}}), 32, 32, true, true, 132, F::W_NONE);
    cigar_case("unmapped with a CIGAR", 100, 4, cigar({{10, 'M'}}), 10, 10, true, false, 101, F::W_NONE);
    cigar_case("empty CIGAR", 100, 0, cigar({}), 0, 0, false, false, 101, F::W_NONE);
    cigar_case("no reference-consuming operation", 100, 0, cigar({{4, 'S'}, {3, 'I'}, {2, 'P'}}), 0, 7, false, false, 101, F::W_NONE);
    cigar_case("600000000M", 100, 0, cigar({{200000000, 'M'}, {200000000, 'M'}, {200000000, 'M'}}), 600000000, 600000000, true, false, 600000100,
               F::W_CIGAR_REF);
    cigar_case("span past INT32_MAX", INT32_MAX - 10, 0, cigar({{100, 'M'}}), 100, 100, true, false, (int64_t)INT32_MAX + 90, F::W_CIGAR_REF);
    cigar_case("span up to INT32_MAX", INT32_MAX - 100, 0, cigar({{100, 'M'}}), 100, 100, true, false, (int64_t)INT32_MAX, F::W_NONE);
    // ---- one step of the record chain ----
    {
        const char* name;
        name = "3 bytes before stop"; chain_case(name, 103, 103, 100, 40, F::W_OVER_STOP);
        name = "block_size 31"; chain_case(name, 200, 200, 100, 31, F::W_BLOCK_SIZE);
        name = "block_size 2^28 + 1"; chain_case(name, 200, 200, 100, (1u << 28) + 1, F::W_BLOCK_SIZE);
        name = "block_size 0xffffffff"; chain_case(name, 200, 200, 100, 0xffffffffu, F::W_BLOCK_SIZE);
        name = "past total"; chain_case(name, 200, 200, 100, 97, F::W_TRUNCATED);
        name = "2^28 past total"; chain_case(name, 200, 200, 100, 1u << 28, F::W_TRUNCATED);
        name = "past stop, inside total"; chain_case(name, 200, 180, 100, 77, F::W_OVER_STOP);
        name = "at stop exactly"; chain_case(name, 200, 180, 100, 76, F::W_NONE);
        name = "at stop and total exactly"; chain_case(name, 200, 200, 100, 96, F::W_NONE);
        name = "block_size 32 before stop"; chain_case(name, 200, 180, 100, 32, F::W_NONE);
    }
    // ---- the texts ----
    {
        const char* name = "why_text";
        ++g_cases;
        EXPECT_EQ("aux string text", strcmp(F::why_text(F::W_AUX_NUL), "corrupt BAM record (aux string without its NUL)"), 0);
        EXPECT_EQ("aux value type text", strcmp(F::why_text(F::W_AUX_TYPE), "corrupt BAM record (aux value type)"), 0);
        EXPECT_EQ("truncated text", strcmp(F::why_text(F::W_TRUNCATED), "truncated BAM record"), 0);
        EXPECT_EQ("CIGAR text", strcmp(F::why_text(F::W_CIGAR_REF), "corrupt BAM record (CIGAR reference length)"), 0);
        EXPECT_EQ("unknown reason", strcmp(F::why_text(F::W_COUNT), "corrupt BAM record"), 0);
        EXPECT_EQ("W_AUX_VALUE", F::W_AUX_VALUE, 14);
        EXPECT_EQ("W_COUNT", F::W_COUNT, 16);
    }
    free(g_heap);
    printf("%s: %d cases, %d mismatches\n", g_bad ? "FAILED" : "ok", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
