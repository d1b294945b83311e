// Stand-alone driver of tools/asan_left_align.sh: the left-alignment rule of dl4vc_amd/csrc/cand_left_align.h (the rule
// Walk::close_run runs on the GPU) under AddressSanitizer and UBSan, called as the kernels call it (lal::align on the key's
// words) and through cg_left_align_host.  Every contig lives in a heap buffer that ends where it ends, so one code read before
// or past it is reported.  Each result is held to what left-alignment means, stated without the rule's own arithmetic: the
// haplotype (the contig with the indel applied) is unchanged, the placement does not lie below the floor, and no further step
// to the left is possible -- or the floor is the only thing in its way, which is what `clamped` says.
// The grid: contigs of 1..12 bases over {A, C, N} (all of them up to 9 bases, every 3rd of 10, every 27th of 11 and every 81st of 12), every
// anchor, L in 1..4, both kinds, every floor.  Then hostile observations: an anchor at 0, below 0 and past the contig, a + L at
// and past the contig's end, L = 63 with a shift far beyond L, and L = 64, which no key holds.
#include "../dl4vc_amd/csrc/cand_left_align.h"
#include "../include/dl4vc_candgen.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

namespace L = cand::lal;
long long failures = 0, cases = 0, shifted = 0, clamped_n = 0, beyond = 0;

void check(bool ok, const char* what, const std::string& g, int kind, long long a, int len, long long floor) {
    if (ok) return;
    if (++failures <= 20) fprintf(stderr, "FAIL %s: contig %s kind %d anchor %lld L %d floor %lld\n", what, g.c_str(), kind, a, len, floor);
}

std::string letters(const uint8_t* c, size_t n) {
    std::string s;
    for (size_t i = 0; i < n; ++i) s += "=ACMGRSVTWYHKDBN"[c[i] & 15];
    return s;
}

// the contig with the indel applied
std::vector<uint8_t> haplotype(const std::vector<uint8_t>& g, int kind, long long a, const std::vector<uint8_t>& bases) {
    std::vector<uint8_t> h(g.begin(), g.begin() + a + 1);
    if (kind == L::INS) {
        h.insert(h.end(), bases.begin(), bases.end());
        h.insert(h.end(), g.begin() + a + 1, g.end());
    } else {
        h.insert(h.end(), g.begin() + a + 1 + (long long)bases.size(), g.end());
    }
    return h;
}

bool acgt(int c) { return c == 1 || c == 2 || c == 4 || c == 8; }

// one observation through both entries
void run(const std::vector<uint8_t>& g, int kind, long long a, int anchor, const std::vector<uint8_t>& bases, long long floor) {
    const int len = (int)bases.size();
    const std::string name = letters(g.data(), g.size());
    std::unique_ptr<uint8_t[]> codes(new uint8_t[g.size()]);                  // exact size: the red zone starts at its end
    memcpy(codes.get(), g.data(), g.size());
    std::unique_ptr<uint8_t[]> out(new uint8_t[len + 1]);
    int64_t pos = -1;
    int32_t flags = -1;
    const int rc = cg_left_align_host(codes.get(), (int64_t)g.size(), kind, 1, a, anchor, bases.data(), len, floor, &pos, out.get(), &flags);
    check(rc == 0, cg_last_error(), name, kind, a, len, floor);
    if (rc) return;
    ++cases;
    bool fits = len <= L::MAX_L && (anchor & ~15) == 0;
    for (int j = 0; j < len; ++j) fits = fits && bases[j] < 16;
    if (fits) {                                                               // the kernels' call: the key's words, in place
        uint64_t w[4] = {0, 0, 0, 0};
        L::put_code(w, 0, anchor);
        for (int j = 0; j < len; ++j) L::put_code(w, j + 1, bases[j]);
        int fl = 0;
        const int64_t k = L::align(kind, true, w, len, codes.get(), (int64_t)g.size(), a, floor, &fl);
        check(a - k == pos && fl == flags, "the two entries disagree", name, kind, a, len, floor);
        for (int j = 0; j <= len; ++j) check(L::code_at(w, j) == out[j], "the two entries disagree on a base", name, kind, a, len, floor);
    }
    if (!(flags & L::ELIGIBLE)) {
        check(pos == a && out[0] == anchor && (len == 0 || memcmp(out.get() + 1, bases.data(), len) == 0) && flags == 0,
              "an observation that is not eligible came back changed", name, kind, a, len, floor);
        return;
    }
    const long long fl0 = floor < 0 ? 0 : floor;
    std::vector<uint8_t> nb(out.get() + 1, out.get() + 1 + len);
    check(pos <= a && pos >= 0 && (pos >= fl0 || pos == a), "placement below the floor", name, kind, a, len, floor);
    check(out[0] == g[pos] && acgt(out[0]), "anchor is not the contig's base", name, kind, a, len, floor);
    check(haplotype(g, kind, a, bases) == haplotype(g, kind, pos, nb), "the haplotype changed", name, kind, a, len, floor);
    // one more step: possible when the contig's base to the left is ACGT and the indel moved there gives the same haplotype
    bool more = false;
    if (pos >= 1 && acgt(g[pos - 1])) {
        std::vector<uint8_t> mb(nb);
        if (kind == L::INS) { mb.insert(mb.begin(), mb.back()); mb.pop_back(); }
        else for (int j = 0; j < len; ++j) mb[j] = g[pos + j];
        more = (kind == L::DEL ? g[pos] == g[pos + len] : g[pos] == nb.back()) && haplotype(g, kind, pos - 1, mb) == haplotype(g, kind, a, bases);
    }
    const bool at_floor = pos - 1 < fl0;
    check(!more || at_floor, "not left-most", name, kind, a, len, floor);
    check(((flags & L::CLAMPED) != 0) == (more && at_floor), "clamped is wrong", name, kind, a, len, floor);
    shifted += pos != a;
    clamped_n += (flags & L::CLAMPED) != 0;
    beyond += a - pos > len;
}

}  // namespace

int main() {
    const uint8_t alphabet[3] = {1, 2, 15};                                   // A, C, N
    const char* words[] = {"AAAA", "ACAC", "CACA", "CCAC"};
    for (int n = 1; n <= 12; ++n) {
        long long total = 1;
        for (int i = 0; i < n; ++i) total *= 3;
        const long long step = n <= 9 ? 1 : n == 10 ? 3 : n == 11 ? 27 : 81;
        for (long long id = 0; id < total; id += step) {
            std::vector<uint8_t> g(n);
            long long v = id;
            for (int i = 0; i < n; ++i) { g[i] = alphabet[v % 3]; v /= 3; }
            for (int a = 0; a < n; ++a)
                for (int len = 1; len <= 4; ++len)
                    for (int floor = 0; floor <= a; ++floor) {
                        std::vector<uint8_t> del(len, 1);
                        for (int j = 0; j < len && a + 1 + j < n; ++j) del[j] = g[a + 1 + j];
                        run(g, L::DEL, a, g[a], del, floor);
                        for (const char* word : words) {
                            std::vector<uint8_t> ins(len);
                            for (int j = 0; j < len; ++j) ins[j] = word[j] == 'A' ? 1 : 2;
                            if (n > 8 && word != words[1] && word != words[2]) continue;
                            run(g, L::INS, a, g[a], ins, floor);
                        }
                    }
        }
    }
    const long long grid_cases = cases;
    // hostile observations
    std::vector<uint8_t> rep(1, 4);                                           // G (AC)x60
    for (int i = 0; i < 60; ++i) { rep.push_back(1); rep.push_back(2); }
    const std::vector<uint8_t> one(1, 2);
    for (const long long a : {-1LL, -1000000000000LL, 121LL, 122LL, 1LL << 40}) run(rep, L::DEL, a, 1, one, 0);
    run(rep, L::DEL, 0, 4, std::vector<uint8_t>(1, 1), 0);                    // an anchor at 0
    run(rep, L::INS, 0, 4, one, 0);
    for (int len = 1; len <= 63; ++len)                                       // a + L around the contig's end, up to L = 63
        for (long long a = 121 - len - 2; a <= 120; ++a) {
            if (a < 0) continue;
            std::vector<uint8_t> del(len, 1);
            for (int j = 0; j < len && a + 1 + j < 121; ++j) del[j] = rep[a + 1 + j];
            run(rep, L::DEL, a, rep[a], del, 0);
            run(rep, L::DEL, a, rep[a], del, a / 2);
        }
    for (const int len : {62, 63, 64, 200}) {                                 // long insertions at the end of the repeat
        std::vector<uint8_t> ins(len);
        for (int j = 0; j < len; ++j) ins[j] = (len - 1 - j) & 1 ? 1 : 2;     // ends with C, the base of anchor 120
        run(rep, L::INS, 120, 2, ins, 0);
        run(rep, L::INS, 120, 2, ins, 7);
        run(rep, L::INS, 120, 2, ins, -3);
    }
    run(rep, L::INS, 120, 2, std::vector<uint8_t>(3, 200), 0);                // codes that are no codes
    run(rep, L::INS, 120, 99, one, 0);
    run(rep, 7, 120, 2, one, 0);                                              // a kind that is none
    if (beyond < 1000 || clamped_n < 1000 || shifted < 100000) { fprintf(stderr, "the grid exercised too little: %lld shifted, %lld clamped, %lld beyond L\n", shifted, clamped_n, beyond); return 1; }
    if (failures) { fprintf(stderr, "%lld failures\n", failures); return 1; }
    printf("asan_left_align: ok (%lld grid cases, %lld hostile; %lld shifted, %lld clamped, %lld shifted by more than L)\n", grid_cases,
           cases - grid_cases, shifted, clamped_n, beyond);
    return 0;
}
