// Left-alignment of one indel observation against the reference bases (cg_set_left_align): inside a homopolymer or a short
// tandem repeat the same event has several equally good placements, and the allele keys of cand_kernels.hip count each
// placement apart.  This is the one rule that moves an observation to its left-most placement, as plain C++ that compiles for
// the host and the device: Walk::close_run runs it per observation in count_kernel and emit_kernel, cg_left_align_host on the
// CPU (under a sanitizer: tools/asan_left_align.sh).
//
// Positions are 0-based.  An observation has a kind (INS or DEL), an anchor position a with its base, and L following bases
// B[0..L): the inserted read bases or the deleted reference bases.  Here they are the allele key's own words: w[0..4) holds
// L + 1 BAM nibble codes, 16 per word from the top, the anchor at index 0 and B[j] at index j + 1 (L <= MAX_L).
//   * eligible: the anchor pair is an aligned pair of the read (the caller says so); the anchor base and every B[j] are A, C, G
//     or T; codes[a] is the anchor base; for DEL a + L < length and codes[a + 1 + j] == B[j].  The last two catch a read whose MD
//     disagrees with the FASTA.  An observation that is not eligible stays as it is.
//   * shift: k = 0, and k -> k + 1 while a - k - 1 >= floor, codes[a - k - 1] is A, C, G or T, and
//       DEL: codes[a - k] == codes[a - k + L];
//       INS: codes[a - k] == S_k[L - 1], S_0 = B and S_{k+1} = S_k[L - 1] + S_k[0..L - 1): S_k[j] = B[(j - k) mod L].
//   * result: position a - k, anchor codes[a - k], bases codes[a - k + 1 .. a - k + L] (DEL) or S_k (INS).
//   * clamped: the shift stopped at the floor (a - k - 1 < floor) where floor 0 would have let it go on.
// floor is max(0, POS of the read): the read covers its shifted anchor, so the subregion the new position falls in fetches it.
// No element outside codes[0, length) is read, whatever the observation says.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CL_HD __host__ __device__
#else
#define CL_HD
#endif

namespace cand {
namespace lal {

constexpr int INS = 1, DEL = 2;                     // KIND_INS, KIND_DEL of cand_device.h
constexpr int MAX_L = 63;                           // w holds 64 codes, the anchor among them
constexpr int ELIGIBLE = 1, CLAMPED = 2;            // flags of align()

CL_HD inline bool acgt(int c) { return c == 1 || c == 2 || c == 4 || c == 8; }

// code i of w (selects, not an indexed load: w stays in registers on the device)
CL_HD inline int code_at(const uint64_t* w, int i) {
    const uint64_t x = i < 32 ? (i < 16 ? w[0] : w[1]) : (i < 48 ? w[2] : w[3]);
    return (int)((x >> (60 - 4 * (i & 15))) & 0xf);
}
CL_HD inline void put_code(uint64_t* w, int i, int code) {
    const uint64_t v = (uint64_t)code << (60 - 4 * (i & 15));
    if (i < 16) w[0] |= v; else if (i < 32) w[1] |= v; else if (i < 48) w[2] |= v; else w[3] |= v;
}

CL_HD inline bool eligible(int kind, bool anchor_aligned, const uint64_t* w, int L, const uint8_t* codes, int64_t length, int64_t a) {
    if (!anchor_aligned || L < 1 || L > MAX_L || (kind != INS && kind != DEL)) return false;
    if (a < 0 || a >= length) return false;
    for (int j = 0; j <= L; ++j)
        if (!acgt(code_at(w, j))) return false;
    if (codes[a] != code_at(w, 0)) return false;
    if (kind == DEL) {
        if (a + L >= length) return false;
        for (int j = 0; j < L; ++j)
            if (codes[a + 1 + j] != code_at(w, j + 1)) return false;
    }
    return true;
}

// the shift k of an eligible observation; *clamped as above
CL_HD inline int64_t shift(int kind, const uint64_t* w, int L, const uint8_t* codes, int64_t a, int64_t floor, bool* clamped) {
    if (floor < 0) floor = 0;
    int64_t k = 0;
    int last = L - 1;                               // S_k[L - 1] = B[last], last = (L - 1 - k) mod L
    *clamped = false;
    for (;;) {
        const int64_t p = a - k;                    // >= floor, and codes[p] is A, C, G or T
        if (p - 1 < 0 || !acgt(codes[p - 1])) break;
        if (codes[p] != (kind == DEL ? codes[p + L] : code_at(w, last + 1))) break;
        if (p - 1 < floor) { *clamped = true; break; }
        ++k;
        last = last == 0 ? L - 1 : last - 1;
    }
    return k;
}

// the observation at shift k > 0, written over w
CL_HD inline void place(int kind, uint64_t* w, int L, const uint8_t* codes, int64_t a, int64_t k) {
    const uint64_t b[4] = {w[0], w[1], w[2], w[3]};
    w[0] = w[1] = w[2] = w[3] = 0;
    put_code(w, 0, codes[a - k]);
    if (kind == DEL) {
        for (int j = 0; j < L; ++j) put_code(w, j + 1, codes[a - k + 1 + j]);
    } else {
        int from = (int)((L - k % L) % L);          // (0 - k) mod L
        for (int j = 0; j < L; ++j) {
            put_code(w, j + 1, code_at(b, from + 1));
            from = from + 1 == L ? 0 : from + 1;
        }
    }
}

// The whole rule.  Returns the shift k (0: w and the position a stay) and sets *flags.
CL_HD inline int64_t align(int kind, bool anchor_aligned, uint64_t* w, int L, const uint8_t* codes, int64_t length, int64_t a,
                           int64_t floor, int* flags) {
    *flags = 0;
    if (!eligible(kind, anchor_aligned, w, L, codes, length, a)) return 0;
    bool clamped = false;
    const int64_t k = shift(kind, w, L, codes, a, floor, &clamped);
    *flags = ELIGIBLE | (clamped ? CLAMPED : 0);
    if (k > 0) place(kind, w, L, codes, a, k);
    return k;
}

}  // namespace lal
}  // namespace cand
