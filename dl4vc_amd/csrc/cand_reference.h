// Reference bases for the candidate generator's allele walk (cg_set_reference): the raw bytes of one FASTA contig, line breaks
// included, to one BAM nibble code ("=ACMGRSVTWYHKDBN") per base.  Plain C++ that compiles for the host and the device, so the
// rule that runs in cand_kernels.hip::reference_codes_kernel is the rule cg_reference_codes_host runs on the CPU (under a
// sanitizer: tools/asan_cand_reference.sh).
//   * base p of a contig with `lb` bases on a line of `lw` bytes lies at raw byte p + (p / lb) * (lw - lb);
//   * a letter of the alphabet maps to its code in either case (soft-masked acgtn included), '=' to 0;
//   * any other byte at a base position reads as N (15) and is counted;
//   * a line end ('\n', '\r') or '>' at a base position, or a base position past the raw bytes, means that the index does not
//     describe the file: the conversion stops being meaningful and the caller refuses the contig.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CR_HD __host__ __device__
#else
#define CR_HD
#endif

namespace cand {
namespace refc {

constexpr int OTHER = 16, BROKEN = 17;              // beside the codes 0..15
constexpr uint64_t NONE = ~(uint64_t)0;             // "no broken base"

// what the index must satisfy before any base is looked up
CR_HD inline bool layout_ok(int64_t lb, int64_t lw, int64_t length) { return length >= 0 && (length == 0 || (lb > 0 && lw >= lb)); }

// the raw bytes base 0 .. length - 1 span (the last line's break is not part of them)
CR_HD inline uint64_t raw_span(int64_t lb, int64_t lw, int64_t length) {
    return length <= 0 ? 0 : (uint64_t)(length - 1) + (uint64_t)((length - 1) / lb) * (uint64_t)(lw - lb) + 1;
}

// The one per-base rule: the code of base p (0..15), OTHER for a byte outside the alphabet (the caller stores 15 and counts
// it), BROKEN for a line end, '>' or a position past the raw bytes.  Reads raw[at] only for at < raw_len.
CR_HD inline int base_code(const uint8_t* raw, uint64_t raw_len, int64_t lb, int64_t lw, int64_t p) {
    const uint64_t at = (uint64_t)p + (uint64_t)(p / lb) * (uint64_t)(lw - lb);
    if (at >= raw_len) return BROKEN;
    const uint8_t c = raw[at];
    if (c == '\n' || c == '\r' || c == '>') return BROKEN;
    if (c == '=') return 0;
    switch (c & 0xdf) {      // (only 'a'..'z' fold onto 'A'..'Z')
        case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5; case 'S': return 6;
        case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11; case 'K': return 12;
        case 'D': return 13; case 'B': return 14; case 'N': return 15; default: return OTHER;
    }
}

// The CPU loop over the rule: out[0 .. length) and the count of other bytes; returns the first broken base, or NONE.  What
// lies in out behind a broken base is unspecified.
inline uint64_t codes_host(const uint8_t* raw, uint64_t raw_len, int64_t lb, int64_t lw, int64_t length, uint8_t* out, int64_t* n_other) {
    int64_t other = 0;
    for (int64_t p = 0; p < length; ++p) {
        const int c = base_code(raw, raw_len, lb, lw, p);
        if (c == BROKEN) { *n_other = other; return (uint64_t)p; }
        if (c == OTHER) ++other;
        out[p] = (uint8_t)(c == OTHER ? 15 : c);
    }
    *n_other = other;
    return NONE;
}

}  // namespace refc
}  // namespace cand
