// Stand-alone driver of tools/asan_cand_reference.sh: cg_reference_codes_host (the CPU loop over the per-base rule that
// reference_codes_kernel runs on the GPU) under AddressSanitizer and UBSan.  Every input and output lives in a heap buffer that
// ends where it ends, so one byte read or written past either is reported.  The shapes: lengths 0, 1, linebases - 1, linebases,
// linebases + 1 and several lines, LF and CRLF line ends, a last line without a line end, every byte value at a base position,
// and indexes that do not describe the bytes (wrong line width, bytes that end early), which must be refused, not followed.
#include "../include/dl4vc_candgen.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

namespace {

const char CODES[] = "=ACMGRSVTWYHKDBN";
int failures = 0;

void check(bool ok, const char* what, const std::string& name) {
    if (!ok) { fprintf(stderr, "FAIL %s: %s\n", name.c_str(), what); ++failures; }
}

std::string wrap(const std::string& seq, size_t lb, const char* eol, bool final) {
    std::string out;
    for (size_t i = 0; i < seq.size(); i += lb) {
        out += seq.substr(i, lb);
        if (i + lb < seq.size() || final) out += eol;
    }
    return out;
}

// exact-size heap copies: the sanitizer's red zones start at their ends
struct Run {
    std::unique_ptr<uint8_t[]> raw, out;
    int64_t other = -1;
    int rc = 0;
    Run(const std::string& bytes, int64_t lb, int64_t lw, int64_t length) : raw(new uint8_t[bytes.size()]), out(new uint8_t[(size_t)(length > 0 ? length : 0)]) {
        memcpy(raw.get(), bytes.data(), bytes.size());
        rc = cg_reference_codes_host(raw.get(), bytes.size(), lb, lw, length, out.get(), &other);
    }
};

void good(const std::string& name, const std::string& seq, size_t lb, const char* eol, bool final) {
    const std::string bytes = wrap(seq, lb, eol, final);
    Run r(bytes, (int64_t)lb, (int64_t)(lb + strlen(eol)), (int64_t)seq.size());
    check(r.rc == 0, cg_last_error(), name);
    if (r.rc) return;
    int64_t other = 0;
    for (size_t p = 0; p < seq.size(); ++p) {
        const char c = seq[p], up = (c >= 'a' && c <= 'z') ? (char)(c - 32) : c;
        const char* at = (up == '=' || (up >= 'A' && up <= 'Z')) ? strchr(CODES, up) : nullptr;
        other += !at;
        check(r.out[p] == (at ? at - CODES : 15), "wrong code", name + " base " + std::to_string(p));
    }
    check(r.other == other, "wrong count of other bytes", name);
}

void refused(const std::string& name, const std::string& bytes, int64_t lb, int64_t lw, int64_t length) {
    Run r(bytes, lb, lw, length);
    check(r.rc != 0 && *cg_last_error(), "accepted", name);
}

}  // namespace

int main() {
    const size_t lb = 50;
    std::string seq;
    const char letters[] = "ACGTacgtNnRYKMSWBDHVrykm=*-.xX@";
    uint32_t s = 12345;
    for (int i = 0; i < 4 * 50 + 9; ++i) {
        s = s * 1664525u + 1013904223u;
        seq += letters[(s >> 16) % (sizeof letters - 1)];
    }
    for (const size_t n : {(size_t)0, (size_t)1, lb - 1, lb, lb + 1, seq.size()}) {
        good("lf " + std::to_string(n), seq.substr(0, n), lb, "\n", true);
        good("crlf " + std::to_string(n), seq.substr(0, n), lb, "\r\n", true);
        good("no final line end " + std::to_string(n), seq.substr(0, n), lb, "\n", false);
    }
    std::string all;
    for (int b = 0; b < 256; ++b)
        if (b != '\n' && b != '\r' && b != '>') all += (char)b;
    good("every byte", all, all.size(), "\n", true);
    const std::string lf = wrap(seq, lb, "\n", true);
    refused("line width too large", lf, lb, lb + 2, (int64_t)seq.size());
    refused("line width too small", wrap(seq, lb, "\r\n", true), lb, lb + 1, (int64_t)seq.size());
    refused("bytes end early", lf.substr(0, 120), lb, lb + 1, (int64_t)seq.size());
    refused("no bytes", "", lb, lb + 1, 1);
    refused("next record's header", "AC\n>x\nGG\n", 2, 3, 4);
    refused("zero line bases", "ACGT", 0, 1, 4);
    refused("line narrower than its bases", "ACGT", 4, 3, 4);
    refused("negative length", "ACGT", 4, 5, -1);
    if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
    printf("asan_cand_reference: ok\n");
    return 0;
}
