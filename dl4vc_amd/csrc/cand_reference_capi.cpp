// C ABI of the reference-base conversion (include/dl4vc_candgen.h): the raw bytes of one FASTA contig in host memory, converted
// by the loop over the rule of cand_reference.h on the CPU (cg_reference_codes_host) or by reference_codes_kernel on the GPU
// (cg_reference_codes), and of the left-alignment rule of cand_left_align.h for one observation on the CPU
// (cg_left_align_host).  Also the library's error text (cg_last_error), which cand_capi.cpp shares.  Every entry catches what it
// throws; an index that does not describe the bytes is an error code.
//
// With -DCG_REFERENCE_HOST_ONLY a plain C++ compiler builds the host entry alone (tools/asan_cand_reference.sh runs it under
// sanitizers).
#include "../../include/dl4vc_candgen.h"
#include "cand_left_align.h"
#include "cand_reference.h"
#include "capi_shell.h"
#ifndef CG_REFERENCE_HOST_ONLY
#include "cand_device.h"
#include "device_buffer.h"
#endif

#include <string>

namespace cand {
std::string& last_error() {
    thread_local std::string err;
    return err;
}
}  // namespace cand

namespace {

template <class... A>
int ref_fail(int code, const char* fmt, A... a) { return capi::failf(cand::last_error(), code, fmt, a...); }

int check_arguments(const char* who, const uint8_t* raw, uint64_t raw_len, int64_t lb, int64_t lw, int64_t length, const uint8_t* out,
                    const int64_t* n_other) {
    if (!n_other || (raw_len > 0 && !raw) || (length > 0 && !out)) return ref_fail(-1, "%s: null argument", who);
    if (!cand::refc::layout_ok(lb, lw, length))
        return ref_fail(-1, "%s: %lld bases on lines of %lld bases in %lld bytes is no FASTA layout", who, (long long)length, (long long)lb,
                        (long long)lw);
    return 0;
}

int broken(const char* who, uint64_t p, int64_t lb, int64_t lw) {
    return ref_fail(-3, "%s: a line end, '>' or the end of the bytes at base %llu: lines of %lld bases in %lld bytes do not describe them", who,
                    (unsigned long long)p, (long long)lb, (long long)lw);
}

}  // namespace

extern "C" {

const char* cg_last_error(void) { return cand::last_error().c_str(); }

int cg_reference_codes_host(const uint8_t* raw, uint64_t raw_len, int64_t linebases, int64_t linewidth, int64_t length, uint8_t* out,
                            int64_t* n_other) {
    return capi::guarded(cand::last_error(), "cg_reference_codes_host", [&] {
        if (const int rc = check_arguments("cg_reference_codes", raw, raw_len, linebases, linewidth, length, out, n_other)) return rc;
        const uint64_t bad = cand::refc::codes_host(raw, raw_len, linebases, linewidth, length, out, n_other);
        return bad == cand::refc::NONE ? 0 : broken("cg_reference_codes", bad, linebases, linewidth);
    });
}

int cg_left_align_host(const uint8_t* codes, int64_t length, int32_t kind, int32_t anchor_aligned, int64_t anchor_pos, int32_t anchor_code,
                       const uint8_t* bases, int32_t n_bases, int64_t floor, int64_t* pos_out, uint8_t* bases_out, int32_t* flags) {
    return capi::guarded(cand::last_error(), "cg_left_align_host", [&] {
        namespace L = cand::lal;
        if (!pos_out || !bases_out || !flags || (length > 0 && !codes) || (n_bases > 0 && !bases))
            return ref_fail(-1, "cg_left_align_host: null argument");
        if (length < 0 || n_bases < 0) return ref_fail(-1, "cg_left_align_host: negative length");
        *pos_out = anchor_pos;
        *flags = 0;
        bases_out[0] = (uint8_t)anchor_code;
        for (int32_t j = 0; j < n_bases; ++j) bases_out[j + 1] = bases[j];
        bool codes_ok = (anchor_code & ~0xf) == 0;
        for (int32_t j = 0; j < n_bases; ++j) codes_ok = codes_ok && bases[j] < 16;
        if (n_bases > L::MAX_L || !codes_ok) return 0;           // no key holds it: not eligible, returned as it came
        uint64_t w[4] = {0, 0, 0, 0};
        L::put_code(w, 0, anchor_code);
        for (int32_t j = 0; j < n_bases; ++j) L::put_code(w, j + 1, bases[j]);
        int fl = 0;
        const int64_t k = L::align(kind, anchor_aligned != 0, w, n_bases, codes, length, anchor_pos, floor, &fl);
        *pos_out = anchor_pos - k;
        *flags = fl;
        for (int32_t j = 0; j <= n_bases; ++j) bases_out[j] = (uint8_t)L::code_at(w, j);
        return 0;
    });
}

#ifndef CG_REFERENCE_HOST_ONLY
int cg_reference_codes(const uint8_t* raw, uint64_t raw_len, int64_t linebases, int64_t linewidth, int64_t length, uint8_t* out,
                       int64_t* n_other, int device) {
    return capi::guarded(cand::last_error(), "cg_reference_codes", [&] {
        if (const int rc = check_arguments("cg_reference_codes", raw, raw_len, linebases, linewidth, length, out, n_other)) return rc;
        *n_other = 0;
        if (length == 0) return 0;
#define CR_TRY(x) DEV_TRY(cand::last_error(), "cg_reference_codes: ", x)
        CR_TRY(hipSetDevice(device));
        dev::Buffer d_raw, d_out;
        dev::Array<unsigned long long> d_counts;
        CR_TRY(d_raw.alloc(raw_len + 16));
        CR_TRY(d_out.alloc((size_t)length + 16));
        CR_TRY(d_counts.alloc(2));
        const unsigned long long zero[2] = {0, cand::refc::NONE};
        unsigned long long counts[2];
        if (raw_len) CR_TRY(hipMemcpy(d_raw.p, raw, raw_len, hipMemcpyHostToDevice));
        CR_TRY(hipMemcpy(d_counts.p, zero, sizeof zero, hipMemcpyHostToDevice));
        CR_TRY(cand::launch_reference_codes(d_raw.p, raw_len, linebases, linewidth, length, d_out.p, d_counts.p, nullptr));
        CR_TRY(hipDeviceSynchronize());
        CR_TRY(hipMemcpy(counts, d_counts.p, sizeof counts, hipMemcpyDeviceToHost));
        if (counts[1] != cand::refc::NONE) return broken("cg_reference_codes", counts[1], linebases, linewidth);
        CR_TRY(hipMemcpy(out, d_out.p, (size_t)length, hipMemcpyDeviceToHost));
#undef CR_TRY
        *n_other = (int64_t)counts[0];
        return 0;
    });
}
#endif

}  // extern "C"
