// C ABI of the zlib stream inflate (include/dl4vc_chunks.h): whole zlib streams in host memory, inflated by the text of
// zinflate.h on the CPU with one lane (zi_inflate_host) or by zi_inflate_kernel on the GPU (zi_inflate).  Every entry catches what
// it throws; a bad stream is a status.
//
// With -DZI_HOST_ONLY a plain C++ compiler builds the host entry alone (tools/asan_zinflate.sh runs it under sanitizers).
#ifdef ZI_HOST_ONLY
#include "capi_shell.h"
#include "zinflate.h"
#else
#include "device_buffer.h"
#include "zinflate_device.h"
#endif

#include <string>
#include <vector>

namespace {

thread_local std::string g_zi_err;

template <class... A>
int zi_fail(int code, const char* fmt, A... a) { return capi::failf(g_zi_err, code, fmt, a...); }

// the stream table of a call: input ranges checked against nbytes, slots against out_cap
int make_table(const char* who, const uint8_t* streams, uint64_t nbytes, const uint64_t* off, const uint64_t* len, int64_t n, uint8_t* out,
               uint64_t out_cap, const uint64_t* out_off, const uint64_t* out_len, const uint8_t* raw, int32_t* status,
               std::vector<zi::StreamDesc>& tab) {
    if (n < 0 || n > (int64_t)1 << 30) return zi_fail(-1, "%s: 0..2^30 streams in one call", who);
    if (n > 0 && (!off || !len || !out_off || !out_len || !status || (nbytes && !streams) || (out_cap && !out)))
        return zi_fail(-1, "%s: null argument", who);
    tab.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        zi::StreamDesc& d = tab[i];
        d = zi::StreamDesc{};
        d.raw = raw && raw[i] ? 1 : 0;
        if (off[i] > nbytes || nbytes - off[i] < len[i] || len[i] > 0xffffffffull) {
            d.status = ZI_BAD_RANGE;
        } else if (out_len[i] > zi::MAX_OUTPUT || out_off[i] > out_cap || out_cap - out_off[i] < out_len[i]) {
            d.status = ZI_BAD_SLOT;
        } else {
            d.in_off = off[i];
            d.out_off = out_off[i];
            d.in_len = (uint32_t)len[i];
            d.out_len = (uint32_t)out_len[i];
        }
    }
    return 0;
}

}  // namespace

extern "C" {

const char* zi_last_error(void) { return g_zi_err.c_str(); }

const char* zi_status_text(int status) {
    switch (status) {
        case ZI_OK: return "ok";
        case ZI_BAD_BLOCK_TYPE: return "bad block type";
        case ZI_BAD_STORED_LEN: return "bad stored length";
        case ZI_BAD_CODE_LENGTHS: return "bad code lengths";
        case ZI_BAD_SYMBOL: return "bad symbol";
        case ZI_DISTANCE_BEFORE_START: return "distance before start";
        case ZI_OUTPUT_EXCEEDS_LENGTH: return "the stream holds more than the expected bytes";
        case ZI_OUTPUT_SHORT_OF_LENGTH: return "the stream ends short of the expected bytes";
        case ZI_INPUT_EXHAUSTED: return "input exhausted";
        case ZI_TRAILING_INPUT: return "trailing input";
        case ZI_BAD_SLOT: return "output slot outside the buffer";
        case ZI_BAD_ZLIB_HEADER: return "not a zlib stream header";
        case ZI_ADLER_MISMATCH: return "Adler-32 mismatch";
        case ZI_RAW_SIZE_MISMATCH: return "raw chunk of the wrong size";
        case ZI_BAD_RANGE: return "stream outside the input";
        default: return "unknown status";
    }
}

int zi_inflate_host(const uint8_t* streams, uint64_t nbytes, const uint64_t* off, const uint64_t* len, int64_t n, uint8_t* out,
                    uint64_t out_cap, const uint64_t* out_off, const uint64_t* out_len, const uint8_t* raw, int32_t* status) {
    return capi::guarded(g_zi_err, "zi_inflate_host", [&] {
        std::vector<zi::StreamDesc> tab;
        const int rc = make_table("zi_inflate_host", streams, nbytes, off, len, n, out, out_cap, out_off, out_len, raw, status, tab);
        if (rc) return rc;
        std::vector<uint8_t> ring(zi::RING);
        std::vector<bz::Tables> t(1);
        uint32_t scratch[zi::OneLane::WIDTH];
        for (int64_t i = 0; i < n; ++i) status[i] = zi::run_stream(streams, tab[i], out, ring.data(), t[0], scratch, zi::OneLane{});
        return 0;
    });
}

#ifndef ZI_HOST_ONLY
int zi_inflate(const uint8_t* streams, uint64_t nbytes, const uint64_t* off, const uint64_t* len, int64_t n, uint8_t* out, uint64_t out_cap,
               const uint64_t* out_off, const uint64_t* out_len, const uint8_t* raw, int32_t* status, int device) {
    return capi::guarded(g_zi_err, "zi_inflate", [&] {
        std::vector<zi::StreamDesc> tab;
        const int rc = make_table("zi_inflate", streams, nbytes, off, len, n, out, out_cap, out_off, out_len, raw, status, tab);
        if (rc) return rc;
        if (n == 0) return 0;
#define ZI_TRY(x) DEV_TRY(g_zi_err, "zi_inflate: ", x)
        ZI_TRY(hipSetDevice(device));
        dev::Buffer d_comp, d_out;
        dev::Array<zi::StreamDesc> d_tab;
        dev::Array<int32_t> d_status;
        ZI_TRY(d_comp.alloc(nbytes + 16));
        ZI_TRY(d_tab.alloc(tab.size()));
        ZI_TRY(d_out.alloc(out_cap + 16));
        ZI_TRY(d_status.alloc((size_t)n));
        if (nbytes) ZI_TRY(hipMemcpy(d_comp.p, streams, nbytes, hipMemcpyHostToDevice));
        ZI_TRY(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(zi::StreamDesc), hipMemcpyHostToDevice));
        if (out_cap) ZI_TRY(hipMemcpy(d_out.p, out, out_cap, hipMemcpyHostToDevice));   // (what no slot covers comes back as it went)
        ZI_TRY(zi::launch_inflate(d_comp.p, d_tab.p, n, d_out.p, d_status.p, nullptr));
        ZI_TRY(hipDeviceSynchronize());
        if (out_cap) ZI_TRY(hipMemcpy(out, d_out.p, out_cap, hipMemcpyDeviceToHost));
        ZI_TRY(hipMemcpy(status, d_status.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
#undef ZI_TRY
        return 0;
    });
}
#endif

}  // extern "C"
