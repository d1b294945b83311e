// zd_* of libdl4vc_pileup.so (include/dl4vc_pileup_gpu.h): the compressor's size bound, its host form (the text of zdeflate.h,
// serially) and its device form over caller-supplied device buffers.  With -DZD_HOST_ONLY the file compiles with a plain C++
// compiler into the host entries alone (tools/asan_zdeflate.sh).  Errors go to the text pg_last_error(NULL) returns.
#include "../../include/dl4vc_pileup_gpu.h"
#include "capi_shell.h"
#include "zdeflate.h"

#include <mutex>
#include <string>
#include <vector>

namespace pgh {
extern std::string g_err __attribute__((visibility("hidden")));
}
#ifdef ZD_HOST_ONLY
std::string pgh::g_err;
#else
#include "zdeflate_device.h"
#endif

namespace {

template <class... A>
int zfail(int code, const char* fmt, A... a) { return capi::failf(pgh::g_err, code, fmt, a...); }

bool seg_ok(uint32_t seg) { return seg >= zd::MIN_SEG && seg <= zd::MAX_SEG; }

int deflate_host(const char* who, const uint8_t* in, uint64_t n, uint32_t segment, int32_t flags, uint8_t* out, uint64_t out_cap,
                 uint64_t* size, uint32_t* adler, int32_t* store) {
    return capi::guarded(pgh::g_err, who, [&] {
        if ((n && !in) || !out || !size || !adler || !store) return zfail(-1, "%s: null argument", who);
        if (!seg_ok(segment)) return zfail(-1, "%s: segment must be 1024..32768 bytes", who);
        if (n > zd::MAX_STREAM) return zfail(-1, "%s: more than 2^31 bytes in one stream", who);
        if (out_cap < zd::bound(n, segment)) return zfail(-1, "%s: the output buffer is smaller than zd_bound", who);
        const uint64_t ns = zd::n_segments(n, segment);
        std::vector<uint32_t> sizes(ns), adlers(ns);
        std::vector<uint64_t> offs(ns);
        std::vector<uint16_t> head(zd::HASH_SIZE);
        std::vector<uint32_t> work(flags & ZD_DYNAMIC ? zd::WORK_SIZE : 0), build(flags & ZD_DYNAMIC ? zd::BUILD_SIZE : 0);
        // the segments land where the device's gather puts them: one behind the other after the 2-byte header
        uint64_t at = 2;
        for (uint64_t k = 0; k < ns; ++k) {
            const uint32_t len = (uint32_t)(k + 1 < ns ? segment : n - k * segment);
            const uint8_t* src = in + k * segment;
            int kind = 0;
            adlers[k] = zd::adler32(src, len);
            sizes[k] = flags & ZD_DYNAMIC                  // (at + seg_cap(len) + 4 <= bound)
                           ? zd::deflate_segment_dynamic(src, len, k + 1 == ns, out + at, head.data(), 1, work.data(), 1, build.data(), &kind)
                           : zd::deflate_segment(src, len, k + 1 == ns, out + at, head.data(), 1);
            at += sizes[k];
        }
        const zd::StreamInfo r = zd::finish_stream(n, segment, sizes.data(), adlers.data(), offs.data());
        out[0] = zd::ZLIB_CMF;
        out[1] = zd::ZLIB_FLG;
        for (int b = 0; b < 4; ++b) out[at + b] = (uint8_t)(r.adler >> (8 * (3 - b)));
        *size = r.size;
        *adler = r.adler;
        *store = (int32_t)r.store;
        return 0;
    });
}

}  // namespace

extern "C" {

int zd_bound(uint64_t n, uint32_t segment, uint64_t* bound) {
    if (!bound) return zfail(-1, "zd_bound: null argument");
    if (!seg_ok(segment)) return zfail(-1, "zd_bound: segment must be 1024..32768 bytes");
    if (n > zd::MAX_STREAM) return zfail(-1, "zd_bound: more than 2^31 bytes in one stream");
    *bound = zd::bound(n, segment);
    return 0;
}

int zd_deflate_host(const uint8_t* in, uint64_t n, uint32_t segment, uint8_t* out, uint64_t out_cap, uint64_t* size, uint32_t* adler,
                    int32_t* store) {
    return deflate_host("zd_deflate_host", in, n, segment, 0, out, out_cap, size, adler, store);
}

int zd_deflate_host_flags(const uint8_t* in, uint64_t n, uint32_t segment, int32_t flags, uint8_t* out, uint64_t out_cap, uint64_t* size,
                          uint32_t* adler, int32_t* store) {
    if (flags & ~ZD_DYNAMIC) return zfail(-1, "zd_deflate_host_flags: the only flag of the host form is ZD_DYNAMIC");
    return deflate_host("zd_deflate_host_flags", in, n, segment, flags, out, out_cap, size, adler, store);
}

int zd_code_lengths_host(const uint32_t* freq, int32_t n, int32_t limit, uint8_t* lens) {
    return capi::guarded(pgh::g_err, "zd_code_lengths_host", [&] {
        if (!freq || !lens) return zfail(-1, "zd_code_lengths_host: null argument");
        if (n < 2 || n > (int32_t)zd::N_LL || limit < 1 || limit > zd::MAX_BITS || (n > 2 && (1 << limit) < n))
            return zfail(-1, "zd_code_lengths_host: 2..286 symbols, a limit of 1..15 bits that holds them");
        uint64_t sum = 0;
        for (int32_t s = 0; s < n; ++s) sum += freq[s];
        if (sum > 65535) return zfail(-1, "zd_code_lengths_host: the counts add up to more than 65535");
        std::vector<uint32_t> t(freq, freq + n), build(zd::BUILD_SIZE);
        zd::code_lengths(t.data(), 1, (uint32_t)n, limit, build.data());
        for (int32_t s = 0; s < n; ++s) lens[s] = (uint8_t)t[s];
        return 0;
    });
}

#ifndef ZD_HOST_ONLY
int zd_deflate(const uint8_t* in_dev, uint64_t chunk_bytes, int64_t n_chunks, uint32_t segment, int32_t flags, uint8_t* out_dev,
               uint64_t out_cap, uint64_t* offsets, uint64_t* sizes, uint32_t* adlers, uint8_t* store, void* stream) {
    static std::mutex mu;
    static zd::Ctx* ctx = nullptr;             // (a test entry: one set of work buffers per process, kept)
    return capi::guarded(pgh::g_err, "zd_deflate", [&] {
        if (!in_dev || !out_dev || !offsets || !sizes || !adlers || !store) return zfail(-1, "zd_deflate: null argument");
        if (!seg_ok(segment)) return zfail(-1, "zd_deflate: segment must be 1024..32768 bytes");
        if (chunk_bytes > zd::MAX_STREAM || n_chunks < 1 || n_chunks > 65535) return zfail(-1, "zd_deflate: 1..65535 chunks of at most 2^31 bytes");
        if (flags & ~7) return zfail(-1, "zd_deflate: flags are ZD_REVERSED | ZD_RAW_ON_STORE | ZD_DYNAMIC");
        if (out_cap / (uint64_t)n_chunks < zd::bound(chunk_bytes, segment)) return zfail(-1, "zd_deflate: the output buffer is smaller than n_chunks * zd_bound");
        std::lock_guard<std::mutex> lk(mu);
        if (!ctx) ctx = zd::ctx_create();
        hipStream_t s = (hipStream_t)stream;
        zd::Streams r{};
        const char* msg = nullptr;
        if (zd::run(ctx, in_dev, chunk_bytes, n_chunks, segment, flags & ZD_REVERSED, flags & ZD_RAW_ON_STORE, flags & ZD_DYNAMIC, out_dev, s, nullptr,
                    &r, &msg))
            return zfail(-2, "zd_deflate: %s", msg);
        hipError_t e = hipMemcpyAsync(offsets, r.offs, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sizes, r.sizes, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(adlers, r.adlers, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(store, r.store, (size_t)n_chunks, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return zfail(-2, "zd_deflate: device: %s", hipGetErrorString(e));
        return 0;
    });
}
#endif

}  // extern "C"
