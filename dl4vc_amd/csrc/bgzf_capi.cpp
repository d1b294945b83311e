// C ABI of the BGZF inflate (include/dl4vc_bgzf.h): whole BGZF blocks in host memory, inflated by the decode core of
// bgzf_inflate.h on the CPU (bz_inflate_host) or by bgzf_inflate_kernel on the GPU (bz_inflate).  Every entry catches what it
// throws; a bad block is a status.
//
// With -DBZ_HOST_ONLY a plain C++ compiler builds the host entry alone (tools/asan_bgzf.sh runs it under sanitizers).
#ifdef BZ_HOST_ONLY
#include "bgzf_inflate.h"
#include "capi_shell.h"
#else
#include "bgzf_device.h"
#endif

#include <string>
#include <vector>

namespace {

thread_local std::string g_bz_err;

template <class... A>
int bz_fail(int code, const char* fmt, A... a) { return capi::failf(g_bz_err, code, fmt, a...); }

// the block table of a call: headers and trailers validated, slots checked against out_cap
int make_table(const uint8_t* blocks, uint64_t nbytes, const uint64_t* block_off, int64_t n, uint64_t out_cap, const uint64_t* out_off,
               std::vector<bz::BlockDesc>& tab) {
    if (n < 0 || (n > 0 && (!blocks || !block_off || !out_off))) return bz_fail(-1, "bz_inflate: null argument");
    tab.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        uint32_t bsize = 0;
        bz::parse_block(blocks, nbytes, block_off[i], tab[i], &bsize);
        tab[i].out_off = out_off[i];
        if (tab[i].status == BZ_OK && (out_off[i] > out_cap || out_cap - out_off[i] < tab[i].isize)) tab[i].status = BZ_BAD_SLOT;
    }
    return 0;
}

}  // namespace

extern "C" {

const char* bz_last_error(void) { return g_bz_err.c_str(); }

const char* bz_status_text(int status) {
    switch (status) {
        case BZ_OK: return "ok";
        case BZ_BAD_BLOCK_TYPE: return "bad block type";
        case BZ_BAD_STORED_LEN: return "bad stored length";
        case BZ_BAD_CODE_LENGTHS: return "bad code lengths";
        case BZ_BAD_SYMBOL: return "bad symbol";
        case BZ_DISTANCE_BEFORE_START: return "distance before start";
        case BZ_OUTPUT_EXCEEDS_ISIZE: return "output exceeds ISIZE";
        case BZ_OUTPUT_SHORT_OF_ISIZE: return "output short of ISIZE";
        case BZ_INPUT_EXHAUSTED: return "input exhausted";
        case BZ_TRAILING_INPUT: return "trailing input";
        case BZ_CRC_MISMATCH: return "CRC mismatch";
        case BZ_BAD_HEADER: return "not a BGZF block";
        case BZ_BAD_SLOT: return "output slot outside the buffer";
        default: return "unknown status";
    }
}

int bz_inflate_host(const uint8_t* blocks, uint64_t nbytes, const uint64_t* block_off, int64_t n_blocks, uint8_t* out, uint64_t out_cap,
                    const uint64_t* out_off, int32_t* status) {
    return capi::guarded(g_bz_err, "bz_inflate_host", [&] {
        if (n_blocks > 0 && (!out || !status)) return bz_fail(-1, "bz_inflate_host: null argument");
        std::vector<bz::BlockDesc> tab;
        const int rc = make_table(blocks, nbytes, block_off, n_blocks, out_cap, out_off, tab);
        if (rc) return rc;
        uint32_t table[256];
        for (uint32_t i = 0; i < 256; ++i) table[i] = bz::crc_table_entry(i);
        std::vector<bz::Tables> t(1);
        for (int64_t i = 0; i < n_blocks; ++i) status[i] = bz::inflate_block_host(blocks, tab[i], out, t[0], table);
        return 0;
    });
}

#ifndef BZ_HOST_ONLY
int bz_inflate(const uint8_t* blocks, uint64_t nbytes, const uint64_t* block_off, int64_t n_blocks, uint8_t* out, uint64_t out_cap,
               const uint64_t* out_off, int32_t* status, int device) {
    return capi::guarded(g_bz_err, "bz_inflate", [&] {
        if (n_blocks > 0 && (!out || !status)) return bz_fail(-1, "bz_inflate: null argument");
        if (n_blocks > (int64_t)1 << 30) return bz_fail(-1, "bz_inflate: too many blocks in one call");
        std::vector<bz::BlockDesc> tab;
        const int rc = make_table(blocks, nbytes, block_off, n_blocks, out_cap, out_off, tab);
        if (rc) return rc;
        if (n_blocks == 0) return 0;
#define BZ_TRY(x) DEV_TRY(g_bz_err, "bz_inflate: ", x)
        BZ_TRY(hipSetDevice(device));
        dev::Buffer d_comp, d_out;
        dev::Array<bz::BlockDesc> d_tab;
        dev::Array<int32_t> d_status;
        BZ_TRY(d_comp.alloc(nbytes + 16));
        BZ_TRY(d_tab.alloc(tab.size()));
        BZ_TRY(d_out.alloc(out_cap + 16));
        BZ_TRY(d_status.alloc((size_t)n_blocks));
        BZ_TRY(hipMemcpy(d_comp.p, blocks, nbytes, hipMemcpyHostToDevice));
        BZ_TRY(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(bz::BlockDesc), hipMemcpyHostToDevice));
        if (out_cap) BZ_TRY(hipMemcpy(d_out.p, out, out_cap, hipMemcpyHostToDevice));   // (what no slot covers comes back as it went)
        BZ_TRY(bz::launch_inflate(d_comp.p, d_tab.p, n_blocks, d_out.p, d_status.p, nullptr));
        BZ_TRY(hipDeviceSynchronize());
        if (out_cap) BZ_TRY(hipMemcpy(out, d_out.p, out_cap, hipMemcpyDeviceToHost));
        BZ_TRY(hipMemcpy(status, d_status.p, (size_t)n_blocks * sizeof(int32_t), hipMemcpyDeviceToHost));
#undef BZ_TRY
        return 0;
    });
}
#endif

}  // extern "C"
