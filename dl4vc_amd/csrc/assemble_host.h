// Host side of the site assembly (assemble_kernels.hip), shared by its two entries: pg_assemble_device (pileup_capi.cpp: the stored
// planes of the GPU pileup encoder, a slot = S * L bytes of one plane) and cl_assemble_device (chunk_capi.cpp: the planes inside
// the inflated records of a candidate file, a slot = one record).  Every index the kernel follows is checked here first.
#pragma once

#include "device_buffer.h"
#include "pileup_device.h"
#include "plan_entry.h"

#include <climits>
#include <cstring>
#include <string>

namespace pgh {

// What a handle keeps for assemble(): its error text and device, the site sources and rows (device), their pinned staging (+ the
// three [m][L] host planes), and the event after which the staging of the previous call may be overwritten.  A handle that
// derives from it waits in its own destructor too: its members go before these do.
struct AssembleState {
    std::string err;
    int32_t device = 0;
    dev::Buffer d_meta;
    dev::Pinned h_meta;
    dev::Event ev_meta; bool meta_busy = false;
    void wait_meta() {
        if (ev_meta && meta_busy) (void)hipEventSynchronize(ev_meta);
        meta_busy = false;
    }
    ~AssembleState() { wait_meta(); }
};

// src[plane] + slot * slot_stride is the [S][L] plane of a slot; `who` names the entry in the error texts.
inline int assemble(AssembleState* h, const char* who, const uint8_t* const src[3], int64_t slot_stride, int64_t n_slots, int32_t S,
                    int32_t L, const int32_t* slots, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t R,
                    const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                    uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                    uint8_t* var_mask_out, void* stream) {
    if (m < 0 || n_slots < 0 || S < 1 || L < 1 || R < 1) return capi::failf(h->err, -1, "%s: bad shape", who);
    if (R > S) return capi::failf(h->err, -1, "%s: %d rows per site but only %d are stored", who, R, S);
    if (S > INT16_MAX) return capi::failf(h->err, -1, "%s: %d stored rows do not fit the int16 row index", who, S);
    if (rows && S > plan_entry::MAX_STORED) return capi::failf(h->err, -1, "%s: %d stored rows do not fit a plan entry beside its zero-reads bit", who, S);
    if (m > INT32_MAX / 4 || (int64_t)R * L > INT32_MAX / 2) return capi::failf(h->err, -1, "%s: too large", who);
    if (slot_stride < (int64_t)S * L) return capi::failf(h->err, -1, "%s: a slot stride of %lld bytes is less than a plane", who, (long long)slot_stride);
    if (m == 0) return 0;
    if (!src[0] || !src[1] || !src[2] || !slots || !ref || !ref_mask || !var_mask || !reads_out || !qual_out || !strand_out || !ref_out ||
        !ref_mask_out || !var_mask_out)
        return capi::failf(h->err, -1, "%s: null argument", who);
    // every index the kernel follows is checked here: a slot or a row outside the stored planes never reaches the device
    bool any_rows = false;
    for (int64_t i = 0; i < m; ++i) {
        if (slots[i] < 0 || slots[i] >= n_slots) return capi::failf(h->err, -1, "%s: site %lld names slot %d of %lld", who, (long long)i, slots[i],
                                                              (long long)n_slots);
        if (rows && !(first_rows && first_rows[i])) {
            any_rows = true;
            const int16_t* r = rows + (size_t)i * R;
            for (int k = 0; k < R; ++k) {                   // (the zero-reads bit of an entry is not part of its row, plan_entry.h)
                const int row = plan_entry::stored_row(r[k]);
                if (row < 0 || row >= S) return capi::failf(h->err, -1, "%s: site %lld row %d names stored row %d of %d", who, (long long)i, k, row, S);
            }
        }
    }
    dev::DeviceGuard guard;
    if (hipSetDevice(h->device) != hipSuccess) return capi::failf(h->err, -2, "hipSetDevice(%d) failed", h->device);
    if (h->ev_meta.ensure(hipEventDisableTiming) != hipSuccess) return capi::failf(h->err, -2, "hipEventCreate failed");
    if (h->meta_busy) {                                  // the previous call's staging and device copies are still its own
        if (hipEventSynchronize(h->ev_meta) != hipSuccess) return capi::failf(h->err, -2, "hipEventSynchronize failed");
        h->meta_busy = false;
    }
    const size_t b_sites = (size_t)m * sizeof(pg::SiteSrc), b_rows = any_rows ? (size_t)m * R * sizeof(int16_t) : 0;
    const size_t b_dev = b_sites + b_rows, b_line = (size_t)m * L;
    if (h->d_meta.ensure(b_dev) != hipSuccess) return capi::failf(h->err, -2, "hipMalloc of the assembly table failed");
    if (h->h_meta.ensure(b_dev + 3 * b_line) != hipSuccess) return capi::failf(h->err, -2, "hipHostMalloc of the assembly staging failed");
    pg::SiteSrc* hs = (pg::SiteSrc*)h->h_meta.p;
    for (int64_t i = 0; i < m; ++i) hs[i] = pg::SiteSrc{slots[i], (!rows || (first_rows && first_rows[i])) ? 1 : 0};
    if (b_rows) memcpy(h->h_meta.p + b_sites, rows, b_rows);
    uint8_t* lines = h->h_meta.p + b_dev;
    memcpy(lines, ref, b_line); memcpy(lines + b_line, ref_mask, b_line); memcpy(lines + 2 * b_line, var_mask, b_line);
    hipStream_t s = (hipStream_t)stream;
    hipError_t rc = hipMemcpyAsync(h->d_meta.p, h->h_meta.p, b_dev, hipMemcpyHostToDevice, s);
    uint8_t* line_out[3] = {ref_out, ref_mask_out, var_mask_out};
    for (int c = 0; c < 3 && rc == hipSuccess; ++c)
        rc = hipMemcpyAsync(line_out[c], lines + c * b_line, b_line, hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) {
        pg::AssembleArgs a{};
        a.src[0] = src[0]; a.src[1] = src[1]; a.src[2] = src[2];
        a.dst[0] = reads_out; a.dst[1] = qual_out; a.dst[2] = strand_out;
        a.sites = (const pg::SiteSrc*)h->d_meta.p;
        a.rows = (const int16_t*)(h->d_meta.p + b_sites);
        a.slot_stride = slot_stride;
        a.S = S; a.R = R; a.L = L;
        a.use[0] = 1; a.use[1] = use_q != 0; a.use[2] = use_strand != 0;
        rc = pg::launch_assemble(a, (int32_t)m, s);
    }
    h->meta_busy = true;                                 // (also after a failure: some of the copies may be enqueued)
    if (hipEventRecord(h->ev_meta, s) != hipSuccess && rc == hipSuccess) rc = hipErrorUnknown;
    if (rc != hipSuccess) return capi::failf(h->err, -2, "device: %s", hipGetErrorString(rc));
    return 0;
}

}  // namespace pgh
