// cl_* of libdl4vc_pileup.so (include/dl4vc_chunks.h): the raw chunks of a candidate file, read by the caller, are uploaded and
// inflated on the device (zinflate_kernels.hip) into a buffer of records the handle owns; the members outside the three planes
// come back to pinned host memory in two pitched copies per call, and the sites are assembled from the planes where they lie
// inside the records (assemble_kernels.hip with the record size as the slot stride).  Every extern "C" body catches what it
// throws; a damaged chunk is a status.
#include "assemble_host.h"
#include "chunk_view.h"
#include "zinflate_device.h"

#include <vector>

struct cl_loader : pgh::AssembleState {
    int64_t record_bytes = 0, max_chunks = 0, plane = 0, blob_bytes = 0;
    int32_t chunk_records = 0, window = 0, stored_rows = 0;
    int64_t plane_off[3] = {0, 0, 0};
    int64_t span0 = 0, span1_off = 0, span1 = 0;      // the non-plane members: [0, span0) and [span1_off, span1_off + span1)
    int64_t n_records = 0;                            // of the last cl_inflate_chunks_device call
    dev::Buffer d_comp, d_records;
    dev::Array<zi::StreamDesc> d_tab;
    dev::Array<int32_t> d_status;
    dev::Pinned h_tab;                                // the table, then the statuses
    dev::Pinned h_blob;
    dev::Event ev[6];                                 // upload | inflate | copy back | ; assemble
    bool assemble_timed = false;
    cl_stats st{};
    ~cl_loader() { wait_meta(); }                     // (the last assembly may still be reading the records)
};

// what the record store (store_capi.cpp) reads of a loader: the records of its last cl_inflate_chunks_device call
clh::RecordsView clh::records_view(const cl_loader* h) {
    RecordsView v{};
    v.records = h->d_records.p; v.record_bytes = h->record_bytes; v.n_records = h->n_records;
    for (int k = 0; k < 3; ++k) v.plane_off[k] = h->plane_off[k];
    v.window = h->window; v.stored_rows = h->stored_rows; v.device = h->device;
    return v;
}

namespace {

std::string g_cl_err;

template <class... A>
int cfail(cl_loader* h, int code, const char* fmt, A... a) { return capi::failf(h ? h->err : g_cl_err, code, fmt, a...); }

#define CL_TRY(x) DEV_TRY(h->err, "", x)

int open_loader(cl_loader* h, int64_t max_records) {
    const int64_t SL = h->plane, W = h->window, rb = h->record_bytes;
    const int64_t* p = h->plane_off;
    // the packed record of hdf5_schema.record_dtype: 16 + 15 W bytes, reads, W + 133 bytes, quality, strand
    if (p[0] != 16 + 15 * W || p[1] != p[0] + SL + W + 133 || p[2] != p[1] + SL || rb != p[2] + SL)
        return cfail(h, -1, "cl_open: planes at %lld / %lld / %lld of a %lld-byte record are not the candidate record's layout at %d rows "
                            "of %d columns", (long long)p[0], (long long)p[1], (long long)p[2], (long long)rb, h->stored_rows, h->window);
    h->span0 = p[0]; h->span1_off = p[0] + SL; h->span1 = W + 133;
    h->blob_bytes = h->span0 + h->span1;
    const uint64_t chunk_bytes = (uint64_t)rb * h->chunk_records;
    if (chunk_bytes > zi::MAX_OUTPUT) return cfail(h, -1, "cl_open: a chunk of %llu bytes is more than one stream may hold", (unsigned long long)chunk_bytes);
    h->max_chunks = (max_records + h->chunk_records - 1) / h->chunk_records + 1;
    if (h->max_chunks * h->chunk_records > INT32_MAX / 2) return cfail(h, -1, "cl_open: too many records per call");
    CL_TRY(hipSetDevice(h->device));
    CL_TRY(h->d_records.alloc((size_t)h->max_chunks * chunk_bytes + 16));
    CL_TRY(h->d_tab.alloc((size_t)h->max_chunks));
    CL_TRY(h->d_status.alloc((size_t)h->max_chunks));
    CL_TRY(h->h_tab.alloc((size_t)h->max_chunks * (sizeof(zi::StreamDesc) + sizeof(int32_t))));
    CL_TRY(h->h_blob.alloc((size_t)h->max_chunks * h->chunk_records * h->blob_bytes + 16));
    // blocking-sync events: the thread that waits for an inflate (tens of ms for a chunk of a megabyte) sleeps instead of spinning
    for (dev::Event& e : h->ev) CL_TRY(e.ensure(hipEventBlockingSync));
    return 0;
}

int inflate_chunks(cl_loader* h, const uint8_t* comp, uint64_t nbytes, const uint64_t* off, const uint64_t* len, const uint8_t* raw,
                   int64_t n, void* stream, const uint8_t** blob, int32_t* status) {
    if (n < 0 || n > h->max_chunks) return cfail(h, -1, "cl_inflate_chunks_device: %lld chunks, the handle was opened for %lld",
                                                 (long long)n, (long long)h->max_chunks);
    if (!blob || (n > 0 && (!comp || !off || !len || !status))) return cfail(h, -1, "cl_inflate_chunks_device: null argument");
    *blob = h->h_blob.p;
    h->st = cl_stats{};
    h->assemble_timed = false;
    h->n_records = 0;
    if (n == 0) return 0;
    const uint64_t chunk_bytes = (uint64_t)h->record_bytes * h->chunk_records;
    zi::StreamDesc* tab = (zi::StreamDesc*)h->h_tab.p;
    int32_t* h_status = (int32_t*)(h->h_tab.p + (size_t)h->max_chunks * sizeof(zi::StreamDesc));
    for (int64_t c = 0; c < n; ++c) {
        zi::StreamDesc d{};
        d.raw = raw && raw[c] ? 1 : 0;
        if (off[c] > nbytes || nbytes - off[c] < len[c] || len[c] > 0xffffffffull) d.status = ZI_BAD_RANGE;
        else { d.in_off = off[c]; d.in_len = (uint32_t)len[c]; d.out_off = (uint64_t)c * chunk_bytes; d.out_len = (uint32_t)chunk_bytes; }
        tab[c] = d;
        h->st.compressed_bytes += (int64_t)len[c];
        h->st.raw_chunks += d.raw;
    }
    CL_TRY(hipSetDevice(h->device));
    if (h->d_comp.ensure((size_t)nbytes + 16) != hipSuccess) return cfail(h, -2, "hipMalloc of the chunk buffer failed");
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_rec = n * h->chunk_records;
    CL_TRY(hipEventRecord(h->ev[0], s));
    CL_TRY(hipMemcpyAsync(h->d_comp.p, comp, nbytes, hipMemcpyHostToDevice, s));
    CL_TRY(hipMemcpyAsync(h->d_tab.p, tab, (size_t)n * sizeof(zi::StreamDesc), hipMemcpyHostToDevice, s));
    CL_TRY(hipEventRecord(h->ev[1], s));
    CL_TRY(zi::launch_inflate(h->d_comp.p, h->d_tab.p, n, h->d_records.p, h->d_status.p, s));
    CL_TRY(hipEventRecord(h->ev[2], s));
    // two spans per record: device pitch = the record, host pitch = the blob
    CL_TRY(hipMemcpy2DAsync(h->h_blob.p, (size_t)h->blob_bytes, h->d_records.p, (size_t)h->record_bytes, (size_t)h->span0, (size_t)n_rec,
                            hipMemcpyDeviceToHost, s));
    CL_TRY(hipMemcpy2DAsync(h->h_blob.p + h->span0, (size_t)h->blob_bytes, h->d_records.p + h->span1_off, (size_t)h->record_bytes,
                            (size_t)h->span1, (size_t)n_rec, hipMemcpyDeviceToHost, s));
    CL_TRY(hipMemcpyAsync(h_status, h->d_status.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    CL_TRY(hipEventRecord(h->ev[3], s));
    CL_TRY(hipEventSynchronize(h->ev[3]));               // (everything of this call on `s` lies in front of the event)
    float ms[3] = {0, 0, 0};
    for (int k = 0; k < 3; ++k) CL_TRY(hipEventElapsedTime(&ms[k], h->ev[k], h->ev[k + 1]));
    h->st.upload_ms = ms[0]; h->st.inflate_ms = ms[1]; h->st.blob_copy_back_ms = ms[2];
    h->st.chunks = n;
    h->st.inflated_bytes = (int64_t)(n * chunk_bytes);
    memcpy(status, h_status, (size_t)n * sizeof(int32_t));
    h->n_records = n_rec;
    return 0;
}

// What both cl_center_counts_* entries refuse: 0 = fine.
int counts_arguments(cl_loader* h, const char* who, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, const int32_t* counts) {
    if (m < 0 || m > INT32_MAX || rows < 1 || window < 3) return cfail(h, -1, "%s: bad shape", who);
    if (m > 0 && (!reads || !counts)) return cfail(h, -1, "%s: null argument", who);
    return 0;
}

}  // namespace

extern "C" {

const char* cl_last_error(const cl_loader_t* h) { return h ? h->err.c_str() : g_cl_err.c_str(); }

int cl_open(int64_t record_bytes, int32_t chunk_records, int32_t window, int32_t stored_rows, const int64_t* plane_off, int64_t max_records,
            int32_t device, cl_loader_t** out) {
    if (!out || !plane_off) return cfail(nullptr, -1, "cl_open: null argument");
    *out = nullptr;
    if (record_bytes < 1 || chunk_records < 1 || window < 1 || stored_rows < 1 || stored_rows > INT16_MAX || max_records < 1 ||
        (int64_t)window * stored_rows > (1 << 24))
        return cfail(nullptr, -1, "cl_open: bad shape");
    return capi::guarded(g_cl_err, "cl_open", [&] {
        cl_loader* h = new cl_loader();
        h->record_bytes = record_bytes; h->chunk_records = chunk_records; h->window = window; h->stored_rows = stored_rows;
        h->plane = (int64_t)window * stored_rows;
        h->device = device;
        for (int k = 0; k < 3; ++k) h->plane_off[k] = plane_off[k];
        const int rc = open_loader(h, max_records);
        if (rc) {
            g_cl_err = h->err;
            delete h;
            return rc;
        }
        *out = h;
        return 0;
    });
}

void cl_close(cl_loader_t* h) {
    try {
        if (h) (void)hipSetDevice(h->device);
        delete h;
    } catch (...) {
    }
}

int cl_inflate_chunks_device(cl_loader_t* h, const uint8_t* comp, uint64_t nbytes, const uint64_t* off, const uint64_t* len,
                             const uint8_t* raw, int64_t n_chunks, void* stream, const uint8_t** blob, int32_t* status) {
    if (!h) return cfail(nullptr, -1, "cl_inflate_chunks_device: null handle");
    return capi::guarded(h->err, "cl_inflate_chunks_device", [&] {
        return inflate_chunks(h, comp, nbytes, off, len, raw, n_chunks, stream, blob, status);
    });
}

int cl_assemble_device(cl_loader_t* h, const int32_t* slots, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t reads,
                       const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                       uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                       uint8_t* var_mask_out, void* stream) {
    if (!h) return cfail(nullptr, -1, "cl_assemble_device: null handle");
    return capi::guarded(h->err, "cl_assemble_device", [&] {
        const uint8_t* src[3] = {h->d_records.p + h->plane_off[0], h->d_records.p + h->plane_off[1], h->d_records.p + h->plane_off[2]};
        hipStream_t s = (hipStream_t)stream;
        const bool timed = m > 0 && hipEventRecord(h->ev[4], s) == hipSuccess;
        const int rc = pgh::assemble(h, "cl_assemble_device", src, h->record_bytes, h->n_records, h->stored_rows, h->window, slots, rows,
                                     first_rows, m, reads, ref, ref_mask, var_mask, use_q, use_strand, reads_out, qual_out, strand_out,
                                     ref_out, ref_mask_out, var_mask_out, stream);
        h->assemble_timed = rc == 0 && timed && hipEventRecord(h->ev[5], s) == hipSuccess;
        return rc;
    });
}

int cl_center_counts_device(cl_loader_t* h, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, int32_t* counts, void* stream) {
    if (!h) return cfail(nullptr, -1, "cl_center_counts_device: null handle");
    return capi::guarded(h->err, "cl_center_counts_device", [&] {
        if (const int rc = counts_arguments(h, "cl_center_counts_device", reads, m, rows, window, counts)) return rc;
        CL_TRY(hipSetDevice(h->device));
        CL_TRY(pg::launch_center_counts(reads, m, rows, window, (window - 1) / 2, counts, (hipStream_t)stream));
        return 0;
    });
}

int cl_center_counts_host(cl_loader_t* h, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, int32_t* counts, void* stream) {
    (void)stream;
    if (const int rc = counts_arguments(h, "cl_center_counts_host", reads, m, rows, window, counts)) return rc;
    const int64_t col = (window - 1) / 2;
    for (int64_t i = 0; i < m; ++i) {
        int32_t* c = counts + i * 2 * pg::COUNT_TOKENS;
        for (int k = 0; k < 2 * pg::COUNT_TOKENS; ++k) c[k] = 0;
        const uint8_t* site = reads + (size_t)i * rows * window + col;
        for (int32_t r = 0; r < rows; ++r)
            for (int k = 0; k < 2; ++k) {
                const uint8_t t = site[(size_t)r * window + k];
                if (t < pg::COUNT_TOKENS) ++c[k * pg::COUNT_TOKENS + t];
            }
    }
    return 0;
}

int cl_get_stats(cl_loader_t* h, cl_stats* out) {
    if (!h || !out) return cfail(nullptr, -1, "cl_get_stats: null argument");
    if (h->assemble_timed) {
        float ms = 0;
        if (hipEventSynchronize(h->ev[5]) == hipSuccess && hipEventElapsedTime(&ms, h->ev[4], h->ev[5]) == hipSuccess) h->st.assemble_ms = ms;
        h->assemble_timed = false;
    }
    *out = h->st;
    return 0;
}

}  // extern "C"
