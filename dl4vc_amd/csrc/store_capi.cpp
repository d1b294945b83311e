// cl_store_* of libdl4vc_pileup.so (include/dl4vc_chunks.h): the record store.  The records a cl_loader handle inflated (or the
// slots of the pileup encoder's three plane arrays, cl_store_append_planes_device: the same kernels, another address rule) are
// measured (record_extent), laid out on the host (store_host.h: record order, 16-byte boundaries, slabs no record straddles, the
// capacity checked before anything is packed), packed into device slabs (store_pack) and from then on assembled from there
// (store_assemble) -- the file is inflated once per run, not once per epoch.  A store opened with device < 0 keeps its slabs in
// host memory and takes the CPU twins of the three kernels (cl_store_pack_host, cl_store_assemble_host): the definitions the
// kernels are tested against.  Every extern "C" body catches what it throws; every index is checked before it is followed.
//
// cl_store_set_format(h, 1) before the first append chooses the compact format of store_host.h: record_spans instead of
// record_extent (kept, cells and the mergeable flag come back and are checked before they size anything; the rows' spans stay in
// device scratch), the layout by each record's own span, store_pack_compact for the mergeable records and store_pack for the
// others in the same append, and the assembly by each record's format.  A host store takes the CPU twins of all of them.
//
// With -DCL_STORE_HOST_ONLY a plain C++ compiler builds the host store alone (tools/asan_store.sh runs it under sanitizers).
#include "../../include/dl4vc_chunks.h"
#include "store_host.h"

#ifdef CL_STORE_HOST_ONLY
#include "capi_shell.h"
#else
#include "assemble_host.h"
#include "chunk_view.h"
#include "store_device.h"
#endif

#include <algorithm>
#include <climits>
#include <memory>
#include <string>
#include <vector>

namespace {

struct Slab {
    uint64_t cap = 0, used = 0;
    std::unique_ptr<uint8_t[]> host;                  // a host store's slab: cap bytes
#ifndef CL_STORE_HOST_ONLY
    dev::Buffer d;                                    // a device store's: SLAB_GUARD | cap | SLAB_PAD
#endif
    uint8_t* data = nullptr;                          // the first of the cap bytes
};

struct Rec {
    int32_t slab = 0, kept = -1;                      // kept < 0: not appended yet
    uint64_t off = 0;
    int32_t format = st::FORMAT_ROWS;                 // the layout of its bytes (a compact store's records that are not mergeable: rows)
    uint64_t bytes = 0;                               // its span in the slab
};

// what an append knows of its records once they are measured
struct Measured {
    std::vector<int32_t> format, cells;
    std::vector<uint64_t> span;
    void resize(size_t n) { format.assign(n, st::FORMAT_ROWS); cells.assign(n, 0); span.assign(n, 0); }
};

#ifdef CL_STORE_HOST_ONLY
struct StoreBase {
    std::string err;
    int32_t device = -1;
};
#else
typedef pgh::AssembleState StoreBase;
#endif

}  // namespace

struct cl_store : StoreBase {
    int32_t window = 0, stored_rows = 0;
    int64_t n_records = 0;
    uint64_t capacity = 0, slab_bytes = 0;
    bool on_host = false;
    int fill = -1;                                    // >= 0: every new slab's allocation is filled with this byte first
    int32_t format = st::FORMAT_ROWS;                 // cl_store_set_format: what a mergeable record is stored as
    cl_store_format_stats fstats{};
    st::Cursor cur;
    std::vector<std::unique_ptr<Slab>> slabs;
    std::vector<Rec> table;
    cl_store_stats stats{};
#ifndef CL_STORE_HOST_ONLY
    dev::Array<st::DevRec> d_table;
    dev::Buffer d_app;                                // an append's slots, extents (or span sums and row spans) and pack items
    dev::Pinned h_app;
    dev::Event ev[6];                                 // extent or spans | copy back ; pack | ; assemble |
    bool assemble_timed = false;
    ~cl_store() { wait_meta(); }
#endif
};

namespace {

std::string g_store_err;

template <class... A>
int sfail(cl_store* h, int code, const char* fmt, A... a) { return capi::failf(h ? h->err : g_store_err, code, fmt, a...); }

// the planes of a record lie inside it
bool planes_inside(const int64_t* plane_off, int64_t record_bytes, int64_t plane) {
    for (int p = 0; p < 3; ++p)
        if (plane_off[p] < 0 || plane_off[p] > record_bytes - plane) return false;
    return true;
}

// What both append entries check of the records they are given: 0 = fine.
int check_append(cl_store* h, const char* who, const int32_t* slots, const int32_t* records, int64_t n, int64_t n_slots, int32_t* kept_out) {
    if (n < 0 || n > INT32_MAX / 4) return sfail(h, -1, "%s: bad record count", who);
    if (n > 0 && (!slots || !records || !kept_out)) return sfail(h, -1, "%s: null argument", who);
    for (int64_t i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= n_slots) return sfail(h, -1, "%s: entry %lld names slot %d of %lld", who, (long long)i, slots[i],
                                                          (long long)n_slots);
        if (records[i] < 0 || records[i] >= h->n_records) return sfail(h, -1, "%s: entry %lld names record %d of %lld", who, (long long)i,
                                                                     records[i], (long long)h->n_records);
        if (h->table[records[i]].kept >= 0) return sfail(h, -1, "%s: record %d is in the store already", who, records[i]);
    }
    std::vector<int32_t> seen(records, records + n);
    std::sort(seen.begin(), seen.end());
    const auto dup = std::adjacent_find(seen.begin(), seen.end());
    if (dup != seen.end()) return sfail(h, -1, "%s: record %d is named twice", who, *dup);
    return 0;
}

// the layout of an append: places and the new slabs' sizes, or the refusal (-3: the capacity)
int place_records(cl_store* h, const char* who, st::Cursor& cur, const Measured& ms, int64_t n, std::vector<st::Place>& places,
                  std::vector<uint64_t>& new_caps) {
    places.resize((size_t)n);
    int64_t at = 0;
    const int rc = st::layout_spans(cur, ms.span.data(), n, h->slab_bytes, h->capacity, places.data(), new_caps, &at);
    if (rc == st::LAYOUT_CAPACITY) {
        h->stats.refused_fit_records = at;               // what the caller's message needs: counted here, once
        h->stats.refused_fit_bytes = (int64_t)h->cur.stored;
        for (int64_t i = 0; i < at; ++i) h->stats.refused_fit_bytes += (int64_t)ms.span[(size_t)i];
        return sfail(h, -3, "%s: the store's capacity of %llu bytes would be exceeded: it holds %lld records in %llu bytes, and %lld of "
                            "the %lld records of this call fit", who, (unsigned long long)h->capacity, (long long)h->stats.records,
                     (unsigned long long)h->cur.stored, (long long)at, (long long)n);
    }
    if (rc == st::LAYOUT_SLAB)
        return sfail(h, -1, "%s: a record of %llu bytes does not fit a slab of %llu", who, (unsigned long long)ms.span[(size_t)at],
                     (unsigned long long)h->slab_bytes);
    return 0;
}

// the spans of records in the rows layout, by their extents
void rows_spans(const cl_store* h, const int32_t* kept, int64_t n, Measured& ms) {
    ms.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) ms.span[(size_t)i] = st::record_span(kept[i], h->window);
}

void commit(cl_store* h, const st::Cursor& cur, const int32_t* records, const int32_t* kept, const Measured& ms,
            const std::vector<st::Place>& places, int64_t n, int64_t record_bytes) {
    for (int64_t i = 0; i < n; ++i) {
        Rec& r = h->table[records[i]];
        r.slab = places[i].slab; r.off = places[i].off; r.kept = kept[i];
        const uint64_t b = ms.span[(size_t)i];
        r.format = ms.format[(size_t)i]; r.bytes = b;
        if (b) h->slabs[r.slab]->used = r.off + b;
        if (r.format == st::FORMAT_COMPACT) {
            ++h->fstats.compact_records; h->fstats.compact_bytes += (int64_t)b;
        } else {
            ++h->fstats.rows_records; h->fstats.rows_bytes += (int64_t)b;
        }
    }
    h->cur = cur;
    h->stats.records += n;
    h->stats.stored_bytes = (int64_t)cur.stored;
    h->stats.inflated_bytes += n * record_bytes;
    h->stats.slabs = (int64_t)h->slabs.size();
}

// What both assemble entries check: 0 = fine.
int check_assemble(cl_store* h, const char* who, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t R,
                   const void* const* pointers, int n_pointers) {
    const int32_t S = h->stored_rows;
    if (m < 0 || R < 1) return sfail(h, -1, "%s: bad shape", who);
    if (R > S) return sfail(h, -1, "%s: %d rows per site but only %d are stored", who, R, S);
    if (rows && S > plan_entry::MAX_STORED) return sfail(h, -1, "%s: %d stored rows do not fit a plan entry beside its zero-reads bit", who, S);
    if (m > INT32_MAX / 4 || (int64_t)R * h->window > INT32_MAX / 2) return sfail(h, -1, "%s: too large", who);
    if (m == 0) return 0;
    if (!records) return sfail(h, -1, "%s: null argument", who);
    for (int k = 0; k < n_pointers; ++k)
        if (!pointers[k]) return sfail(h, -1, "%s: null argument", who);
    for (int64_t i = 0; i < m; ++i) {
        if (records[i] < 0 || records[i] >= h->n_records) return sfail(h, -1, "%s: site %lld names record %d of %lld", who, (long long)i,
                                                                     records[i], (long long)h->n_records);
        if (h->table[records[i]].kept < 0) return sfail(h, -1, "%s: site %lld names record %d, which is not in the store", who, (long long)i,
                                                       records[i]);
        if (rows && !(first_rows && first_rows[i])) {
            const int16_t* r = rows + (size_t)i * R;
            for (int k = 0; k < R; ++k) {                   // (the zero-reads bit of an entry is not part of its row, plan_entry.h)
                const int row = plan_entry::stored_row(r[k]);
                if (row < 0 || row >= S) return sfail(h, -1, "%s: site %lld row %d names stored row %d of %d", who, (long long)i, k, row, S);
            }
        }
    }
    return 0;
}

int extent_arguments(cl_store* h, const char* who, const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes,
                     const int64_t* plane_off, int32_t S, int32_t W, int64_t* n_slots) {
    if (!plane_off || S < 1 || W < 1 || record_bytes < 1 || (int64_t)S * W > (1 << 24)) return sfail(h, -1, "%s: bad shape", who);
    if (!planes_inside(plane_off, record_bytes, (int64_t)S * W))
        return sfail(h, -1, "%s: a plane of %d rows of %d columns does not lie inside a record of %lld bytes", who, S, W, (long long)record_bytes);
    if (inflated_bytes && !inflated) return sfail(h, -1, "%s: null argument", who);
    *n_slots = (int64_t)(inflated_bytes / (uint64_t)record_bytes);
    return 0;
}

// the same for three plane arrays [n_slots][S][W]
int planes_arguments(cl_store* h, const char* who, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, int32_t S,
                     int32_t W) {
    if (S < 1 || W < 1 || (int64_t)S * W > (1 << 24) || n_slots < 0 || n_slots > INT32_MAX) return sfail(h, -1, "%s: bad shape", who);
    if (n_slots && (!reads || !qual || !strand)) return sfail(h, -1, "%s: null argument", who);
    return 0;
}

#ifndef CL_STORE_HOST_ONLY
#define ST_TRY(x) DEV_TRY(h->err, "", x)

int open_device(cl_store* h) {
    ST_TRY(hipSetDevice(h->device));
    ST_TRY(h->d_table.alloc((size_t)std::max<int64_t>(h->n_records, 1)));
    ST_TRY(hipMemset(h->d_table.p, 0, (size_t)std::max<int64_t>(h->n_records, 1) * sizeof(st::DevRec)));
    for (dev::Event& e : h->ev) ST_TRY(e.ensure(hipEventBlockingSync));
    return 0;
}

// What both device appends do once their source is known: slots[i] of src (n_slots of them, source_bytes each in the statistics)
// becomes record records[i].
int append_source(cl_store* h, const char* who, const st::Source& src, int64_t n_slots, int64_t source_bytes, const int32_t* slots,
                  const int32_t* records, int64_t n, void* stream, int32_t* kept_out) {
    if (const int rc = check_append(h, who, slots, records, n, n_slots, kept_out)) return rc;
    if (n == 0) return 0;
    dev::DeviceGuard guard;
    ST_TRY(hipSetDevice(h->device));
    h->wait_meta();
    hipStream_t s = (hipStream_t)stream;
    const bool compact = h->format == st::FORMAT_COMPACT;
    // slots | extents, or span sums | pack items | (compact) the rows' spans, which stay on the device
    const size_t b_i32 = (size_t)n * sizeof(int32_t), b_items = (size_t)n * sizeof(st::PackItem);
    const size_t b_meas = compact ? (size_t)n * sizeof(st::SpanSums) : b_i32;
    const size_t o_kept = (b_i32 + 15) & ~(size_t)15, o_items = o_kept + ((b_meas + 15) & ~(size_t)15);
    const size_t o_rowspans = o_items + ((b_items + 15) & ~(size_t)15);
    const size_t b_dev = o_rowspans + (compact ? (size_t)n * h->stored_rows * sizeof(uint16_t) : 0);
    if (h->d_app.ensure(b_dev) != hipSuccess) return sfail(h, -2, "hipMalloc of the append tables failed");
    if (h->h_app.ensure(o_rowspans) != hipSuccess) return sfail(h, -2, "hipHostMalloc of the append staging failed");
    memcpy(h->h_app.p, slots, b_i32);
    ST_TRY(hipMemcpyAsync(h->d_app.p, h->h_app.p, b_i32, hipMemcpyHostToDevice, s));
    ST_TRY(hipEventRecord(h->ev[0], s));
    if (compact)
        ST_TRY(st::launch_spans(src, (const int32_t*)h->d_app.p, n, (st::SpanSums*)(h->d_app.p + o_kept), (uint16_t*)(h->d_app.p + o_rowspans), s));
    else
        ST_TRY(st::launch_extent(src, (const int32_t*)h->d_app.p, n, (int32_t*)(h->d_app.p + o_kept), s));
    ST_TRY(hipEventRecord(h->ev[1], s));
    ST_TRY(hipMemcpyAsync(h->h_app.p + o_kept, h->d_app.p + o_kept, b_meas, hipMemcpyDeviceToHost, s));
    ST_TRY(hipStreamSynchronize(s));
    Measured ms;
    if (compact) {
        // every value the device returns is checked before it sizes anything
        const st::SpanSums* got = (const st::SpanSums*)(h->h_app.p + o_kept);
        ms.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            const st::SpanSums& g = got[i];
            if (g.kept < 0 || g.kept > h->stored_rows) return sfail(h, -2, "%s: the device gave an extent of %d rows", who, g.kept);
            if (g.cells < 0 || (int64_t)g.cells > (int64_t)g.kept * h->window)
                return sfail(h, -2, "%s: the device gave %d cells in %d rows of %d columns", who, g.cells, g.kept, h->window);
            if (g.mergeable != 0 && g.mergeable != 1) return sfail(h, -2, "%s: the device gave a mergeable flag of %d", who, g.mergeable);
            kept_out[i] = g.kept;
            ms.format[(size_t)i] = g.mergeable ? st::FORMAT_COMPACT : st::FORMAT_ROWS;
            ms.cells[(size_t)i] = g.cells;
            ms.span[(size_t)i] = st::format_span(ms.format[(size_t)i], g.kept, g.cells, h->window);
        }
    } else {
        const int32_t* h_kept = (const int32_t*)(h->h_app.p + o_kept);
        for (int64_t i = 0; i < n; ++i) {
            if (h_kept[i] < 0 || h_kept[i] > h->stored_rows) return sfail(h, -2, "%s: the device gave an extent of %d rows", who, h_kept[i]);
            kept_out[i] = h_kept[i];
        }
        rows_spans(h, kept_out, n, ms);
    }
    st::Cursor cur = h->cur;
    std::vector<st::Place> places;
    std::vector<uint64_t> new_caps;
    if (const int rc = place_records(h, who, cur, ms, n, places, new_caps)) return rc;
    const size_t had = h->slabs.size();
    for (uint64_t cap : new_caps) {
        std::unique_ptr<Slab> slab(new Slab());
        const size_t bytes = (size_t)(st::SLAB_GUARD + cap + st::SLAB_PAD);
        hipError_t e = slab->d.alloc(bytes);
        if (e == hipSuccess && h->fill >= 0) e = hipMemsetAsync(slab->d.p, h->fill, bytes, s);
        if (e != hipSuccess) {
            h->slabs.resize(had);
            return sfail(h, -2, "%s: hipMalloc of a slab of %llu bytes failed: %s", who, (unsigned long long)cap, hipGetErrorString(e));
        }
        slab->cap = cap;
        slab->data = slab->d.p + st::SLAB_GUARD;
        h->slabs.push_back(std::move(slab));
    }
    // the items of the records in the rows layout from the front, of the compact records from the back: a launch each
    st::PackItem* items = (st::PackItem*)(h->h_app.p + o_items);
    int64_t n_rows = 0, n_compact = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t addr = kept_out[i] ? (uint64_t)reinterpret_cast<uintptr_t>(h->slabs[places[i].slab]->data + places[i].off) : 0;
        const st::PackItem it{addr, slots[i], kept_out[i], records[i], (int32_t)i, ms.cells[(size_t)i], (int32_t)ms.span[(size_t)i]};
        if (ms.format[(size_t)i] == st::FORMAT_COMPACT) items[n - ++n_compact] = it;
        else items[n_rows++] = it;
    }
    const st::PackItem* d_items = (const st::PackItem*)(h->d_app.p + o_items);
    hipError_t rc = hipMemcpyAsync(h->d_app.p + o_items, items, b_items, hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) rc = hipEventRecord(h->ev[2], s);
    if (rc == hipSuccess) rc = st::launch_pack(src, d_items, n_rows, h->d_table.p, s);
    if (rc == hipSuccess)
        rc = st::launch_pack_compact(src, d_items + n_rows, n_compact, (const uint16_t*)(h->d_app.p + o_rowspans), h->d_table.p, s);
    if (rc == hipSuccess) rc = hipEventRecord(h->ev[3], s);
    if (rc == hipSuccess) rc = hipStreamSynchronize(s);
    if (rc != hipSuccess) {
        (void)hipStreamSynchronize(s);                    // (nothing of the call is in flight when its slabs go)
        h->slabs.resize(had);
        return sfail(h, -2, "%s: device: %s", who, hipGetErrorString(rc));
    }
    float t_ms[2] = {0, 0};
    ST_TRY(hipEventElapsedTime(&t_ms[0], h->ev[0], h->ev[1]));
    ST_TRY(hipEventElapsedTime(&t_ms[1], h->ev[2], h->ev[3]));
    (compact ? h->fstats.spans_ms : h->stats.extent_ms) += t_ms[0];
    h->stats.pack_ms += t_ms[1];
    commit(h, cur, records, kept_out, ms, places, n, source_bytes);
    return 0;
}

int append_device(cl_store* h, cl_loader_t* loader, const int32_t* slots, const int32_t* records, int64_t n, void* stream, int32_t* kept_out) {
    const char* who = "cl_store_append_device";
    if (h->on_host) return sfail(h, -1, "%s: the store was opened in host memory", who);
    if (!loader) return sfail(h, -1, "%s: null loader", who);
    const clh::RecordsView v = clh::records_view(loader);
    if (v.window != h->window || v.stored_rows != h->stored_rows)
        return sfail(h, -1, "%s: the loader holds records of %d rows of %d columns, the store of %d of %d", who, v.stored_rows, v.window,
                     h->stored_rows, h->window);
    if (v.device != h->device) return sfail(h, -1, "%s: the loader is on device %d, the store on device %d", who, v.device, h->device);
    st::Source src{};
    for (int p = 0; p < 3; ++p) src.plane[p] = v.records + v.plane_off[p];
    src.stride = v.record_bytes; src.S = h->stored_rows; src.W = h->window;
    return append_source(h, who, src, v.n_records, v.record_bytes, slots, records, n, stream, kept_out);
}

int append_planes_device(cl_store* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, const int32_t* slots,
                         const int32_t* records, int64_t n, void* stream, int32_t* kept_out) {
    const char* who = "cl_store_append_planes_device";
    if (h->on_host) return sfail(h, -1, "%s: the store was opened in host memory", who);
    if (const int rc = planes_arguments(h, who, reads, qual, strand, n_slots, h->stored_rows, h->window)) return rc;
    st::Source src{};
    src.plane[0] = reads; src.plane[1] = qual; src.plane[2] = strand;
    src.stride = (int64_t)h->stored_rows * h->window; src.S = h->stored_rows; src.W = h->window;
    return append_source(h, who, src, n_slots, 3 * src.stride, slots, records, n, stream, kept_out);
}

int assemble_device(cl_store* h, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t R,
                    const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand, uint8_t* const out[6],
                    void* stream) {
    const char* who = "cl_store_assemble_device";
    if (h->on_host) return sfail(h, -1, "%s: the store was opened in host memory", who);
    const void* ptrs[9] = {ref, ref_mask, var_mask, out[0], out[1], out[2], out[3], out[4], out[5]};
    if (const int rc = check_assemble(h, who, records, rows, first_rows, m, R, ptrs, 9)) return rc;
    if (m == 0) return 0;
    const int32_t L = h->window;
    bool any_rows = false;
    for (int64_t i = 0; i < m && rows && !any_rows; ++i) any_rows = !(first_rows && first_rows[i]);
    dev::DeviceGuard guard;
    if (hipSetDevice(h->device) != hipSuccess) return sfail(h, -2, "hipSetDevice(%d) failed", h->device);
    if (h->ev_meta.ensure(hipEventDisableTiming) != hipSuccess) return sfail(h, -2, "hipEventCreate failed");
    if (h->meta_busy) {                                  // the previous call's staging and device copies are still its own
        if (hipEventSynchronize(h->ev_meta) != hipSuccess) return sfail(h, -2, "hipEventSynchronize failed");
        h->meta_busy = false;
    }
    const size_t b_sites = (size_t)m * sizeof(pg::SiteSrc), b_rows = any_rows ? (size_t)m * R * sizeof(int16_t) : 0;
    const size_t b_dev = b_sites + b_rows, b_line = (size_t)m * L;
    if (h->d_meta.ensure(b_dev) != hipSuccess) return sfail(h, -2, "hipMalloc of the assembly table failed");
    if (h->h_meta.ensure(b_dev + 3 * b_line) != hipSuccess) return sfail(h, -2, "hipHostMalloc of the assembly staging failed");
    pg::SiteSrc* hs = (pg::SiteSrc*)h->h_meta.p;
    for (int64_t i = 0; i < m; ++i) hs[i] = pg::SiteSrc{records[i], (!rows || (first_rows && first_rows[i])) ? 1 : 0};
    if (b_rows) memcpy(h->h_meta.p + b_sites, rows, b_rows);
    uint8_t* lines = h->h_meta.p + b_dev;
    memcpy(lines, ref, b_line); memcpy(lines + b_line, ref_mask, b_line); memcpy(lines + 2 * b_line, var_mask, b_line);
    hipStream_t s = (hipStream_t)stream;
    const bool timed = hipEventRecord(h->ev[4], s) == hipSuccess;
    hipError_t rc = hipMemcpyAsync(h->d_meta.p, h->h_meta.p, b_dev, hipMemcpyHostToDevice, s);
    for (int c = 0; c < 3 && rc == hipSuccess; ++c)
        rc = hipMemcpyAsync(out[3 + c], lines + c * b_line, b_line, hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) {
        st::AssembleArgs a{};
        a.table = h->d_table.p;
        a.dst[0] = out[0]; a.dst[1] = out[1]; a.dst[2] = out[2];
        a.sites = (const pg::SiteSrc*)h->d_meta.p;
        a.rows = (const int16_t*)(h->d_meta.p + b_sites);
        a.R = R; a.L = L;
        a.use[0] = 1; a.use[1] = use_q != 0; a.use[2] = use_strand != 0;
        rc = st::launch_store_assemble(a, (int32_t)m, h->fstats.compact_records > 0, s);
    }
    h->meta_busy = true;                                 // (also after a failure: some of the copies may be enqueued)
    if (hipEventRecord(h->ev_meta, s) != hipSuccess && rc == hipSuccess) rc = hipErrorUnknown;
    if (rc != hipSuccess) return sfail(h, -2, "device: %s", hipGetErrorString(rc));
    h->assemble_timed = timed && hipEventRecord(h->ev[5], s) == hipSuccess;
    return 0;
}
#endif

// What both host appends do once their source is known (append_source on a host store).
int pack_source(cl_store* h, const char* who, const st::HostSource& src, int64_t n_slots, int64_t source_bytes, const int32_t* slots,
                const int32_t* records, int64_t n, int32_t* kept_out) {
    if (const int rc = check_append(h, who, slots, records, n, n_slots, kept_out)) return rc;
    const bool compact = h->format == st::FORMAT_COMPACT;
    const size_t S = (size_t)h->stored_rows;
    Measured ms;
    std::vector<uint16_t> rowspans;
    if (compact) {
        ms.resize((size_t)n);
        rowspans.resize((size_t)n * S);
        for (int64_t i = 0; i < n; ++i) {
            const st::SpanSums g = st::spans_host(src, slots[i], h->stored_rows, h->window, rowspans.data() + (size_t)i * S);
            kept_out[i] = g.kept;
            ms.format[(size_t)i] = g.mergeable ? st::FORMAT_COMPACT : st::FORMAT_ROWS;
            ms.cells[(size_t)i] = g.cells;
            ms.span[(size_t)i] = st::format_span(ms.format[(size_t)i], g.kept, g.cells, h->window);
        }
    } else {
        for (int64_t i = 0; i < n; ++i) kept_out[i] = st::extent_host(src, slots[i], h->stored_rows, h->window);
        rows_spans(h, kept_out, n, ms);
    }
    st::Cursor cur = h->cur;
    std::vector<st::Place> places;
    std::vector<uint64_t> new_caps;
    if (const int rc = place_records(h, who, cur, ms, n, places, new_caps)) return rc;
    for (uint64_t cap : new_caps) {
        std::unique_ptr<Slab> slab(new Slab());
        slab->host.reset(new uint8_t[(size_t)cap]);
        if (h->fill >= 0) memset(slab->host.get(), h->fill, (size_t)cap);
        slab->cap = cap;
        slab->data = slab->host.get();
        h->slabs.push_back(std::move(slab));
    }
    for (int64_t i = 0; i < n; ++i) {
        if (!kept_out[i]) continue;
        uint8_t* dst = h->slabs[places[i].slab]->data + places[i].off;
        if (ms.format[(size_t)i] == st::FORMAT_COMPACT) st::pack_compact_host(src, slots[i], h->window, kept_out[i], rowspans.data() + (size_t)i * S, dst);
        else st::pack_host(src, slots[i], h->window, kept_out[i], dst);
    }
    commit(h, cur, records, kept_out, ms, places, n, source_bytes);
    return 0;
}

int pack_host(cl_store* h, const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off, const int32_t* slots,
              const int32_t* records, int64_t n, int32_t* kept_out) {
    const char* who = "cl_store_pack_host";
    if (!h->on_host) return sfail(h, -1, "%s: the store was opened on a device", who);
    int64_t n_slots = 0;
    if (const int rc = extent_arguments(h, who, inflated, inflated_bytes, record_bytes, plane_off, h->stored_rows, h->window, &n_slots)) return rc;
    return pack_source(h, who, st::record_source(inflated, record_bytes, plane_off), n_slots, record_bytes, slots, records, n, kept_out);
}

int pack_planes_host(cl_store* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, const int32_t* slots,
                     const int32_t* records, int64_t n, int32_t* kept_out) {
    const char* who = "cl_store_pack_planes_host";
    if (!h->on_host) return sfail(h, -1, "%s: the store was opened on a device", who);
    if (const int rc = planes_arguments(h, who, reads, qual, strand, n_slots, h->stored_rows, h->window)) return rc;
    return pack_source(h, who, st::planar_source(reads, qual, strand, h->stored_rows, h->window), n_slots,
                       3 * (int64_t)h->stored_rows * h->window, slots, records, n, kept_out);
}

int assemble_host(cl_store* h, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t R, const uint8_t* ref,
                  const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand, uint8_t* const out[6]) {
    const char* who = "cl_store_assemble_host";
    if (!h->on_host) return sfail(h, -1, "%s: the store was opened on a device", who);
    const void* ptrs[9] = {ref, ref_mask, var_mask, out[0], out[1], out[2], out[3], out[4], out[5]};
    if (const int rc = check_assemble(h, who, records, rows, first_rows, m, R, ptrs, 9)) return rc;
    const int32_t L = h->window;
    const size_t span = (size_t)R * L;
    const int use[3] = {1, use_q != 0, use_strand != 0};
    for (int64_t i = 0; i < m; ++i) {
        const Rec& r = h->table[records[i]];
        const bool first = !rows || (first_rows && first_rows[i]);
        for (int p = 0; p < 3; ++p) {
            uint8_t* dst = out[p] + (size_t)i * span;
            if (!use[p]) {
                memset(dst, 0, span);
                continue;
            }
            const uint8_t* rec = r.kept ? h->slabs[r.slab]->data + r.off : nullptr;
            const int16_t* site_rows = first ? nullptr : rows + (size_t)i * R;
            if (r.format == st::FORMAT_COMPACT) st::assemble_compact_plane_host(rec, r.kept, p, site_rows, R, L, dst);
            else st::assemble_plane_host(rec ? rec + (size_t)p * r.kept * L : nullptr, r.kept, p, site_rows, R, L, dst);
        }
    }
    const size_t b_line = (size_t)m * L;
    if (b_line) {
        memcpy(out[3], ref, b_line); memcpy(out[4], ref_mask, b_line); memcpy(out[5], var_mask, b_line);
    }
    return 0;
}

}  // namespace

extern "C" {

const char* cl_store_last_error(const cl_store_t* h) { return h ? h->err.c_str() : g_store_err.c_str(); }

int cl_store_open(int32_t window, int32_t stored_rows, int64_t n_records, uint64_t capacity_bytes, uint64_t slab_bytes, int32_t device,
                  cl_store_t** out) {
    if (!out) return sfail(nullptr, -1, "cl_store_open: null argument");
    *out = nullptr;
    if (window < 1 || stored_rows < 1 || stored_rows > INT16_MAX || (int64_t)window * stored_rows > (1 << 24) || n_records < 0 ||
        n_records > INT32_MAX / 2)
        return sfail(nullptr, -1, "cl_store_open: bad shape");
    if (slab_bytes < 16 || (slab_bytes & 15) || slab_bytes > ((uint64_t)1 << 40))
        return sfail(nullptr, -1, "cl_store_open: a slab holds a multiple of 16 bytes, 16 to 2^40");
#ifdef CL_STORE_HOST_ONLY
    if (device >= 0) return sfail(nullptr, -1, "cl_store_open: this build has the host store only (device < 0)");
#endif
    return capi::guarded(g_store_err, "cl_store_open", [&] {
        std::unique_ptr<cl_store> h(new cl_store());
        h->window = window; h->stored_rows = stored_rows; h->n_records = n_records;
        h->capacity = capacity_bytes; h->slab_bytes = slab_bytes;
        h->device = device; h->on_host = device < 0;
        h->table.resize((size_t)n_records);
#ifndef CL_STORE_HOST_ONLY
        if (!h->on_host) {
            dev::DeviceGuard guard;
            if (const int rc = open_device(h.get())) {
                g_store_err = h->err;
                return rc;
            }
        }
#endif
        *out = h.release();
        return 0;
    });
}

void cl_store_close(cl_store_t* h) {
    try {
#ifndef CL_STORE_HOST_ONLY
        if (h && !h->on_host) {
            dev::DeviceGuard guard;
            (void)hipSetDevice(h->device);
            delete h;
            return;
        }
#endif
        delete h;
    } catch (...) {
    }
}

int cl_store_debug_fill(cl_store_t* h, int32_t value) {
    if (!h) return sfail(nullptr, -1, "cl_store_debug_fill: null handle");
    if (value < -1 || value > 255) return sfail(h, -1, "cl_store_debug_fill: -1 (no fill) or a byte");
    h->fill = value;
    return 0;
}

int cl_store_set_format(cl_store_t* h, int32_t format) {
    if (!h) return sfail(nullptr, -1, "cl_store_set_format: null handle");
    return capi::guarded(h->err, "cl_store_set_format", [&] {
        if (format != st::FORMAT_ROWS && format != st::FORMAT_COMPACT)
            return sfail(h, -1, "cl_store_set_format: format %d: 0 (rows) or 1 (compact)", format);
        if (h->stats.records > 0) return sfail(h, -1, "cl_store_set_format: the store holds records already: the format is chosen before the first append");
        if (format == st::FORMAT_COMPACT && h->window > st::COMPACT_MAX_WINDOW)
            return sfail(h, -1, "cl_store_set_format: the compact format keeps a row's first column and length in eight bits each: a window of "
                                "%d columns exceeds its %d", h->window, st::COMPACT_MAX_WINDOW);
        h->format = format;
        return 0;
    });
}

int cl_store_append_device(cl_store_t* h, cl_loader_t* loader, const int32_t* slots, const int32_t* records, int64_t n, void* stream,
                           int32_t* kept_out) {
    if (!h) return sfail(nullptr, -1, "cl_store_append_device: null handle");
#ifdef CL_STORE_HOST_ONLY
    (void)loader; (void)slots; (void)records; (void)n; (void)stream; (void)kept_out;
    return sfail(h, -1, "cl_store_append_device: this build has the host store only");
#else
    return capi::guarded(h->err, "cl_store_append_device", [&] { return append_device(h, loader, slots, records, n, stream, kept_out); });
#endif
}

int cl_store_append_planes_device(cl_store_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots,
                                  const int32_t* slots, const int32_t* records, int64_t n, void* stream, int32_t* kept_out) {
    if (!h) return sfail(nullptr, -1, "cl_store_append_planes_device: null handle");
#ifdef CL_STORE_HOST_ONLY
    (void)reads; (void)qual; (void)strand; (void)n_slots; (void)slots; (void)records; (void)n; (void)stream; (void)kept_out;
    return sfail(h, -1, "cl_store_append_planes_device: this build has the host store only");
#else
    return capi::guarded(h->err, "cl_store_append_planes_device", [&] {
        return append_planes_device(h, reads, qual, strand, n_slots, slots, records, n, stream, kept_out);
    });
#endif
}

int cl_store_assemble_device(cl_store_t* h, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t reads,
                             const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                             uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                             uint8_t* var_mask_out, void* stream) {
    if (!h) return sfail(nullptr, -1, "cl_store_assemble_device: null handle");
#ifdef CL_STORE_HOST_ONLY
    (void)records; (void)rows; (void)first_rows; (void)m; (void)reads; (void)ref; (void)ref_mask; (void)var_mask; (void)use_q; (void)use_strand;
    (void)reads_out; (void)qual_out; (void)strand_out; (void)ref_out; (void)ref_mask_out; (void)var_mask_out; (void)stream;
    return sfail(h, -1, "cl_store_assemble_device: this build has the host store only");
#else
    return capi::guarded(h->err, "cl_store_assemble_device", [&] {
        uint8_t* const out[6] = {reads_out, qual_out, strand_out, ref_out, ref_mask_out, var_mask_out};
        return assemble_device(h, records, rows, first_rows, m, reads, ref, ref_mask, var_mask, use_q, use_strand, out, stream);
    });
#endif
}

int cl_store_center_counts_device(cl_store_t* h, const uint8_t* reads, int64_t m, int32_t rows, int32_t window, int32_t* counts, void* stream) {
    if (!h) return sfail(nullptr, -1, "cl_store_center_counts_device: null handle");
#ifdef CL_STORE_HOST_ONLY
    (void)reads; (void)m; (void)rows; (void)window; (void)counts; (void)stream;
    return sfail(h, -1, "cl_store_center_counts_device: this build has the host store only");
#else
    return capi::guarded(h->err, "cl_store_center_counts_device", [&] {
        if (h->on_host) return sfail(h, -1, "cl_store_center_counts_device: the store was opened in host memory");
        if (m < 0 || m > INT32_MAX || rows < 1 || window < 3) return sfail(h, -1, "cl_store_center_counts_device: bad shape");
        if (m > 0 && (!reads || !counts)) return sfail(h, -1, "cl_store_center_counts_device: null argument");
        dev::DeviceGuard guard;
        ST_TRY(hipSetDevice(h->device));
        ST_TRY(pg::launch_center_counts(reads, m, rows, window, (window - 1) / 2, counts, (hipStream_t)stream));
        return 0;
    });
#endif
}

int cl_store_extent_host(const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off, int32_t stored_rows,
                         int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out) {
    const char* who = "cl_store_extent_host";
    return capi::guarded(g_store_err, who, [&] {
        int64_t n_slots = 0;
        if (const int rc = extent_arguments(nullptr, who, inflated, inflated_bytes, record_bytes, plane_off, stored_rows, window, &n_slots)) return rc;
        if (n < 0) return sfail(nullptr, -1, "%s: bad record count", who);
        if (n > 0 && (!slots || !kept_out)) return sfail(nullptr, -1, "%s: null argument", who);
        for (int64_t i = 0; i < n; ++i)
            if (slots[i] < 0 || slots[i] >= n_slots) return sfail(nullptr, -1, "%s: entry %lld names slot %d of %lld", who, (long long)i, slots[i],
                                                              (long long)n_slots);
        const st::HostSource src = st::record_source(inflated, record_bytes, plane_off);
        for (int64_t i = 0; i < n; ++i) kept_out[i] = st::extent_host(src, slots[i], stored_rows, window);
        return 0;
    });
}

int cl_store_extent_planes_host(const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, int32_t stored_rows,
                                int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out) {
    const char* who = "cl_store_extent_planes_host";
    return capi::guarded(g_store_err, who, [&] {
        if (const int rc = planes_arguments(nullptr, who, reads, qual, strand, n_slots, stored_rows, window)) return rc;
        if (n < 0) return sfail(nullptr, -1, "%s: bad record count", who);
        if (n > 0 && (!slots || !kept_out)) return sfail(nullptr, -1, "%s: null argument", who);
        for (int64_t i = 0; i < n; ++i)
            if (slots[i] < 0 || slots[i] >= n_slots) return sfail(nullptr, -1, "%s: entry %lld names slot %d of %lld", who, (long long)i, slots[i],
                                                              (long long)n_slots);
        const st::HostSource src = st::planar_source(reads, qual, strand, stored_rows, window);
        for (int64_t i = 0; i < n; ++i) kept_out[i] = st::extent_host(src, slots[i], stored_rows, window);
        return 0;
    });
}

namespace {

// what both spans entries do once their source is known
int spans_source(const char* who, const st::HostSource& src, int64_t n_slots, int32_t S, int32_t W, const int32_t* slots, int64_t n, int32_t* kept_out,
                 int32_t* cells_out, int32_t* mergeable_out, uint16_t* rowspans_out) {
    if (W > st::COMPACT_MAX_WINDOW) return sfail(nullptr, -1, "%s: a window of %d columns exceeds the compact format's %d", who, W, st::COMPACT_MAX_WINDOW);
    if (n < 0) return sfail(nullptr, -1, "%s: bad record count", who);
    if (n > 0 && (!slots || !kept_out || !cells_out || !mergeable_out || !rowspans_out)) return sfail(nullptr, -1, "%s: null argument", who);
    for (int64_t i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= n_slots) return sfail(nullptr, -1, "%s: entry %lld names slot %d of %lld", who, (long long)i, slots[i],
                                                          (long long)n_slots);
    for (int64_t i = 0; i < n; ++i) {
        const st::SpanSums g = st::spans_host(src, slots[i], S, W, rowspans_out + (size_t)i * S);
        kept_out[i] = g.kept; cells_out[i] = g.cells; mergeable_out[i] = g.mergeable;
    }
    return 0;
}

}  // namespace

int cl_store_spans_host(const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off, int32_t stored_rows,
                        int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out, int32_t* cells_out, int32_t* mergeable_out,
                        uint16_t* rowspans_out) {
    const char* who = "cl_store_spans_host";
    return capi::guarded(g_store_err, who, [&] {
        int64_t n_slots = 0;
        if (const int rc = extent_arguments(nullptr, who, inflated, inflated_bytes, record_bytes, plane_off, stored_rows, window, &n_slots)) return rc;
        return spans_source(who, st::record_source(inflated, record_bytes, plane_off), n_slots, stored_rows, window, slots, n, kept_out, cells_out,
                            mergeable_out, rowspans_out);
    });
}

int cl_store_spans_planes_host(const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots, int32_t stored_rows,
                               int32_t window, const int32_t* slots, int64_t n, int32_t* kept_out, int32_t* cells_out, int32_t* mergeable_out,
                               uint16_t* rowspans_out) {
    const char* who = "cl_store_spans_planes_host";
    return capi::guarded(g_store_err, who, [&] {
        if (const int rc = planes_arguments(nullptr, who, reads, qual, strand, n_slots, stored_rows, window)) return rc;
        return spans_source(who, st::planar_source(reads, qual, strand, stored_rows, window), n_slots, stored_rows, window, slots, n, kept_out,
                            cells_out, mergeable_out, rowspans_out);
    });
}

int cl_store_pack_planes_host(cl_store_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, int64_t n_slots,
                              const int32_t* slots, const int32_t* records, int64_t n, int32_t* kept_out) {
    if (!h) return sfail(nullptr, -1, "cl_store_pack_planes_host: null handle");
    return capi::guarded(h->err, "cl_store_pack_planes_host", [&] {
        return pack_planes_host(h, reads, qual, strand, n_slots, slots, records, n, kept_out);
    });
}

int cl_store_pack_host(cl_store_t* h, const uint8_t* inflated, uint64_t inflated_bytes, int64_t record_bytes, const int64_t* plane_off,
                       const int32_t* slots, const int32_t* records, int64_t n, int32_t* kept_out) {
    if (!h) return sfail(nullptr, -1, "cl_store_pack_host: null handle");
    return capi::guarded(h->err, "cl_store_pack_host", [&] {
        return pack_host(h, inflated, inflated_bytes, record_bytes, plane_off, slots, records, n, kept_out);
    });
}

int cl_store_assemble_host(cl_store_t* h, const int32_t* records, const int16_t* rows, const uint8_t* first_rows, int64_t m, int32_t reads,
                           const uint8_t* ref, const uint8_t* ref_mask, const uint8_t* var_mask, int32_t use_q, int32_t use_strand,
                           uint8_t* reads_out, uint8_t* qual_out, uint8_t* strand_out, uint8_t* ref_out, uint8_t* ref_mask_out,
                           uint8_t* var_mask_out, void* stream) {
    (void)stream;
    if (!h) return sfail(nullptr, -1, "cl_store_assemble_host: null handle");
    return capi::guarded(h->err, "cl_store_assemble_host", [&] {
        uint8_t* const out[6] = {reads_out, qual_out, strand_out, ref_out, ref_mask_out, var_mask_out};
        return assemble_host(h, records, rows, first_rows, m, reads, ref, ref_mask, var_mask, use_q, use_strand, out);
    });
}

int cl_store_record(cl_store_t* h, int64_t record, int32_t* slab, int64_t* offset, int32_t* kept) {
    if (!h || !slab || !offset || !kept) return sfail(h, -1, "cl_store_record: null argument");
    return capi::guarded(h->err, "cl_store_record", [&] {
        if (record < 0 || record >= h->n_records) return sfail(h, -1, "cl_store_record: record %lld of %lld", (long long)record, (long long)h->n_records);
        const Rec& r = h->table[(size_t)record];
        if (r.kept < 0) return sfail(h, -1, "cl_store_record: record %lld is not in the store", (long long)record);
        *slab = r.slab; *offset = (int64_t)r.off; *kept = r.kept;
#ifndef CL_STORE_HOST_ONLY
        if (!h->on_host) {                               // what the kernels follow: the device's table entry
            dev::DeviceGuard guard;
            st::DevRec d{};
            ST_TRY(hipSetDevice(h->device));
            ST_TRY(hipMemcpy(&d, h->d_table.p + record, sizeof d, hipMemcpyDeviceToHost));
            *kept = d.kept; *slab = -1; *offset = -1;
            if (d.addr == 0) { *slab = 0; *offset = 0; }
            for (size_t k = 0; k < h->slabs.size() && d.addr; ++k) {
                const uint64_t base = (uint64_t)reinterpret_cast<uintptr_t>(h->slabs[k]->data);
                if (d.addr >= base && d.addr < base + h->slabs[k]->cap) { *slab = (int32_t)k; *offset = (int64_t)(d.addr - base); }
            }
        }
#endif
        return 0;
    });
}

int cl_store_record_span(cl_store_t* h, int64_t record, int32_t* format, int64_t* bytes) {
    if (!h || !format || !bytes) return sfail(h, -1, "cl_store_record_span: null argument");
    return capi::guarded(h->err, "cl_store_record_span", [&] {
        if (record < 0 || record >= h->n_records)
            return sfail(h, -1, "cl_store_record_span: record %lld of %lld", (long long)record, (long long)h->n_records);
        const Rec& r = h->table[(size_t)record];
        if (r.kept < 0) return sfail(h, -1, "cl_store_record_span: record %lld is not in the store", (long long)record);
        *format = r.format; *bytes = (int64_t)r.bytes;
#ifndef CL_STORE_HOST_ONLY
        if (!h->on_host) {                               // the format the kernels follow: the device's table entry
            dev::DeviceGuard guard;
            st::DevRec d{};
            ST_TRY(hipSetDevice(h->device));
            ST_TRY(hipMemcpy(&d, h->d_table.p + record, sizeof d, hipMemcpyDeviceToHost));
            *format = d.format;
        }
#endif
        return 0;
    });
}

int cl_store_slab(cl_store_t* h, int32_t slab, uint8_t* dst, uint64_t dst_bytes, int64_t* data_off, int64_t* used, int64_t* capacity) {
    if (!h || !data_off || !used || !capacity) return sfail(h, -1, "cl_store_slab: null argument");
    return capi::guarded(h->err, "cl_store_slab", [&] {
        if (slab < 0 || (size_t)slab >= h->slabs.size()) return sfail(h, -1, "cl_store_slab: slab %d of %lld", slab, (long long)h->slabs.size());
        const Slab& s = *h->slabs[slab];
        *used = (int64_t)s.used; *capacity = (int64_t)s.cap;
        *data_off = h->on_host ? 0 : st::SLAB_GUARD;
        const uint64_t bytes = h->on_host ? s.cap : (uint64_t)(st::SLAB_GUARD + s.cap + st::SLAB_PAD);
        if (!dst) return 0;                              // (the sizes alone)
        if (dst_bytes < bytes) return sfail(h, -1, "cl_store_slab: the slab's allocation holds %llu bytes", (unsigned long long)bytes);
        if (h->on_host) {
            memcpy(dst, s.host.get(), (size_t)bytes);
            return 0;
        }
#ifndef CL_STORE_HOST_ONLY
        dev::DeviceGuard guard;
        ST_TRY(hipSetDevice(h->device));
        ST_TRY(hipMemcpy(dst, s.d.p, (size_t)bytes, hipMemcpyDeviceToHost));
#endif
        return 0;
    });
}

int cl_store_get_stats(cl_store_t* h, cl_store_stats* out) {
    if (!h || !out) return sfail(h, -1, "cl_store_get_stats: null argument");
#ifndef CL_STORE_HOST_ONLY
    if (h->assemble_timed) {
        float ms = 0;
        if (hipEventSynchronize(h->ev[5]) == hipSuccess && hipEventElapsedTime(&ms, h->ev[4], h->ev[5]) == hipSuccess) h->stats.assemble_ms = ms;
        h->assemble_timed = false;
    }
#endif
    *out = h->stats;
    return 0;
}

int cl_store_get_format_stats(cl_store_t* h, cl_store_format_stats* out) {
    if (!h || !out) return sfail(h, -1, "cl_store_get_format_stats: null argument");
    *out = h->fstats;
    out->format = h->format;
    return 0;
}

}  // extern "C"
