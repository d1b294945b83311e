// C ABI of libdl4vc_dan.so (include/dl4vc_dan.h): handle lifecycle, upload of the packed checkpoint (dan_pack.h), chunked
// execution plan.  Host code only; kernels are in dan_kernels.hip.  Every device resource of a handle is a member that frees
// itself (device_buffer.h); every entry whose body can throw runs under capi::guarded (capi_shell.h).
#include "../../include/dl4vc_dan.h"
#include "dan_kernels.h"
#include "dan_net.h"
#include "dan_pack.h"
#include "device_buffer.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <vector>

using namespace dan;

namespace {

std::string g_create_error;

struct EventPair { dev::Event a, b; };
struct KernelStat {
    std::vector<EventPair*> pending;
    int64_t launches = 0;
    double ms = 0.0;
};

struct Family;

// floats per site of bin_logits, vt_logits, vt_prob, bp, aux
constexpr int OUT_W[5] = {2, 3, 3, 1, 22};
constexpr int OUT_TOTAL = 2 + 3 + 3 + 1 + 22;

// the six input planes (reads, qual, strand [B][R][L]; ref, ref_mask, var_mask [B][L]) and their bytes per site
struct Planes {
    const uint8_t* p[6];
    size_t per_site[6];
    Planes(const dan_config& c, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, const uint8_t* ref,
           const uint8_t* ref_mask, const uint8_t* var_mask) : p{reads, qual, strand, ref, ref_mask, var_mask} {
        for (int i = 0; i < 6; ++i) per_site[i] = i < 3 ? (size_t)c.reads * c.length : (size_t)c.length;
    }
    // a batch of nb sites, plane behind plane in one block (the staging buffers): where each plane starts, and the block's bytes
    size_t offsets(size_t nb, size_t off[6]) const {
        size_t o = 0;
        for (int i = 0; i < 6; ++i) { off[i] = o; o += nb * per_site[i]; }
        return o;
    }
    Planes(const dan_config& c, const uint8_t* block, size_t nb) : Planes(c, block, block, block, block, block, block) {
        size_t off[6];
        offsets(nb, off);
        for (int i = 0; i < 6; ++i) p[i] = block + off[i];
    }
    Planes at(int64_t site) const { Planes q = *this; for (int i = 0; i < 6; ++i) q.p[i] += (size_t)site * per_site[i]; return q; }
    bool complete() const { for (auto q : p) if (!q) return false; return true; }
    size_t site_bytes() const { size_t off[6]; return offsets(1, off); }
};

// the five outputs; any may be null
struct Outs {
    float* p[5];
    Outs(float* bin_logits, float* vt_logits, float* vt_prob, float* bp, float* aux) : p{bin_logits, vt_logits, vt_prob, bp, aux} {}
    // a batch of nb sites, output behind output in one block of nb * OUT_TOTAL floats
    Outs(float* block, size_t nb) : p{} { for (int i = 0; i < 5; ++i) { p[i] = block; block += nb * OUT_W[i]; } }
    Outs at(int64_t site) const { Outs q = *this; for (int i = 0; i < 5; ++i) if (q.p[i]) q.p[i] += site * OUT_W[i]; return q; }
};

}  // namespace

struct dan_handle {
    dan_config cfg{};
    TensorMap tensors;
    bool finalized = false;
    mutable std::string err;
    int n_segments = 0;
    std::vector<int> seg_begin, seg_end;     // 0-based layer ranges
    int F = 0;                               // feature width
    int64_t F_stride = 0;                    // padded to a multiple of 16
    int n0_stride = 0;                       // fc_sizes[0] padded to a multiple of 16 (K of the second FC)
    int chunk = 0, max_batch = 0;
    bool chunk_auto = false;                                   // the chunk was sized by dan_create (free device memory), not by the caller
    int wino = 0;                            // dilation-2 layers in Winograd form (F(4,3) or F(2,3) by window: launch_segment)
    int tap_layer = -1;
    int last_chunk_sites = 0;
    int64_t last_batch = 0;
    // device memory: every block below is owned by `blocks`
    dev::Blocks blocks;
    float* d_wl = nullptr;                   // [layers][LAYER_STRIDE] weight blocks (fp32 path)
    char* d_wlp = nullptr;                   // [layers][WP_LAYER_BYTES] 32x32x16 fragments of the ping-pong bf16 kernel (precision 2)
    char* d_wlr = nullptr;                   // the same blocks as 16x16x32 fragments (sixteen-wave form, dan_config.bf16_form = 1)
    float* d_wc16 = nullptr;                 // compression weights in the channel order of a 16-byte bf16 load of h
    const float* d_hw = nullptr;             // d_wc or d_wc16: what the family's highway kernel reads
    float *d_wpool = nullptr, *d_cols = nullptr, *d_cp = nullptr, *d_zero = nullptr;   // conv(read-mean): weights [segment][128][384], scratch, result
    const Family* fam = nullptr;             // the kernel family of cfg.precision (FAMILIES below), chosen by dan_finalize
    char* d_wlx = nullptr;                   // [layers][WX_LAYER_BYTES] hi / lo 16x16x32 fragments of the bf16x3 kernel
    unsigned res_mask = 0;
    float *d_emb = nullptr, *d_pe = nullptr;
    float* d_l0tab = nullptr;                // fp32 path: layer 1 by table (dan_kernels.h L0_*)
    float *d_y = nullptr, *d_pool = nullptr, *d_h = nullptr, *d_tap = nullptr;
    float* d_y2 = nullptr;                   // fp32 windows above MPOS columns (two units per read): the segments' y alternates between d_y and d_y2
    bool split = false;
    int* d_rowsrc = nullptr;                 // empty-row map of the current chunk (skip_empty_rows)
    int *d_work = nullptr, *d_work_count = nullptr;   // ... and the list of rows to compute
    int n_cus = 0;
    // read-axis pooling inside the segment kernel (dan_kernels.h SegmentArgs::fold; dan_set_pool_form)
    const char* fold_why_not = nullptr;      // why the in-segment form does not apply to this handle (null: it does)
    int pool_form = 0;                       // 0 = per chunk by its site count, 1 = separate tail kernels, 2 = in-segment
    int last_pool_form = 1;                  // the form the last chunk ran (before the first: the one a full chunk would)
    float* d_fold = nullptr;                 // [workgroup][2][L][CPAD] running planes of the site-owning workgroups
    float *d_wc = nullptr, *d_bc = nullptr;
    float *d_feat = nullptr, *d_hid0 = nullptr, *d_hid1 = nullptr;
    float* d_fc_ws = nullptr;                                  // split-k partial sums of FC1 [2][max_batch][fc0]
    float *d_w0 = nullptr, *d_b0 = nullptr, *d_w1 = nullptr, *d_b1 = nullptr, *d_wh = nullptr, *d_bh = nullptr;
    uint16_t* d_w0x = nullptr;               // precision >= 1: FC1's weights as two bf16 planes [2][n0][F_stride] (hi, lo) for launch_fcx
    // staging for the host-pointer entry points
    uint8_t* d_in = nullptr;
    float* d_out = nullptr;
    // asynchronous host-pointer path (dan_forward_async / dan_wait): two slots, made on first use (async_init)
    struct Slot {
        dev::Pinned pin_in, pin_out;
        uint8_t* dev_in = nullptr;
        float* dev_out = nullptr;
        dev::Event ev_comp, ev_done;
        std::deque<dev::Event> ev_slice;         // one per conv chunk of a macro-batch: "this chunk's inputs are on the device"
        int64_t ticket = -1, n = 0;
        Outs dst{nullptr, nullptr, nullptr, nullptr, nullptr};
    } slot[2];
    dev::Stream s_h2d, s_comp, s_d2h;
    int64_t next_ticket = 0;
    // profiling: the pairs live in `events` for the handle's life and move between `event_pool` and the kernels' pending lists
    bool profiling = false;
    std::map<std::string, KernelStat> stats;
    std::deque<EventPair> events;
    std::vector<EventPair*> event_pool;
};

namespace {

template <class... A>
int fail(const dan_handle* h, int code, const char* fmt, A... a) { return capi::failf(h ? h->err : g_create_error, code, fmt, a...); }

// an extern "C" body: what it throws becomes code -4 and "<who>: <what()>" in the handle's error text (before a handle exists:
// in dan_create's)
template <class F>
int guarded(const dan_handle* h, const char* who, F&& body) { return capi::guarded(h ? h->err : g_create_error, who, std::forward<F>(body)); }

#define HIPCHK(h, call)                                                                          \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return fail(h, DAN_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

template <typename T>
int upload(dan_handle* h, T** p, const std::vector<T>& v) {
    HIPCHK(h, h->blocks.take(p, v.size(), false));
    HIPCHK(h, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return DAN_OK;
}

// body() between two events on s when profiling is on, counted under kernel k; body() alone when it is off
template <class F>
int timed(dan_handle* h, const char* k, hipStream_t s, F&& body) {
    if (!h->profiling) return body();
    EventPair* ev;
    if (!h->event_pool.empty()) { ev = h->event_pool.back(); h->event_pool.pop_back(); }
    else { h->events.emplace_back(); ev = &h->events.back(); }
    int rc = [&] {
        HIPCHK(h, ev->a.ensure()); HIPCHK(h, ev->b.ensure());
        HIPCHK(h, hipEventRecord(ev->a, s));
        if (int rb = body()) return rb;
        HIPCHK(h, hipEventRecord(ev->b, s));
        return (int)DAN_OK;
    }();
    if (rc) h->event_pool.push_back(ev); else h->stats[k].pending.push_back(ev);
    return rc;
}

int prof_collect(dan_handle* h, KernelStat& st) {
    for (EventPair* ev : st.pending) {
        HIPCHK(h, hipEventSynchronize(ev->b));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, ev->a, ev->b));
        st.ms += ms;
        st.launches += 1;
        h->event_pool.push_back(ev);
    }
    st.pending.clear();
    return 0;
}

// ---- one seam per kernel family (dan_config.precision) ------------------------------------------------------------------------
// One segment launch of one chunk, as the chunk loop sees it; a family's function below turns it into its kernel's arguments.
struct SegmentCall {
    int sg, ns;                              // segment, sites of the chunk
    Planes in;                               // the six input planes at the chunk's offset
    float *y_in, *y_out;                     // the previous segment's output and this one's (two buffers only where the window is split)
    float* tap;                              // null: the tap layer is not in this segment
    bool fold;                               // fp32 only: the read-axis pooling inside the segment kernel ...
    float* feat;                             // ... which writes the chunk's feature rows from the last segment
};

// the fields SegmentArgs, SegmentXArgs and SegmentPArgs name alike
template <class Args>
void fill_segment_common(Args& a, const dan_handle* h, const SegmentCall& q) {
    const dan_config& c = h->cfg;
    a.l_begin = h->seg_begin[q.sg]; a.l_end = h->seg_end[q.sg];
    a.n_layers = c.layers; a.dil_mid = c.dil_mid; a.dil_final = c.dil_final;
    a.res_mask = h->res_mask; a.has_hw = c.bottleneck > 0;
    a.R = c.reads; a.L = c.length;
    a.reads = q.in.p[0]; a.qual = q.in.p[1]; a.strand = q.in.p[2]; a.ref = q.in.p[3]; a.ref_mask = q.in.p[4]; a.var_mask = q.in.p[5];
    a.emb = h->d_emb; a.pe = h->d_pe;
    a.h_layer_stride = (long long)h->chunk * c.reads * c.length * HPAD;
    a.tap = q.tap; a.tap_layer = h->tap_layer;
    a.work = h->d_work; a.work_count = h->d_rowsrc ? h->d_work_count : nullptr;
}

int segment_fp32(dan_handle* h, const SegmentCall& q, hipStream_t s) {
    SegmentArgs a{};
    fill_segment_common(a, h, q);
    // one unit per read and y in place -- or, above MPOS columns, two units per read and y alternating between two buffers (a unit
    // reads the other unit's columns of the input while that one stores its output); dan_create checked that the units fit
    if (!plan_units(a, a.L, segment_halo(h->cfg, a.l_begin, a.l_end))) return fail(h, DAN_ERR_STATE, "unit plan failed for segment %d", q.sg);
    a.wl = h->d_wl; a.wino = h->wino; a.l0_tab = h->d_l0tab;
    a.y = q.y_in; a.y_out = q.y_out; a.pool = q.sg > 0 ? h->d_pool : nullptr; a.h = h->d_h;
    if (q.fold) {
        a.fold = 1; a.fold_scratch = h->d_fold;
        if (q.sg + 1 < h->n_segments) a.fold_pool = h->d_pool;
        else { a.fold_feat = q.feat; a.fold_feat_stride = h->F_stride; a.fold_C = h->cfg.c_final; }
    }
    launch_segment(a, q.ns, h->n_cus, s);
    return DAN_OK;
}

int segment_bf16x(dan_handle* h, const SegmentCall& q, hipStream_t s) {
    SegmentXArgs a{};
    fill_segment_common(a, h, q);
    if (!plan_units(a, a.L, segment_halo(h->cfg, a.l_begin, a.l_end))) return fail(h, DAN_ERR_STATE, "unit plan failed for segment %d", q.sg);   // (as in segment_fp32)
    a.wl = h->d_wlx;
    a.stagger = -1;                                          // (the launcher's own start offsets)
    a.y = (uint16_t*)q.y_in; a.y_out = (uint16_t*)q.y_out; a.pool = q.sg > 0 ? h->d_cp : nullptr; a.h = h->d_h;
    launch_segmentx(a, q.ns, h->n_cus, s);
    return DAN_OK;
}

int segment_bf16p(dan_handle* h, const SegmentCall& q, hipStream_t s) {
    SegmentPArgs a{};
    fill_segment_common(a, h, q);
    a.wl = h->d_wlp; a.wlr = h->d_wlr; a.form = h->cfg.bf16_form;
    a.y = (uint16_t*)h->d_y; a.pool = q.sg > 0 ? h->d_cp : nullptr; a.h = (uint16_t*)h->d_h;     // (one unit up to P_LMAX: y in place)
    launch_segmentp(a, q.ns, h->n_cus, s);
    return DAN_OK;
}

// the launchers of dan_kernels.h behind one signature per tail: y / h as const void* (fp32, bf16 or two bf16 planes)
typedef void ReadMeanFn(const void* y, float* pool, int n, int R, int L, const int* rs, hipStream_t s);
typedef void FinalPoolFn(const void* y, float* feat, long long fs, int n, int R, int L, int C, const int* rs, hipStream_t s);
typedef void HighwayFn(const void* hb, long long hls, const float* wc, long long wcls, const float* bc, float* feat, long long fs, int off, int n, int R, int L, int H, int nl, const int* rs, hipStream_t s);
void read_mean_f32(const void* y, float* pool, int n, int R, int L, const int* rs, hipStream_t s) { launch_read_mean((const float*)y, pool, n, R, L, rs, s); }
void read_mean_x(const void* y, float* pool, int n, int R, int L, const int* rs, hipStream_t s) { launch_read_meanx((const uint16_t*)y, pool, n, R, L, rs, s); }
void read_mean_16(const void* y, float* pool, int n, int R, int L, const int* rs, hipStream_t s) { launch_read_mean16((const uint16_t*)y, pool, n, R, L, rs, s); }
void final_pool_f32(const void* y, float* feat, long long fs, int n, int R, int L, int C, const int* rs, hipStream_t s) { launch_final_pool((const float*)y, feat, fs, n, R, L, C, rs, s); }
void final_pool_x(const void* y, float* feat, long long fs, int n, int R, int L, int C, const int* rs, hipStream_t s) { launch_final_poolx((const uint16_t*)y, feat, fs, n, R, L, C, rs, s); }
void final_pool_16(const void* y, float* feat, long long fs, int n, int R, int L, int C, const int* rs, hipStream_t s) { launch_final_pool16((const uint16_t*)y, feat, fs, n, R, L, C, rs, s); }
void highway_f32(const void* hb, long long hls, const float* wc, long long wcls, const float* bc, float* feat, long long fs, int off, int n, int R, int L, int H,
                 int nl, const int* rs, hipStream_t s) { launch_highway((const float*)hb, hls, wc, wcls, bc, feat, fs, off, n, R, L, H, nl, rs, s); }
void highway_16(const void* hb, long long hls, const float* wc, long long wcls, const float* bc, float* feat, long long fs, int off, int n, int R, int L, int H,
                int nl, const int* rs, hipStream_t s) { launch_highway16((const uint16_t*)hb, hls, wc, wcls, bc, feat, fs, off, n, R, L, H, nl, rs, s); }

// What the forward asks of a family, one row per precision; everything else in run_batches is the same for the three.
struct Family {
    int (*segment)(dan_handle*, const SegmentCall&, hipStream_t);
    ReadMeanFn* read_mean;
    FinalPoolFn* final_pool;
    HighwayFn* highway;                      // (reads dan_handle::d_hw: the compression weights in its order)
    bool conv_pool;                          // the read-mean enters the layer behind it as conv(pool) (launch_conv_pool), not inside the segment
    int elem_bytes;                          // bytes per element of y and h in HBM
    int y_copies;                            // buffers of y for windows above MPOS columns (two units per read: y out of place)
    // the reductions read the buffer the last segment wrote (false: always d_y).  This documents an invariant and switches nothing: a
    bool tails_follow_y;                     // family with one y buffer never splits a window, so that buffer IS d_y there
};
const Family FAMILIES[3] = {
    {segment_fp32, read_mean_f32, final_pool_f32, highway_f32, false, 4, 2, true},   // 0: fp32 MFMA (dan_kernels.hip)
    {segment_bf16x, read_mean_x, final_pool_x, highway_f32, true, 4, 2, true},       // 1: bf16x3 (dan_kernels_bf16x.hip): y as hi / lo bf16 planes, h fp32
    {segment_bf16p, read_mean_16, final_pool_16, highway_16, true, 2, 1, false},     // 2: plain bf16 (dan_kernels_bf16p.hip): y and h as bf16
};

// ---- dan_finalize's device half: what dan_pack.h packed, uploaded in a fixed order of allocations ------------------------------
int upload_packed(dan_handle* h, const Packed& pk) {
    const dan_config& c = h->cfg;
    const int n0 = c.fc_sizes[0];
    int rc = DAN_OK;
    if ((rc = upload(h, &h->d_emb, pk.emb->data)) || (rc = upload(h, &h->d_pe, pk.pe->data))) return rc;
    if (!pk.l0tab.empty() && (rc = upload(h, &h->d_l0tab, pk.l0tab))) return rc;
    if (!pk.wlp.empty() && ((rc = upload(h, &h->d_wlp, pk.wlp)) || (rc = upload(h, &h->d_wlr, pk.wlr)))) return rc;
    if (!pk.wc16.empty() && (rc = upload(h, &h->d_wc16, pk.wc16))) return rc;
    if (!pk.wlx.empty() && (rc = upload(h, &h->d_wlx, pk.wlx))) return rc;
    if (!pk.zero.empty() && ((rc = upload(h, &h->d_wpool, pk.wpool)) || (rc = upload(h, &h->d_zero, pk.zero)))) return rc;
    if ((rc = upload(h, &h->d_wl, pk.wl))) return rc;
    if (!pk.wc.empty() && ((rc = upload(h, &h->d_wc, pk.wc)) || (rc = upload(h, &h->d_bc, pk.bc)))) return rc;
    h->d_hw = h->d_wc16 ? h->d_wc16 : h->d_wc;
    if (pk.fc0) {                                            // fp32: the rows of fc.0 at the padded stride, zeros behind them
        HIPCHK(h, h->blocks.take(&h->d_w0, (size_t)n0 * h->F_stride, true));
        HIPCHK(h, hipMemcpy2D(h->d_w0, h->F_stride * sizeof(float), pk.fc0->data.data(), (size_t)h->F * sizeof(float),
                              (size_t)h->F * sizeof(float), n0, hipMemcpyHostToDevice));
    } else if ((rc = upload(h, &h->d_w0x, pk.w0x))) return rc;
    if ((rc = upload(h, &h->d_w1, pk.w1)) || (rc = upload(h, &h->d_b0, pk.b0)) || (rc = upload(h, &h->d_b1, pk.b1))) return rc;
    if ((rc = upload(h, &h->d_wh, pk.wh)) || (rc = upload(h, &h->d_bh, pk.bh))) return rc;
    return DAN_OK;
}

// activations / workspaces, sized for one chunk (conv) and one macro-batch (FC)
int alloc_workspaces(dan_handle* h) {
    const dan_config& c = h->cfg;
    const int L = c.length, R = c.reads, H = c.bottleneck, n1 = c.fc_sizes[1];
    const size_t read_floats = (size_t)L * CPAD;
    const size_t act_div = sizeof(float) / h->fam->elem_bytes;   // (bf16 y / h: half a float per element)
    dev::Blocks& b = h->blocks;
    HIPCHK(h, b.take(&h->d_y, (size_t)h->chunk * R * read_floats / act_div, false));
    if (h->split && h->fam->y_copies < 2) return fail(h, DAN_ERR_STATE, "a split window needs a family with two y buffers");
    if (h->split) HIPCHK(h, b.take(&h->d_y2, (size_t)h->chunk * R * read_floats, false));
    HIPCHK(h, b.take(&h->d_pool, (size_t)h->chunk * read_floats, false));
    if (!h->fold_why_not) HIPCHK(h, b.take(&h->d_fold, (size_t)(h->n_cus & ~7) * 2 * read_floats, false));
    if (h->fam->conv_pool && h->n_segments > 1) {
        HIPCHK(h, b.take(&h->d_cp, (size_t)h->chunk * read_floats, false));
        HIPCHK(h, b.take(&h->d_cols, (size_t)h->chunk * L * 3 * CPAD, false));
    }
    if (c.skip_empty_rows) {
        HIPCHK(h, b.take(&h->d_rowsrc, (size_t)h->chunk * R, false));     // int32 per pileup row
        HIPCHK(h, b.take(&h->d_work, (size_t)h->chunk * R + 4, false));
        h->d_work_count = h->d_work + (size_t)h->chunk * R;
    }
    if (H > 0) HIPCHK(h, b.take(&h->d_h, (size_t)c.layers * h->chunk * R * L * HPAD / act_div, false));
    HIPCHK(h, b.take(&h->d_feat, (size_t)h->max_batch * h->F_stride, false));
    HIPCHK(h, hipMemset(h->d_feat, 0, (size_t)h->max_batch * h->F_stride * sizeof(float)));
    HIPCHK(h, b.take(&h->d_hid0, (size_t)h->max_batch * h->n0_stride, false));
    HIPCHK(h, b.take(&h->d_hid1, (size_t)h->max_batch * n1, false));
    HIPCHK(h, hipMemset(h->d_hid0, 0, (size_t)h->max_batch * h->n0_stride * sizeof(float)));
    HIPCHK(h, b.take(&h->d_fc_ws, (size_t)2 * h->max_batch * c.fc_sizes[0], false));
    HIPCHK(h, b.take(&h->d_in, (size_t)h->max_batch * Planes(c, nullptr, 0).site_bytes(), false));
    HIPCHK(h, b.take(&h->d_out, (size_t)h->max_batch * OUT_TOTAL, false));
    return DAN_OK;
}

int create(const dan_config* cfg, dan_t** out) {
    if (!cfg || !out) return fail(nullptr, DAN_ERR_INVALID_ARG, "dan_create: null argument");
    *out = nullptr;
    const dan_config& c = *cfg;
    if (c.layers < 1 || c.layers > DAN_MAX_LAYERS) return fail(nullptr, DAN_ERR_INVALID_ARG, "layers must be in 1..%d", DAN_MAX_LAYERS);
    if (c.reads < 1) return fail(nullptr, DAN_ERR_INVALID_ARG, "reads must be >= 1");
    if (c.precision < 0 || c.precision > 2)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "precision %d unknown (0 = fp32 MFMA, 1 = bf16x3 split, 2 = bf16)", c.precision);
    // precisions 0 and 1 above MPOS columns: every read as two overlapping units (dan_kernels.h plan_units; checked per segment below)
    const int max_len = P_LMAX;
    if (c.length < 8 || c.length > max_len)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "length %d unsupported by the LDS-resident path at precision %d (8..%d)", c.length, c.precision, max_len);
    if (c.c_init < 1 || c.c_init > CPAD || c.c_final < 1 || c.c_final > CPAD)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "channel counts must be in 1..%d", CPAD);
    if (c.layers == 1 && c.c_init != c.c_final)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "a single conv layer needs init_conv_channels == final_conv_channels (model.py:214,257)");
    if (c.bottleneck < 0 || c.bottleneck > HPAD) return fail(nullptr, DAN_ERR_INVALID_ARG, "bottleneck must be in 0..%d", HPAD);
    if (c.dil_mid < 1 || c.dil_mid > HALO || c.dil_final < 1 || c.dil_final > HALO)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "dilations must be in 1..%d", HALO);
    if (c.fc_sizes[0] < 1 || c.fc_sizes[1] < 1) return fail(nullptr, DAN_ERR_INVALID_ARG, "fc_sizes must be positive");
    if (c.residual_start == 1 || c.residual_start < 0)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "Do not allow residuals starting at conv layer %d", c.residual_start);   // model.py:209
    if ((c.pool_layers_mask & 1u) || (c.pool_layers_mask >> c.layers))
        return fail(nullptr, DAN_ERR_INVALID_ARG, "pool layers must lie in 1..layers-1");
    // Winograd forms (dan_kernels.hip): fp32 path, and every conv after the first must have dilation 2
    const bool wino_ok = c.precision == 0 && (c.layers < 3 || c.dil_mid == 2) && (c.layers < 2 || c.dil_final == 2);
    if (c.conv_algo < 0 || c.conv_algo > 2) return fail(nullptr, DAN_ERR_INVALID_ARG, "conv_algo %d unknown (0 = auto, 1 = direct, 2 = winograd)", c.conv_algo);
    if (c.skip_empty_rows < 0 || c.skip_empty_rows > 1) return fail(nullptr, DAN_ERR_INVALID_ARG, "skip_empty_rows must be 0 or 1");
    if (c.bf16_form < 0 || c.bf16_form > 1) return fail(nullptr, DAN_ERR_INVALID_ARG, "bf16_form %d unknown (0 = eight waves, 1 = sixteen waves)", c.bf16_form);
    if (c.bf16_form != 0 && c.precision != 2) return fail(nullptr, DAN_ERR_INVALID_ARG, "bf16_form selects a form of the precision-2 kernel");
    if (c.conv_algo == 2 && !wino_ok)
        return fail(nullptr, DAN_ERR_INVALID_ARG, "conv_algo 2 (winograd) needs precision 0 and dilation 2 on every conv layer after the first");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || c.device_id < 0 || c.device_id >= ndev)
        return fail(nullptr, DAN_ERR_NO_DEVICE, "no HIP device %d (found %d): the DAN forward has no CPU path", c.device_id, ndev);
    std::unique_ptr<dan_handle> owner(new dan_handle());
    dan_handle* h = owner.get();
    h->cfg = c;
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c.device_id) == hipSuccess) h->n_cus = cus; }
    h->fold_why_not = c.precision != 0 ? "the in-segment pooling form exists for precision 0 only"
                    : c.length > MPOS ? "the in-segment pooling form needs one unit per read (windows up to 208 columns)"
                    : c.skip_empty_rows ? "the in-segment pooling form computes every row: not with skip_empty_rows"
                    : h->n_cus < 8 ? "the in-segment pooling form needs at least 8 compute units" : nullptr;
    h->last_pool_form = h->fold_why_not ? 1 : 2;
    h->max_batch = c.max_batch > 0 ? c.max_batch : 4096;
    if (c.chunk_sites > 0) {
        h->chunk = c.chunk_sites;
    } else {
        // default: the largest power-of-two chunk (<= the FC macro-batch) whose segment-boundary activations y and bottleneck
        // outputs h stay under 48 GB -- 288 GB of HBM per GPU: fewer, larger launches (2048 sites at 64 x 201: +1.7 % over 128) --
        // and under a third of what the device has FREE now (a shared or smaller device sizes down instead of failing in hipMalloc;
        // the feature matrix, FC workspaces and weights take their share of the rest)
        // (precision 2 keeps y and h as bf16: half the bytes per site, twice the sites per chunk -- 1024 at 128 x 301)
        const double elem = c.precision == 2 ? 2.0 : 4.0;
        const double y_copies = (c.precision != 2 && c.length > MPOS) ? 2.0 : 1.0;       // (two units per read: y out of place)
        const double per_site = (double)c.reads * c.length * (y_copies * CPAD + (double)c.layers * (c.bottleneck > 0 ? HPAD : 0)) * elem;
        double budget = 48e9;
        size_t free_b = 0, total_b = 0;
        // (hipMemGetInfo reports on the CURRENT device: switch for the question, then back -- dan_create leaves the calling
        // thread's device as it found it; the result depends on what else holds memory at this moment, so the choice is
        // reported by dan_query("chunk_sites") and measurements key on that, never on the default being a given number)
        int prev_dev = -1;
        (void)hipGetDevice(&prev_dev);
        if (hipSetDevice(c.device_id) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0)
            budget = std::min(budget, (double)free_b / 3.0);
        if (prev_dev >= 0 && prev_dev != c.device_id) (void)hipSetDevice(prev_dev);
        h->chunk_auto = true;
        int chunk = 128;
        while (chunk * 2 <= h->max_batch && (double)(chunk * 2) * per_site <= budget) chunk *= 2;
        while (chunk > 1 && (double)chunk * per_site > budget) chunk /= 2;
        h->chunk = chunk;
    }
    // the read-axis reductions put the chunk's site index in gridDim.y (limit 65 535): no chunk exceeds 32 768 sites,
    // whatever the caller or the automatic sizing asks for (results do not depend on the chunking)
    h->chunk = std::min(h->chunk, 32768);
    h->wino = wino_ok && c.conv_algo != 1;
    h->max_batch = ((h->max_batch + h->chunk - 1) / h->chunk) * h->chunk;
    h->F = feature_width(c);
    h->F_stride = pad16(h->F);
    h->n0_stride = (int)pad16(c.fc_sizes[0]);
    int b = 0;
    for (int l1 = 1; l1 <= c.layers; ++l1)
        if (l1 == c.layers || pool_after(c, l1)) { h->seg_begin.push_back(b); h->seg_end.push_back(l1); b = l1; }
    h->n_segments = (int)h->seg_begin.size();
    if (c.precision != 2 && c.length > MPOS) {
        // every segment's two units must fit the 208-row image: half the window + the segment's receptive-field radius
        for (int sg = 0; sg < h->n_segments; ++sg) {
            SegmentArgs probe{};
            const int halo = segment_halo(c, h->seg_begin[sg], h->seg_end[sg]);
            if (!plan_units(probe, c.length, halo))
                return fail(nullptr, DAN_ERR_INVALID_ARG, "length %d unsupported at precisions 0 and 1 with these dilations: layers %d..%d reach %d "
                            "columns sideways, half the window plus that exceeds the %d-column LDS image", c.length,
                            h->seg_begin[sg] + 1, h->seg_end[sg], halo, MPOS);
        }
        h->split = true;
    }
    *out = owner.release();
    return DAN_OK;
}

int set_tensor(dan_t* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (h->finalized) return fail(h, DAN_ERR_STATE, "dan_set_tensor('%s') after dan_finalize", name);
    Tensor t;
    t.shape.assign(shape, shape + ndim);
    for (auto s : t.shape)
        if (s < 0) return fail(h, DAN_ERR_SHAPE, "tensor '%s': negative dimension", name);
    t.data.assign(data, data + t.numel());
    h->tensors[name] = std::move(t);
    return DAN_OK;
}

// pack on the host (dan_pack.h), upload, allocate the workspaces
int finalize(dan_t* h) {
    if (h->finalized) return fail(h, DAN_ERR_STATE, "dan_finalize called twice");
    const dan_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device_id));
    h->fam = &FAMILIES[c.precision];
    const PackFamily pf{c.precision, h->fam->conv_pool, h->fam->highway == highway_16};
    Packed pk;
    int rc = pack_network(c, h->tensors, h->seg_begin, pf, &pk, h->err);
    if (rc) return rc;
    h->res_mask = pk.res_mask;
    if ((rc = upload_packed(h, pk)) || (rc = alloc_workspaces(h))) return rc;
    HIPCHK(h, hipDeviceSynchronize());
    h->tensors.clear();
    h->finalized = true;
    return DAN_OK;
}

// The in-segment pooling form gives a workgroup whole sites, so a chunk that does not deal evenly leaves compute units idle at
// its end: with W workgroups in 8 XCD slices the chunk takes ceil(ceil(ns / 8) / (W / 8)) site-times where the row form takes
// ns / W.  It is chosen when that loss is smaller than what the fold saves (FOLD_GAIN: measured, HISTORY.md).
constexpr double FOLD_GAIN = 0.013;
bool fold_deals_evenly(int ns, int n_cus) {
    const int W = n_cus & ~7;
    if (W < 8 || ns <= 0) return false;
    const int per = (ns + 7) / 8, rounds = (per + W / 8 - 1) / (W / 8);
    return (double)rounds * W / ns - 1.0 < FOLD_GAIN;
}

// feed (may be null): called in front of the k-th conv chunk's first launch; it brings that chunk's inputs onto the device (on a
// stream of its own) and hands back the event the compute stream waits for.  The asynchronous host path uploads a macro-batch
// chunk by chunk THROUGH this: chunk k's launches are queued before the host touches chunk k + 1, so the forward of chunk 0 starts
// after one chunk's staging and the staging of chunk k + 1 runs under chunk k's kernels.
struct ChunkFeed {
    int (*fn)(void* ctx, int64_t first_site, int n_sites, int64_t k, hipEvent_t* ready);
    void* ctx;
};

// what every forward checks first: the handle is final, the site count in range (max_sites < 0: any), no plane missing
int check_forward(const dan_handle* h, const char* entry, int64_t n_sites, int64_t max_sites, const Planes& in) {
    if (!h->finalized) return fail(h, DAN_ERR_STATE, "%s before dan_finalize", entry);
    if (max_sites >= 0 && (n_sites < 0 || n_sites > max_sites))
        return fail(h, DAN_ERR_INVALID_ARG, "%s takes 0..max_batch (%d) sites per call, got %lld", entry, (int)max_sites, (long long)n_sites);
    if (n_sites < 0) return fail(h, DAN_ERR_INVALID_ARG, "negative site count");
    if (n_sites > 0 && !in.complete()) return fail(h, DAN_ERR_INVALID_ARG, "null input plane");
    return DAN_OK;
}

// the forward of n_sites > 0 sites on device buffers, enqueued on s: macro-batches of max_batch sites (FC), chunks of `chunk` (conv)
int run_batches(dan_t* h, const Planes& in, int64_t n_sites, const Outs& out, hipStream_t s, const ChunkFeed* feed) {
    const dan_config& c = h->cfg;
    const Family& fam = *h->fam;
    HIPCHK(h, hipSetDevice(c.device_id));
    const int L = c.length, R = c.reads, H = c.bottleneck;
    const long long h_layer_stride = (long long)h->chunk * R * L * HPAD;
    for (int64_t mb = 0; mb < n_sites; mb += h->max_batch) {
        const int nb = (int)std::min<int64_t>(h->max_batch, n_sites - mb);
        for (int c0 = 0; c0 < nb; c0 += h->chunk) {
            const int ns = std::min(h->chunk, nb - c0);
            const int64_t g0 = mb + c0;                      // first site of the chunk in the caller's arrays
            const Planes cin = in.at(g0);
            if (feed) {
                hipEvent_t ready;
                int rcf = feed->fn(feed->ctx, g0, ns, g0 / h->chunk, &ready); if (rcf) return rcf;
                HIPCHK(h, hipStreamWaitEvent(s, ready, 0));
            }
            int rc = DAN_OK;
            if (h->d_rowsrc) {
                rc = timed(h, "row_map", s, [&] {
                    launch_row_map(cin.p[0], cin.p[1], cin.p[2], h->d_rowsrc, h->d_work, h->d_work_count, ns, R, L, s);
                    return (int)DAN_OK;
                });
                if (rc) return rc;
            }
            const bool fold = !h->fold_why_not && (h->pool_form == 2 || (h->pool_form == 0 && fold_deals_evenly(ns, h->n_cus)));
            float* const feat = h->d_feat + (size_t)c0 * h->F_stride;
            float* y_seg = h->d_y;                           // where the segment just launched left its output
            for (int sg = 0; sg < h->n_segments; ++sg) {
                float* const y_in = y_seg;                   // the previous segment's output
                if (h->split) y_seg = (y_seg == h->d_y) ? h->d_y2 : h->d_y;
                const bool tap_here = h->tap_layer >= 0 && ((h->tap_layer == 0 && sg == 0) ||
                                                            (h->tap_layer > h->seg_begin[sg] && h->tap_layer <= h->seg_end[sg]));
                const SegmentCall q{sg, ns, cin, y_in, y_seg, tap_here ? h->d_tap : nullptr, fold, feat};
                if ((rc = timed(h, "conv_segment", s, [&] { return fam.segment(h, q, s); }))) return rc;
                if (fold) {
                    HIPCHK(h, hipGetLastError());
                } else if (sg + 1 < h->n_segments) {
                    rc = timed(h, "pool", s, [&] {
                        fam.read_mean(fam.tails_follow_y ? y_seg : h->d_y, h->d_pool, ns, R, L, h->d_rowsrc, s);
                        if (fam.conv_pool) {
                            const int ln = h->seg_begin[sg + 1];                      // 0-based layer behind the pool: its dilation
                            launch_conv_pool(h->d_pool, h->d_wpool + (size_t)(sg + 1) * CPAD * 3 * CPAD, h->d_zero, h->d_cols, h->d_cp, ns, L,
                                             ln + 1 < c.layers ? c.dil_mid : c.dil_final, s);
                        }
                        return (int)DAN_OK;
                    });
                    if (rc) return rc;
                    HIPCHK(h, hipGetLastError());            // a refused launch must not let garbage flow on to the FC
                }
            }
            if (!fold) {                                     // (in-segment form: the last segment has written the pooled blocks)
                rc = timed(h, "pool", s, [&] {
                    fam.final_pool(fam.tails_follow_y ? y_seg : h->d_y, feat, h->F_stride, ns, R, L, c.c_final, h->d_rowsrc, s);
                    return (int)DAN_OK;
                });
                if (rc) return rc;
                HIPCHK(h, hipGetLastError());
            }
            if (H > 0) {
                rc = timed(h, "highway", s, [&] {
                    fam.highway(h->d_h, h_layer_stride, h->d_hw, (long long)hw_layer_floats(L), h->d_bc, feat, h->F_stride,
                                2 * c.c_final * L, ns, R, L, H, c.layers, h->d_rowsrc, s);
                    return (int)DAN_OK;
                });
                if (rc) return rc;
            }
            h->last_chunk_sites = ns;
            h->last_pool_form = fold ? 2 : 1;
        }
        const Outs o = out.at(mb);
        int rc = timed(h, "fc", s, [&] {
            if (h->d_w0x)
                launch_fcx(h->d_feat, h->F_stride, h->d_w0x, h->F_stride, (long long)c.fc_sizes[0] * h->F_stride, h->d_b0, h->d_hid0, h->n0_stride,
                           nb, c.fc_sizes[0], (int)h->F_stride, 1, s, h->d_fc_ws, (long long)2 * h->max_batch * c.fc_sizes[0]);
            else
                launch_fc(h->d_feat, h->F_stride, h->d_w0, h->F_stride, h->d_b0, h->d_hid0, h->n0_stride, nb, c.fc_sizes[0],
                          (int)h->F_stride, 1, s, h->d_fc_ws, (long long)2 * h->max_batch * c.fc_sizes[0]);
            launch_fc(h->d_hid0, h->n0_stride, h->d_w1, h->n0_stride, h->d_b1, h->d_hid1, c.fc_sizes[1], nb, c.fc_sizes[1],
                      h->n0_stride, 1, s);
            launch_heads(h->d_hid1, c.fc_sizes[1], h->d_wh, h->d_bh, nb, o.p[0], o.p[1], o.p[2], o.p[3], o.p[4], s);
            return (int)DAN_OK;
        });
        if (rc) return rc;
        h->last_batch = nb;
    }
    HIPCHK(h, hipGetLastError());
    return DAN_OK;
}

// synchronous forward on host buffers: a macro-batch at a time through the handle's staging blocks
int forward_host(dan_t* h, const Planes& in, int64_t n_sites, const Outs& out) {
    if (h->slot[0].ticket >= 0 || h->slot[1].ticket >= 0)      // (the workspaces are shared and the streams differ)
        return fail(h, DAN_ERR_STATE, "dan_forward while asynchronous batches are in flight: dan_wait for them first");
    const dan_config& c = h->cfg;
    HIPCHK(h, hipSetDevice(c.device_id));
    for (int64_t mb = 0; mb < n_sites; mb += h->max_batch) {
        const size_t nb = (size_t)std::min<int64_t>(h->max_batch, n_sites - mb);
        const Planes src = in.at(mb), d_in(c, h->d_in, nb);
        for (int i = 0; i < 6; ++i) HIPCHK(h, hipMemcpy((void*)d_in.p[i], src.p[i], nb * src.per_site[i], hipMemcpyHostToDevice));
        const Outs d_out(h->d_out, nb), dst = out.at(mb);
        int rc = run_batches(h, d_in, (int64_t)nb, d_out, nullptr, nullptr);
        if (rc) return rc;
        HIPCHK(h, hipDeviceSynchronize());
        for (int i = 0; i < 5; ++i)
            if (dst.p[i]) HIPCHK(h, hipMemcpy(dst.p[i], d_out.p[i], nb * OUT_W[i] * sizeof(float), hipMemcpyDeviceToHost));
    }
    return DAN_OK;
}

// the asynchronous path's streams, slots and events: each made once, so a set that a failed call left half-made is completed by
// the next call and freed with the handle
int async_init(dan_handle* h) {
    const size_t in_bytes = (size_t)h->max_batch * Planes(h->cfg, nullptr, 0).site_bytes(), out_floats = (size_t)h->max_batch * OUT_TOTAL;
    HIPCHK(h, h->s_h2d.ensure());
    HIPCHK(h, h->s_comp.ensure());
    HIPCHK(h, h->s_d2h.ensure());
    for (auto& sl : h->slot) {
        if (!sl.pin_in.get()) HIPCHK(h, sl.pin_in.alloc(in_bytes));
        if (!sl.pin_out.get()) HIPCHK(h, sl.pin_out.alloc(out_floats * sizeof(float)));
        if (!sl.dev_in) HIPCHK(h, h->blocks.take(&sl.dev_in, in_bytes, false));
        if (!sl.dev_out) HIPCHK(h, h->blocks.take(&sl.dev_out, out_floats, false));
        HIPCHK(h, sl.ev_comp.ensure(hipEventDisableTiming));
        HIPCHK(h, sl.ev_done.ensure(hipEventDisableTiming));
        while (sl.ev_slice.size() < (size_t)(h->max_batch + h->chunk - 1) / h->chunk) sl.ev_slice.emplace_back();
        for (auto& e : sl.ev_slice) HIPCHK(h, e.ensure(hipEventDisableTiming));
    }
    return DAN_OK;
}

// One conv chunk of an asynchronous batch: caller's pageable planes -> the slot's pinned mirror -> the device, on the copy stream.
// The mirror is filled by up to four threads (one core moves pageable memory at 5-10 GB/s: 118 MB per chunk at 128 x 301).  Nothing
// here allocates: a fixed table of pieces and of threads; a thread that cannot be started (std::system_error) leaves its pieces to
// the calling thread.
struct AsyncStage {
    dan_handle* h; dan_handle::Slot* sl;
    Planes src;                              // the caller's planes
    size_t off[6];                           // where the batch's planes start in the slot's staging blocks
};

int stage_chunk(void* ctx, int64_t first_site, int n_sites, int64_t k, hipEvent_t* ready) {
    AsyncStage& st = *static_cast<AsyncStage*>(ctx);
    dan_handle* h = st.h;
    dan_handle::Slot& sl = *st.sl;
    if (k < 0 || (size_t)k >= sl.ev_slice.size()) return fail(h, DAN_ERR_STATE, "chunk %lld outside the slot's event table", (long long)k);
    const size_t ns = (size_t)n_sites;
    const Planes src = st.src.at(first_site);
    size_t off[6];
    for (int i = 0; i < 6; ++i) off[i] = st.off[i] + (size_t)first_site * src.per_site[i];
    constexpr int MAX_THR = 4;
    struct Piece { uint8_t* dst; const uint8_t* src; size_t n; };
    Piece pieces[3 * MAX_THR + 3];
    int n_pieces = 0;
    const int n_thr = ns * src.site_bytes() >= ((size_t)32 << 20) ? MAX_THR : 1;
    for (int i = 0; i < 6; ++i) {
        const size_t n = ns * src.per_site[i];
        const int parts = (i < 3) ? n_thr : 1;                   // the three read planes are the bytes; the site planes ride with thread 0
        for (int t = 0; t < parts; ++t) {
            const size_t a0 = n * t / parts, a1 = n * (t + 1) / parts;
            pieces[n_pieces++] = {sl.pin_in.get() + off[i] + a0, src.p[i] + a0, a1 - a0};
        }
    }
    // pieces 0 .. 3 n_thr - 1 are the read planes' parts (piece j belongs to thread j % n_thr), the rest the site planes
    std::thread workers[MAX_THR];
    bool started[MAX_THR] = {false, false, false, false};
    const Piece* pc = pieces;
    for (int t = 1; t < n_thr; ++t) {
        try {
            workers[t] = std::thread([pc, t, n_thr] { for (int j = t; j < 3 * n_thr; j += n_thr) memcpy(pc[j].dst, pc[j].src, pc[j].n); });
            started[t] = true;
        } catch (...) {}
    }
    for (int j = 0; j < n_pieces; ++j)
        if (j >= 3 * n_thr || !started[j % n_thr]) memcpy(pieces[j].dst, pieces[j].src, pieces[j].n);
    for (int t = 1; t < n_thr; ++t) if (started[t]) workers[t].join();
    for (int i = 0; i < 6; ++i)
        HIPCHK(h, hipMemcpyAsync(sl.dev_in + off[i], sl.pin_in.get() + off[i], ns * src.per_site[i], hipMemcpyHostToDevice, h->s_h2d));
    HIPCHK(h, hipEventRecord(sl.ev_slice[(size_t)k], h->s_h2d));
    *ready = sl.ev_slice[(size_t)k];
    return DAN_OK;
}

// everything an asynchronous batch of nb > 0 sites puts on the three streams
int enqueue_batch(dan_handle* h, dan_handle::Slot& sl, const Planes& in, size_t nb) {
    AsyncStage st{h, &sl, in, {}};
    in.offsets(nb, st.off);
    const ChunkFeed feed{stage_chunk, &st};
    int rc = run_batches(h, Planes(h->cfg, sl.dev_in, nb), (int64_t)nb, Outs(sl.dev_out, nb), h->s_comp, &feed);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(sl.ev_comp, h->s_comp));
    HIPCHK(h, hipStreamWaitEvent(h->s_d2h, sl.ev_comp, 0));
    HIPCHK(h, hipMemcpyAsync(sl.pin_out.get(), sl.dev_out, nb * OUT_TOTAL * sizeof(float), hipMemcpyDeviceToHost, h->s_d2h));
    HIPCHK(h, hipEventRecord(sl.ev_done, h->s_d2h));
    return DAN_OK;
}

int forward_async(dan_t* h, const Planes& in, int64_t n_sites, const Outs& out, int64_t* ticket) {
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    int rc = async_init(h);
    if (rc) return rc;
    dan_handle::Slot& sl = h->slot[h->next_ticket & 1];
    if (sl.ticket >= 0)
        return fail(h, DAN_ERR_STATE, "two batches are already in flight: dan_wait(%lld) first", (long long)sl.ticket);
    if (n_sites > 0 && (rc = enqueue_batch(h, sl, in, (size_t)n_sites))) {
        // The slot stays free, so nothing of this batch may still be running when the next call fills the slot's staging blocks:
        // wait for what was queued.  h->err keeps the text of the failure.
        (void)hipStreamSynchronize(h->s_h2d);
        (void)hipStreamSynchronize(h->s_comp);
        (void)hipStreamSynchronize(h->s_d2h);
        return rc;
    }
    sl.ticket = h->next_ticket++;
    sl.n = n_sites;
    sl.dst = out;
    *ticket = sl.ticket;
    return DAN_OK;
}

int wait(dan_t* h, int64_t ticket) {
    dan_handle::Slot& sl = h->slot[ticket & 1];
    if (ticket < 0 || sl.ticket != ticket) return fail(h, DAN_ERR_STATE, "dan_wait(%lld): no such batch in flight", (long long)ticket);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    const size_t nb = (size_t)sl.n;
    if (nb) {
        HIPCHK(h, hipEventSynchronize(sl.ev_done));
        const Outs src((float*)sl.pin_out.get(), nb);
        for (int i = 0; i < 5; ++i)
            if (sl.dst.p[i]) memcpy(sl.dst.p[i], src.p[i], nb * OUT_W[i] * sizeof(float));
    }
    sl.ticket = -1;
    return DAN_OK;
}

int query(const dan_t* h, const char* what, int64_t* v) {
    const std::string w(what);
    if (w == "feature_width") *v = h->F;
    else if (w == "feature_stride") *v = h->F_stride;
    else if (w == "chunk_sites") *v = h->chunk;
    else if (w == "chunk_sites_auto") *v = h->chunk_auto ? 1 : 0;
    else if (w == "max_batch") *v = h->max_batch;
    else if (w == "cpad") *v = CPAD;
    else if (w == "layer_stride") *v = LAYER_STRIDE;       // floats per layer of the "wl" buffer, and its two Winograd blocks
    else if (w == "wino_f23_offset") *v = WW_OFF;
    else if (w == "wino_f43_offset") *v = W43_OFF;
    else if (w == "tap_sites") *v = h->last_chunk_sites;
    else if (w == "segments") *v = h->n_segments;
    else if (w == "bf16_pingpong") *v = h->fam == &FAMILIES[2] ? 1 : 0;         // (0 before dan_finalize, as ever)
    else if (w == "bf16x3_split_kernel") *v = h->fam == &FAMILIES[1] ? 1 : 0;
    else if (w == "hidden0_stride") *v = h->n0_stride;
    else if (w == "pool_form") *v = h->last_pool_form;
    else return fail(h, DAN_ERR_INVALID_ARG, "dan_query: unknown key '%s'", what);
    return DAN_OK;
}

// *copied = the floats written to dst
int read_buffer(dan_t* h, const char* name, float* dst, int64_t capacity, int64_t* copied) {
    if (!h->finalized) return fail(h, DAN_ERR_STATE, "dan_read_buffer before dan_finalize");
    const dan_config& c = h->cfg;
    const std::string w(name);
    const float* src = nullptr;
    int64_t n = 0;
    if (w == "tap") { if (!h->d_tap) return fail(h, DAN_ERR_STATE, "no tap was requested"); src = h->d_tap; n = (int64_t)h->last_chunk_sites * c.reads * c.length * CPAD; }
    else if (w == "feature") { src = h->d_feat; n = h->last_batch * h->F_stride; }
    else if (w == "hidden0") { src = h->d_hid0; n = h->last_batch * h->n0_stride; }
    else if (w == "hidden1") { src = h->d_hid1; n = h->last_batch * c.fc_sizes[1]; }
    else if (w == "wl") {                    // the fp32 family's packed weight blocks, [layer][LAYER_STRIDE] (dan_kernels.h)
        if (!h->d_wl) return fail(h, DAN_ERR_STATE, "dan_read_buffer('wl'): this precision keeps no fp32 weight blocks");
        src = h->d_wl; n = (int64_t)c.layers * LAYER_STRIDE;
    }
    else if (w == "pool") { src = h->d_pool; n = (int64_t)h->last_chunk_sites * c.length * CPAD; }
    else if (w == "h") {
        // bottleneck outputs of the last chunk, [layer][site][read][L][HPAD] (layer stride = the chunk's capacity); bf16 on the
        // ping-pong kernel: widened here
        if (!h->d_h) return fail(h, DAN_ERR_STATE, "the network has no highway bottleneck");
        const int64_t per_layer = (int64_t)h->last_chunk_sites * c.reads * c.length * HPAD;
        const int64_t stride = (int64_t)h->chunk * c.reads * c.length * HPAD;
        if (per_layer == 0) return fail(h, DAN_ERR_STATE, "dan_read_buffer('h') before the first forward");
        if (capacity < per_layer)
            return fail(h, DAN_ERR_INVALID_ARG, "dan_read_buffer('h'): capacity %lld is less than one layer (%lld floats)", (long long)capacity,
                        (long long)per_layer);
        n = std::min<int64_t>(per_layer * c.layers, capacity) / per_layer * per_layer;
        HIPCHK(h, hipSetDevice(c.device_id));
        HIPCHK(h, hipDeviceSynchronize());
        const bool h_bf16 = h->fam->elem_bytes == 2;
        std::vector<uint16_t> tmp(h_bf16 ? (size_t)per_layer : 0);
        for (int64_t l = 0; l * per_layer < n; ++l) {
            if (h_bf16) {
                HIPCHK(h, hipMemcpy(tmp.data(), (const uint16_t*)h->d_h + l * stride, (size_t)per_layer * 2, hipMemcpyDeviceToHost));
                for (int64_t i = 0; i < per_layer; ++i) dst[l * per_layer + i] = bf16_float(tmp[(size_t)i]);
            } else {
                HIPCHK(h, hipMemcpy(dst + l * per_layer, h->d_h + l * stride, (size_t)per_layer * sizeof(float), hipMemcpyDeviceToHost));
            }
        }
        *copied = n;
        return DAN_OK;
    }
    else return fail(h, DAN_ERR_INVALID_ARG, "dan_read_buffer: unknown buffer '%s'", name);
    n = std::min(n, capacity);
    HIPCHK(h, hipSetDevice(c.device_id));
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, hipMemcpy(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    *copied = n;
    return DAN_OK;
}

}  // namespace

extern "C" {

int dan_abi_version(void) { return DAN_ABI_VERSION; }

#ifndef DAN_SOURCE_HASH
#define DAN_SOURCE_HASH "unknown"
#endif
const char* dan_source_hash(void) { return DAN_SOURCE_HASH; }

const char* dan_last_error(const dan_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int dan_create(const dan_config* cfg, dan_t** out) {
    return guarded(nullptr, "dan_create", [&] { return create(cfg, out); });
}

int dan_set_tensor(dan_t* h, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!h || !name || !data || (ndim > 0 && !shape) || ndim < 0 || ndim > 8)
        return fail(h, DAN_ERR_INVALID_ARG, "dan_set_tensor: bad argument");
    return guarded(h, "dan_set_tensor", [&] { return set_tensor(h, name, data, shape, ndim); });
}

int dan_finalize(dan_t* h) {
    if (!h) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_finalize", [&] { return finalize(h); });
}

void dan_destroy(dan_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device_id);
    (void)hipDeviceSynchronize();
    delete h;
}

int dan_forward_device(dan_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, const uint8_t* ref,
                       const uint8_t* ref_mask, const uint8_t* var_mask, int64_t n_sites, float* bin_logits,
                       float* vt_logits, float* vt_prob, float* bp, float* aux, void* stream) {
    if (!h) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_forward_device", [&] {
        const Planes in(h->cfg, reads, qual, strand, ref, ref_mask, var_mask);
        const int rc = check_forward(h, "dan_forward", n_sites, -1, in);
        if (rc || n_sites == 0) return rc;
        return run_batches(h, in, n_sites, Outs(bin_logits, vt_logits, vt_prob, bp, aux), (hipStream_t)stream, nullptr);
    });
}

int dan_forward_aux(dan_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, const uint8_t* ref,
                    const uint8_t* ref_mask, const uint8_t* var_mask, int64_t n_sites, float* bin_logits,
                    float* vt_logits, float* vt_prob, float* bp, float* aux) {
    if (!h) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_forward", [&] {
        const Planes in(h->cfg, reads, qual, strand, ref, ref_mask, var_mask);
        const int rc = check_forward(h, "dan_forward", n_sites, -1, in);
        if (rc || n_sites == 0) return rc;
        return forward_host(h, in, n_sites, Outs(bin_logits, vt_logits, vt_prob, bp, aux));
    });
}

int dan_forward(dan_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, const uint8_t* ref,
                const uint8_t* ref_mask, const uint8_t* var_mask, int64_t n_sites, float* bin_logits, float* vt_logits,
                float* vt_prob, float* bp) {
    return dan_forward_aux(h, reads, qual, strand, ref, ref_mask, var_mask, n_sites, bin_logits, vt_logits, vt_prob, bp, nullptr);
}

int dan_forward_async(dan_t* h, const uint8_t* reads, const uint8_t* qual, const uint8_t* strand, const uint8_t* ref,
                      const uint8_t* ref_mask, const uint8_t* var_mask, int64_t n_sites, float* bin_logits,
                      float* vt_logits, float* vt_prob, float* bp, float* aux, int64_t* ticket) {
    if (!h || !ticket) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_forward_async", [&] {
        const Planes in(h->cfg, reads, qual, strand, ref, ref_mask, var_mask);
        const int rc = check_forward(h, "dan_forward_async", n_sites, h->max_batch, in);
        return rc ? rc : forward_async(h, in, n_sites, Outs(bin_logits, vt_logits, vt_prob, bp, aux), ticket);
    });
}

int dan_wait(dan_t* h, int64_t ticket) {
    if (!h) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_wait", [&] { return wait(h, ticket); });
}

int dan_set_tap(dan_t* h, int32_t layer) {
    if (!h) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_set_tap", [&] {
        if (layer < -1 || layer > h->cfg.layers) return fail(h, DAN_ERR_INVALID_ARG, "tap layer %d out of range", layer);
        if (layer >= 0 && !h->d_tap) {
            if (!h->finalized) return fail(h, DAN_ERR_STATE, "dan_set_tap before dan_finalize");
            HIPCHK(h, hipSetDevice(h->cfg.device_id));
            HIPCHK(h, h->blocks.take(&h->d_tap, (size_t)h->chunk * h->cfg.reads * h->cfg.length * CPAD, false));
        }
        h->tap_layer = layer;
        return (int)DAN_OK;
    });
}

int dan_set_pool_form(dan_t* h, int32_t form) {
    if (!h) return DAN_ERR_INVALID_ARG;
    if (form < 0 || form > 2) return fail(h, DAN_ERR_INVALID_ARG, "pool form %d: 0 = automatic, 1 = separate kernels, 2 = in-segment", form);
    if (form == 2 && h->fold_why_not) return fail(h, DAN_ERR_INVALID_ARG, "pool form 2 refused: %s", h->fold_why_not);
    h->pool_form = form;
    h->last_pool_form = (form == 1 || h->fold_why_not) ? 1 : 2;
    return DAN_OK;
}

int64_t dan_query(const dan_t* h, const char* what) {
    if (!h || !what) return DAN_ERR_INVALID_ARG;
    int64_t v = 0;
    const int rc = guarded(h, "dan_query", [&] { return query(h, what, &v); });
    return rc ? rc : v;
}

int64_t dan_read_buffer(dan_t* h, const char* name, float* dst, int64_t capacity) {
    if (!h || !name || !dst || capacity < 0) return DAN_ERR_INVALID_ARG;
    int64_t n = 0;
    const int rc = guarded(h, "dan_read_buffer", [&] { return read_buffer(h, name, dst, capacity, &n); });
    return rc ? rc : n;
}

int dan_profile_enable(dan_t* h, int32_t on) {
    if (!h) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_profile_enable", [&] {
        h->profiling = on != 0;
        for (auto& kv : h->stats) {
            int rc = prof_collect(h, kv.second);
            if (rc) return rc;
            kv.second.launches = 0;
            kv.second.ms = 0.0;
        }
        return (int)DAN_OK;
    });
}

int dan_kernel_stats(dan_t* h, const char* kernel, int64_t* launches, double* total_ms) {
    if (!h || !kernel) return DAN_ERR_INVALID_ARG;
    return guarded(h, "dan_kernel_stats", [&] {
        KernelStat& st = h->stats[kernel];
        int rc = prof_collect(h, st);
        if (rc) return rc;
        if (launches) *launches = st.launches;
        if (total_ms) *total_ms = st.ms;
        return (int)DAN_OK;
    });
}

}  // extern "C"
