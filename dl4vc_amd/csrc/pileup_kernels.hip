// Kernels of libdl4vc_pileup.so.  dan_pileup.cpp::encode_one is the specification; the comments name its steps.
//
// resolve_records: one thread per record -- Rec::resolve (query position, deletion / skip, merged indel length for every
// reference position of the record), the name:sequence hash and the '=' flag.
// location_status: the status rule of one location, shared by the two kernels below.
// census_locations: one workgroup per location -- location_status and one status byte, no plane (pg_census).
// encode_locations: one workgroup per location -- the track filter, the duplicate-key check (LDS hash table), coverage and
// the longest capped insertion per position (LDS atomics), the column map (a serial scan over <= MAX_POS positions), then
// per track the three "has a nonzero cell inside the crop" bits, the trim / centre arithmetic of finish_record and the
// rendering of the kept rows straight into the record planes.  Rows are never materialised at full width: a row's cells are
// enumerated and clipped to the crop [clo, chi), and the strand-pad rule needs only whether the row has a non-deleted base.
#include "pileup_device.h"

namespace pg {
namespace {

constexpr uint8_t START = 6, END = 7, NOINSERT = 8, STRAND_LOWER = 1, STRAND_UPPER = 2, TOK_GAP = 5,
                  TOK_N = 5;
enum { CMATCH, CINS, CDEL, CREF_SKIP, CSOFT_CLIP, CHARD_CLIP, CPADOP, CEQUAL, CDIFF };
__device__ inline bool is_aligned(int op) { return op == CMATCH || op == CEQUAL || op == CDIFF; }
__device__ inline bool is_refop(int op) { return is_aligned(op) || op == CDEL || op == CREF_SKIP; }

// BAM 4-bit codes "=ACMGRSVTWYHKDBN" -> tokens of the converter's table; '=' has none
__constant__ uint8_t SEQ_TOK[16] = {REF_UNKNOWN, 1, 4, 9, 3, 9, 9, 9, 2, 9, 9, 9, 9, 9, 9, 5};
__constant__ char SEQ_CHAR[16] = {'=', 'A', 'C', 'M', 'G', 'R', 'S', 'V', 'T', 'W', 'Y', 'H', 'K', 'D', 'B', 'N'};

__device__ inline uint32_t load_u32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ inline int seq_code(const uint8_t* r, const Rec& m, int qp) {
    const uint8_t b = r[m.seq_off + (qp >> 1)];
    return (qp & 1) ? (b & 0xf) : (b >> 4);
}

__global__ void __launch_bounds__(BLOCK) resolve_records(const uint8_t* __restrict__ buf, Rec* __restrict__ recs, int32_t n,
                                                        int32_t* __restrict__ qpos, int32_t* __restrict__ indel,
                                                        uint8_t* __restrict__ isdel) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    Rec m = recs[i];
    const uint8_t* r = buf + m.off;
    // name:sequence key (the duplicate check of process_tracks); hash equality is only ever used to decline
    uint64_t h = 14695981039346656037ull;
    auto mix = [&](uint8_t c) { h ^= c; h *= 1099511628211ull; };
    for (uint32_t k = 0; k + 1 < m.l_name; ++k) mix(r[32 + k]);
    mix(':');
    bool eq = false;
    for (int k = 0; k < m.l_seq; ++k) {
        const int c = seq_code(r, m, k);
        eq |= c == 0;
        mix((uint8_t)SEQ_CHAR[c]);
    }
    m.hash = h ? h : 1;
    if (eq) m.bits |= R_EQ;
    recs[i].hash = m.hash;
    recs[i].bits = m.bits;
    // Rec::resolve
    int32_t* Qp = qpos + m.res;
    int32_t* Id = indel + m.res;
    uint8_t* Dl = isdel + m.res;
    const uint8_t* cig = r + m.cigar_off;
    const int nc = (int)m.n_cig;
    int x = 0, y = 0;
    for (int k = 0; k < nc; ++k) {
        const uint32_t c = load_u32(cig + 4 * k);
        const int op = c & 0xf, l = (int)(c >> 4);
        if (is_aligned(op)) {
            for (int j = 0; j < l; ++j) { Qp[x + j] = y + j; Id[x + j] = 0; Dl[x + j] = 0; }
            x += l; y += l;
        } else if (op == CDEL || op == CREF_SKIP) {
            for (int j = 0; j < l; ++j) { Qp[x + j] = y; Id[x + j] = 0; Dl[x + j] = 1; }
            x += l;
        } else if (op == CINS || op == CSOFT_CLIP) {
            y += l;
        }
        if (is_refop(op) && x > 0 && k + 1 < nc) {
            const uint32_t c2 = load_u32(cig + 4 * (k + 1));
            const int op2 = c2 & 0xf, l2 = (int)(c2 >> 4);
            int v = 0;
            if (op2 == CDEL && op != CDEL) {
                v = -l2;
                for (int j = k + 2; j < nc; ++j) {
                    const uint32_t c3 = load_u32(cig + 4 * j);
                    if ((int)(c3 & 0xf) != CDEL) break;
                    v -= (int)(c3 >> 4);
                }
            } else if (op2 == CINS) {
                v = l2;
                for (int j = k + 2; j < nc; ++j) {
                    const uint32_t c3 = load_u32(cig + 4 * j);
                    const int op3 = c3 & 0xf;
                    if (op3 == CINS) v += (int)(c3 >> 4);
                    else if (op3 != CPADOP) break;
                }
            } else if (op2 == CPADOP && k + 2 < nc) {
                for (int j = k + 2; j < nc; ++j) {
                    const uint32_t c3 = load_u32(cig + 4 * j);
                    const int op3 = c3 & 0xf;
                    if (op3 == CINS) v += (int)(c3 >> 4);
                    else if (is_refop(op3)) break;
                }
            }
            Id[x - 1] = v;
        }
    }
}

// What one workgroup knows about its location once the column map exists.
struct Ctx {
    const uint8_t* buf;
    const int32_t *qpos, *indel;
    const uint8_t* isdel;
    const int32_t *col, *prev, *longest;
    int32_t s0, stop, ci, cap, cap_ci;
};

// Every cell encode_one writes for one track, in its order: f(column, base token, quality, strand, has_quality_and_strand).
// A NOINSERT cell sets the base plane only.  No two calls for one track name the same column.
template <class F>
__device__ void track_cells(const Ctx& x, const Rec& m, uint8_t pad_strand, F&& f) {
    const uint8_t* r = x.buf + m.off;
    const int lo = max(m.pos, x.s0) - x.s0, hi = min(m.end, x.stop) - x.s0;
    const int a = lo + x.s0 - m.pos, nb = hi - lo;
    const uint8_t strand = (m.bits & R_REVERSE) ? STRAND_LOWER : STRAND_UPPER;
    const int32_t* Qp = x.qpos + m.res + a;
    const int32_t* Id = x.indel + m.res + a;
    const uint8_t* Dl = x.isdel + m.res + a;
    auto tok = [&](int qp) -> uint8_t { return qp < m.l_seq ? SEQ_TOK[seq_code(r, m, qp)] : TOK_N; };
    auto qual = [&](int qp) -> uint8_t { return qp < m.l_seq ? r[m.qual_off + qp] : 0; };
    auto st = [&](int k) -> uint8_t { return Dl[k] ? pad_strand : strand; };
    for (int k = 0; k < nb; ++k) f(x.col[lo + k], Dl[k] ? TOK_GAP : tok(Qp[k]), qual(Qp[k]), st(k), true);
    if (m.pos >= x.s0) f(x.prev[lo], START, qual(Qp[0]), st(0), true);   // head column inside the window
    for (int k = 0; k < nb; ++k) {
        const int p = lo + k, lg = x.longest[p];
        if (lg <= 0) continue;
        const int c0 = x.col[p] + 1, ins = Id[k], q0 = Qp[k];
        const int n_ins = ins > 0 ? min(ins, p == x.ci ? x.cap_ci : x.cap) : 0;
        const uint8_t qk = qual(q0);
        for (int j = 1; j <= lg; ++j) {
            if (j <= n_ins) f(c0 + j - 1, q0 + j < m.l_seq ? SEQ_TOK[seq_code(r, m, q0 + j)] : TOK_N, qk, st(k), true);
            else f(c0 + j - 1, NOINSERT, 0, 0, false);
        }
    }
    if (m.end <= x.stop) {                                             // tail column inside the window
        const int k = nb - 1, p = lo + k;
        f(x.col[p] + x.longest[p] + 1, END, qual(Qp[k]), st(k), true);
    }
}

__device__ inline void block_zero(uint8_t* p, int64_t n) {
    for (int64_t i = threadIdx.x; i < n; i += BLOCK) p[i] = 0;
}

// LDS of one location's workgroup: what the status rule builds and, for a record, what the rendering reads.
struct Work {
    int32_t cover[MAX_POS + 1], longest[MAX_POS], col[MAX_POS], prev[MAX_POS];
    uint8_t covered[MAX_POS];
    int32_t tracks[MAX_TRACKS];
    unsigned long long hash[HASH_SLOTS];
    uint8_t bits[MAX_TRACKS], pad[MAX_TRACKS];
    int32_t wave[BLOCK / 64];
    int32_t n, decline, status, k, first, f[3], clo, chi, off;
};

__device__ inline Ctx make_ctx(const Work& w, const Loc& L, const Params& P, const uint8_t* buf, const int32_t* qpos,
                               const int32_t* indel, const uint8_t* isdel) {
    return Ctx{buf, qpos, indel, isdel, w.col, w.prev, w.longest, L.s0, L.stop, L.ci, P.max_insert_length,
               max(P.max_insert_length_variant, P.max_insert_length)};
}

// The status of one location (0 no record, 1 record, 2 declined), the same value in every thread of the workgroup: the one
// rule of encode_locations and census_locations.  For status 1, w holds the tracks, the column map, the crop (clo, chi, off),
// the pad strands and the kept rows (k, first, f) the rendering needs.  It reads qpos / indel / isdel: the last step
// (finish_record's trim, which gives 0 when the planes keep different row counts) needs every track's cells inside the crop.
__device__ int location_status(Work& w, const Loc& L, const Params& P, const uint8_t* __restrict__ buf, const Rec* __restrict__ recs,
                               const uint8_t* __restrict__ reftok, const int32_t* __restrict__ qpos,
                               const int32_t* __restrict__ indel, const uint8_t* __restrict__ isdel) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (L.pre >= 0) return L.pre;
    const int n_pos = L.stop - L.s0;
    for (int p = tid; p <= n_pos; p += BLOCK) { w.cover[p] = 0; if (p < n_pos) w.longest[p] = 0; }
    for (int i = tid; i < HASH_SLOTS; i += BLOCK) w.hash[i] = 0;
    if (tid == 0) { w.n = 0; w.decline = 0; }
    __syncthreads();

    // ---- resolve_reads + the window filter of process_tracks: tracks in record order (= stable order by clipped start,
    // the host having checked that the run's records are position-sorted)
    for (int base = L.first; base < L.last; base += BLOCK) {
        const int i = base + tid;
        int sel = 0;
        if (i < L.last) {
            const Rec& m = recs[i];
            if (m.bits & R_FLAG_OK) {
                if (m.end > m.pos && m.pos < L.stop && m.end > L.s0) {
                    sel = 1;
                    if (m.bits & (R_SKIP | R_EQ | R_SHORT_SEQ)) w.decline = 1;
                } else if ((m.bits & R_HAS_REF) && m.end == m.pos && m.pos >= L.s0 && m.pos < L.stop) {
                    w.decline = 1;                                     // a zero-length alignment inside the window
                }
            }
        }
        const unsigned long long mask = __ballot(sel);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) w.wave[wave] = __popcll(mask);
        __syncthreads();
        int off = w.n, total = 0;
        for (int v = 0; v < BLOCK / 64; ++v) { if (v < wave) off += w.wave[v]; total += w.wave[v]; }
        if (sel && off + before < MAX_TRACKS) w.tracks[off + before] = i;
        __syncthreads();
        if (tid == 0) w.n += total;
        __syncthreads();
    }
    const int n = w.n;
    if (n > MAX_TRACKS || w.decline) return 2;
    // ---- two tracks sharing a name:sequence key
    for (int t = tid; t < n; t += BLOCK) {
        const unsigned long long h = recs[w.tracks[t]].hash;
        for (unsigned s = (unsigned)h & (HASH_SLOTS - 1);; s = (s + 1) & (HASH_SLOTS - 1)) {
            const unsigned long long prev = atomicCAS(&w.hash[s], 0ull, h);
            if (prev == 0ull) break;
            if (prev == h) { w.decline = 1; break; }
        }
    }
    __syncthreads();
    if (w.decline) return 2;
    // ---- coverage and the longest capped insertion per position
    const int cap = P.max_insert_length, cap_ci = max(P.max_insert_length_variant, P.max_insert_length);
    for (int t = tid; t < n; t += BLOCK) {
        const Rec& m = recs[w.tracks[t]];
        const int lo = max(m.pos, L.s0) - L.s0, hi = min(m.end, L.stop) - L.s0;
        atomicAdd(&w.cover[lo], 1);
        atomicAdd(&w.cover[hi], -1);
        const int32_t* Id = indel + m.res + (L.s0 - m.pos);
        for (int p = lo; p < hi; ++p) {
            const int ins = Id[p];
            if (ins > 0) atomicMax(&w.longest[p], min(ins, p == L.ci ? cap_ci : cap));
        }
    }
    __syncthreads();
    // ---- the column map, the centre and the crop
    if (tid == 0) {
        int run = 0, col = 1, prev = 0, covered = 0;
        for (int p = 0; p < n_pos; ++p) {
            run += w.cover[p];
            w.covered[p] = run > 0;
            if (run > 0) { w.col[p] = col; w.prev[p] = prev; prev = col; col += 1 + w.longest[p]; ++covered; }
        }
        int status = -1;
        if (covered == 0 || L.ci < 0 || L.ci >= n_pos || !w.covered[L.ci]) status = 0;
        else
            for (int p = 0; p < n_pos; ++p)
                if (w.covered[p] && reftok[L.ref + p] == REF_UNKNOWN) { status = 2; break; }
        w.status = status;
        if (status < 0) {
            const int center = w.col[L.ci], n_cols = col + 1;
            w.clo = max(0, center - P.w);
            w.chi = min(center + P.w + 1, n_cols);
            w.off = P.w - (center - w.clo);
        }
    }
    __syncthreads();
    if (w.status >= 0) return w.status;
    const Ctx x = make_ctx(w, L, P, buf, qpos, indel, isdel);
    const int clo = w.clo, chi = w.chi;
    // ---- per track: nonzero cells inside the crop (base, quality, strand planes) and the strand that fills its pads
    for (int t = tid; t < n; t += BLOCK) {
        const Rec& m = recs[w.tracks[t]];
        const int lo = max(m.pos, L.s0) - L.s0, hi = min(m.end, L.stop) - L.s0;
        const uint8_t* Dl = isdel + m.res + (lo + L.s0 - m.pos);
        bool aligned = false;
        for (int k = 0; k < hi - lo && !aligned; ++k) aligned = Dl[k] == 0;
        // deletions carry no strand: the row's own strand, forward when it has none (:1063-1078)
        const uint8_t pad = aligned ? ((m.bits & R_REVERSE) ? STRAND_LOWER : STRAND_UPPER) : STRAND_UPPER;
        uint8_t bits = 0;
        track_cells(x, m, pad, [&](int c, uint8_t, uint8_t q, uint8_t, bool qs) {
            if (c < clo || c >= chi) return;
            bits |= 1;
            if (qs) bits |= 4 | (q ? 2 : 0);
        });
        w.bits[t] = bits;
        w.pad[t] = pad;
    }
    __syncthreads();
    // ---- finish_record: trim the leading rows with nothing inside the crop (each plane alone), keep the middle rows
    if (tid == 0) {
        int f[3] = {0, 0, 0};
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < n; ++r)
                if (w.bits[r] & (1 << c)) { f[c] = r; break; }
        const int nbr = n - f[0], nq = n - f[1], ns = n - f[2];
        const int first = max(0, (nbr - P.max_reads) / 2);
        const int last = min(first + P.max_reads, nbr);
        auto count = [&](int v) { return max(0, min(last, v) - min(first, v)); };
        const int kb = count(nbr), kq = count(nq), ks = count(ns);
        w.status = (kq != kb || ks != kb || kb == 0) ? 0 : 1;
        w.k = min(P.max_reads, kb);
        w.first = first;
        for (int c = 0; c < 3; ++c) w.f[c] = f[c];
    }
    __syncthreads();
    return w.status == 1 ? 1 : 0;
}

__global__ void __launch_bounds__(BLOCK) encode_locations(
    const uint8_t* __restrict__ buf, const Rec* __restrict__ recs, const Loc* __restrict__ locs, const uint8_t* __restrict__ reftok,
    const int32_t* __restrict__ qpos, const int32_t* __restrict__ indel, const uint8_t* __restrict__ isdel, Params P,
    uint8_t* __restrict__ reads, uint8_t* __restrict__ qual, uint8_t* __restrict__ strand, uint8_t* __restrict__ ref_small,
    int32_t* __restrict__ num_small, int8_t* __restrict__ status_small) {
    __shared__ Work w;
    const int tid = threadIdx.x;
    const int li = blockIdx.x;
    const Loc L = locs[li];
    const int64_t plane = (int64_t)P.max_reads * P.W;
    uint8_t* out[3] = {reads + L.slot * plane, qual + L.slot * plane, strand + L.slot * plane};
    // Every byte of the location's slot is stored once, by one thread (zeros unless status 1): no two threads of the
    // workgroup store to one global address, so no ordering between their stores is needed.
    auto empty = [&](int status) {
        for (int c = 0; c < 3; ++c) block_zero(out[c], plane);
        block_zero(ref_small + (int64_t)li * P.W, P.W);
        if (tid == 0) { status_small[li] = (int8_t)status; num_small[li] = 0; }
    };
    const int status = location_status(w, L, P, buf, recs, reftok, qpos, indel, isdel);
    if (status != 1) { empty(status); return; }
    const int n_pos = L.stop - L.s0;
    const Ctx x = make_ctx(w, L, P, buf, qpos, indel, isdel);
    const int clo = w.clo, chi = w.chi, off = w.off;
    const int k = w.k;
    for (int job = tid; job < 3 * k; job += BLOCK) {            // one thread zeroes a kept row, then writes its cells
        const int c = job / k, r = job - c * k;
        const int t = w.f[c] + w.first + r;
        uint8_t* row = out[c] + (int64_t)r * P.W;
        for (int i = 0; i < P.W; ++i) row[i] = 0;
        track_cells(x, recs[w.tracks[t]], w.pad[t], [&](int col, uint8_t b, uint8_t q, uint8_t s, bool qs) {
            if (col < clo || col >= chi) return;
            if (c == 0) row[off + col - clo] = b;
            else if (qs) row[off + col - clo] = c == 1 ? q : s;
        });
    }
    for (int c = 0; c < 3; ++c) block_zero(out[c] + (int64_t)k * P.W, plane - (int64_t)k * P.W);
    // reference line: TOK_GAP, the token of each covered position at its column (assembled in LDS, stored once)
    __shared__ uint8_t s_ref[2 * MAX_WINDOW + 1];
    for (int i = tid; i < chi - clo; i += BLOCK) s_ref[i] = TOK_GAP;
    __syncthreads();
    for (int p = tid; p < n_pos; p += BLOCK)
        if (w.covered[p] && w.col[p] >= clo && w.col[p] < chi) s_ref[w.col[p] - clo] = reftok[L.ref + p];
    __syncthreads();
    uint8_t* ref_out = ref_small + (int64_t)li * P.W;
    for (int i = tid; i < P.W; i += BLOCK) ref_out[i] = (i >= off && i < off + chi - clo) ? s_ref[i - off] : 0;
    if (tid == 0) { status_small[li] = 1; num_small[li] = k; }
}

// The census: the status of every location and nothing else -- one byte per location, stored by thread 0.
__global__ void __launch_bounds__(BLOCK) census_locations(
    const uint8_t* __restrict__ buf, const Rec* __restrict__ recs, const Loc* __restrict__ locs, const uint8_t* __restrict__ reftok,
    const int32_t* __restrict__ qpos, const int32_t* __restrict__ indel, const uint8_t* __restrict__ isdel, Params P,
    int8_t* __restrict__ status_small) {
    __shared__ Work w;
    const Loc L = locs[blockIdx.x];
    const int status = location_status(w, L, P, buf, recs, reftok, qpos, indel, isdel);
    if (threadIdx.x == 0) status_small[blockIdx.x] = (int8_t)status;
}

}  // namespace

hipError_t launch_resolve(const uint8_t* buf, Rec* recs, int32_t n_recs, int32_t* qpos, int32_t* indel, uint8_t* isdel,
                          hipStream_t s) {
    if (n_recs <= 0) return hipSuccess;
    hipLaunchKernelGGL(resolve_records, dim3((n_recs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, buf, recs, n_recs, qpos, indel, isdel);
    return hipGetLastError();
}

hipError_t launch_encode(const uint8_t* buf, const Rec* recs, const Loc* locs, int32_t n_locs, const uint8_t* reftok,
                         const int32_t* qpos, const int32_t* indel, const uint8_t* isdel, Params p, uint8_t* reads,
                         uint8_t* qual, uint8_t* strand, uint8_t* ref_small, int32_t* num_small, int8_t* status_small,
                         hipStream_t s) {
    if (n_locs <= 0) return hipSuccess;
    hipLaunchKernelGGL(encode_locations, dim3(n_locs), dim3(BLOCK), 0, s, buf, recs, locs, reftok, qpos, indel, isdel, p, reads,
                       qual, strand, ref_small, num_small, status_small);
    return hipGetLastError();
}

hipError_t launch_census(const uint8_t* buf, const Rec* recs, const Loc* locs, int32_t n_locs, const uint8_t* reftok,
                         const int32_t* qpos, const int32_t* indel, const uint8_t* isdel, Params p, int8_t* status_small,
                         hipStream_t s) {
    if (n_locs <= 0) return hipSuccess;
    hipLaunchKernelGGL(census_locations, dim3(n_locs), dim3(BLOCK), 0, s, buf, recs, locs, reftok, qpos, indel, isdel, p, status_small);
    return hipGetLastError();
}

}  // namespace pg
