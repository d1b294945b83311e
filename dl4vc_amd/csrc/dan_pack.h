// dan_finalize's host half: the checkpoint's tensors, checked against the configuration and packed into the blocks the kernels
// read (layouts: dan_kernels.h).  Plain host arithmetic -- no HIP runtime call and no handle, so that tools/dan_pack_main.cpp
// runs it on a CPU, under a sanitizer too.  Errors are a code plus text in the caller's string, never an exception.
#pragma once

#include "dan_net.h"
#include "capi_shell.h"

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

namespace dan {

struct Tensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};
using TensorMap = std::map<std::string, Tensor>;

inline const Tensor* need(const TensorMap& m, std::string& err, const std::string& name, std::initializer_list<int64_t> shape, int* rc) {
    auto it = m.find(name);
    if (it == m.end()) {
        *rc = capi::failf(err, DAN_ERR_MISSING_TENSOR, "missing tensor '%s'", name.c_str());
        return nullptr;
    }
    const Tensor& t = it->second;
    std::vector<int64_t> want(shape);
    if (t.shape != want) {
        std::string got, exp;
        for (auto s : t.shape) got += std::to_string(s) + ",";
        for (auto s : want) exp += std::to_string(s) + ",";
        *rc = capi::failf(err, DAN_ERR_SHAPE, "tensor '%s' has shape (%s) but the configuration needs (%s)", name.c_str(),
                          got.c_str(), exp.c_str());
        return nullptr;
    }
    return &t;
}

// fp32 -> bf16 bits, round to nearest even (what v_cvt_pk_bf16_f32 does); NaN stays NaN
inline uint16_t bf16_bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_float(uint16_t b) { uint32_t u = (uint32_t)b << 16; float x; memcpy(&x, &u, 4); return x; }

// MFMA A-fragment order for v_mfma_f32_16x16x4_f32 with the k order of a 16-channel group permuted:
//   packed[((tap*kg + g)*tiles + n)*64 + lane][s] = W[o = 16n + (lane&15)][c = 16g + 4(lane>>4) + s][tap]
// W(o,c,tap) is supplied by the functor (zero outside the real extents).
template <typename F>
void pack_frag(float* out, int taps, int kg, int tiles, F W) {
    size_t i = 0;
    for (int t = 0; t < taps; ++t)
        for (int g = 0; g < kg; ++g)
            for (int n = 0; n < tiles; ++n)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) out[i++] = W(16 * n + (lane & 15), 16 * g + 4 * (lane >> 4) + s, t);
}

// MFMA 32x32x16 bf16 A-fragment order of the ping-pong kernel (dan_kernels.h): fragment ((ks * taps + t) * nq + q), lane, j
// (channel-group major: layer 1's three groups are the first nine steps of the walk):
//   row m = lane & 31 -> output channel 32 q + 16 ((m >> 2) & 1) + 4 (m >> 3) + (m & 3),  k = 16 ks + 8 (lane >> 5) + j
template <typename F>
void pack_fragp(uint16_t* dst, int taps, int ksteps, int nq, F W) {
    for (int t = 0; t < taps; ++t)
        for (int ks = 0; ks < ksteps; ++ks)
            for (int q = 0; q < nq; ++q) {
                uint16_t* f = dst + ((size_t)(ks * taps + t) * nq + q) * (WP_FRAG / 2);
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int m = lane & 31;
                        const int o = 32 * q + 16 * ((m >> 2) & 1) + 4 * (m >> 3) + (m & 3);
                        f[lane * 8 + j] = bf16_bits(W(o, 16 * ks + 8 * (lane >> 5) + j, t));
                    }
            }
}

// MFMA 16x16x32 bf16 A-fragment order of the sixteen-wave form (PLANES 1) and of the bf16x3 kernel (PLANES 2: hi and lo plane of a
// tile side by side, lo = bf16(w - hi)): fragment (((ks * taps + t) * n_ct + ct) * PLANES + plane), lane, j with
//   row r = lane & 15 of channel tile ct -> output channel 32 (ct >> 1) + 8 (r >> 2) + 4 (ct & 1) + (r & 3)   (a lane's two tiles of a
//   column are 8 consecutive channels),  k = 32 ks + 8 (lane >> 4) + j
template <int PLANES, typename F>
void pack_frag16(uint16_t* dst, int taps, int ksteps, int n_ct, F W) {
    for (int ks = 0; ks < ksteps; ++ks)
        for (int t = 0; t < taps; ++t)
            for (int ct = 0; ct < n_ct; ++ct) {
                uint16_t* f = dst + ((size_t)(ks * taps + t) * n_ct + ct) * PLANES * (WP_FRAG / 2);
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int r = lane & 15;
                        const int o = 32 * (ct >> 1) + 8 * (r >> 2) + 4 * (ct & 1) + (r & 3);
                        const float w = W(o, 32 * ks + 8 * (lane >> 4) + j, t);
                        const uint16_t hi = bf16_bits(w);
                        f[lane * 8 + j] = hi;
                        if (PLANES == 2) f[WP_FRAG / 2 + lane * 8 + j] = bf16_bits(w - bf16_float(hi));
                    }
            }
}

// What every family packs conv layer l from: the checkpoint's tensors behind the canonical channel order (zero outside the real
// extents).  layer_source also writes the layer's fp32 constants, which every family copies from the fp32 block.
struct LayerSrc {
    int l = 0, cin = 0, cout = 0, H = 0, L = 0;
    std::vector<int> inv;                                    // canonical channel -> reference channel
    const Tensor *w = nullptr, *wr = nullptr, *wb = nullptr, *wcm = nullptr, *bcm = nullptr;
    float Wf(int o, int cc, int t) const {
        if (o >= cout || cc >= (int)inv.size() || inv[cc] < 0) return 0.f;
        return w->data[((size_t)o * cin + inv[cc]) * 3 + t];
    }
    float Wr(int o, int cc) const { return (o < cout && cc < cout) ? wr->data[(size_t)o * cout + cc] : 0.f; }
    float Wb(int o, int cc) const { return (o < H && cc < cout) ? wb->data[(size_t)o * cout + cc] : 0.f; }
    float Wc(int o, int cc, int pp) const { return (o < H && cc < H) ? wcm->data[((size_t)o * H + cc) * L + pp] : 0.f; }
};

// the tensors of 0-based layer l (checked), its constants cst[CST_FLOATS] (bias, folded eval BN, residual and bottleneck biases)
// and its bit of res_mask
inline int layer_source(const dan_config& c, const TensorMap& m, std::string& err, int l, float* cst, LayerSrc* s, unsigned* res_mask) {
    const int l1 = l + 1;
    int rc = DAN_OK, dil;
    s->l = l; s->H = c.bottleneck; s->L = c.length;
    layer_dims(c, l1, &s->cin, &s->cout, &dil);
    const int cin = s->cin, cout = s->cout, H = s->H;
    const std::string p = "conv1D_layers." + std::to_string(l);
    s->w = need(m, err, p + ".weight", {cout, cin, 1, 3}, &rc); if (!s->w) return rc;
    const Tensor* b = need(m, err, p + ".bias", {cout}, &rc); if (!b) return rc;
    // canonical position of the reference's layer-1 input channels (model.py:517,543,558,625)
    std::vector<int> canon;
    for (int i = 0; i < 2 * EMBED; ++i) canon.push_back(i);
    if (c.use_q) canon.push_back(40);
    if (c.use_strand) canon.push_back(41);
    if (c.use_mask) { canon.push_back(42); canon.push_back(43); canon.push_back(44); }
    s->inv.assign((l == 0 ? KG0 : KGC) * 16, -1);
    for (int i = 0; i < cin; ++i) s->inv[l == 0 ? canon[i] : i] = i;
    for (int o = 0; o < cout; ++o) { cst[CST_BIAS + o] = b->data[o]; cst[CST_SCALE + o] = 1.f; }
    if (c.use_bn) {                                          // eval-mode BN after the ReLU, eps 1e-5 (model.py:750-751)
        const std::string q = "bn1D_layers." + std::to_string(l);
        const Tensor* g = need(m, err, q + ".weight", {cout}, &rc); if (!g) return rc;
        const Tensor* be = need(m, err, q + ".bias", {cout}, &rc); if (!be) return rc;
        const Tensor* mu = need(m, err, q + ".running_mean", {cout}, &rc); if (!mu) return rc;
        const Tensor* var = need(m, err, q + ".running_var", {cout}, &rc); if (!var) return rc;
        for (int o = 0; o < cout; ++o) {
            const double sc = (double)g->data[o] / std::sqrt((double)var->data[o] + 1e-5);
            cst[CST_SCALE + o] = (float)sc;
            cst[CST_SHIFT + o] = (float)((double)be->data[o] - (double)mu->data[o] * sc);
        }
    }
    if (is_residual(c, l1)) {
        const std::string q = "residual_conv_layers." + std::to_string(l1 - c.residual_start);   // model.py:760
        s->wr = need(m, err, q + ".weight", {cout, cout, 1, 1}, &rc); if (!s->wr) return rc;
        const Tensor* br = need(m, err, q + ".bias", {cout}, &rc); if (!br) return rc;
        for (int o = 0; o < cout; ++o) cst[CST_BRES + o] = br->data[o];
        *res_mask |= 1u << l;
    }
    if (H > 0) {
        const std::string q = "conv1D_bottleneck_layers." + std::to_string(l);
        s->wb = need(m, err, q + ".weight", {H, cout, 1, 1}, &rc); if (!s->wb) return rc;
        const Tensor* bb = need(m, err, q + ".bias", {H}, &rc); if (!bb) return rc;
        for (int o = 0; o < H; ++o) cst[CST_BBOT + o] = bb->data[o];
        const std::string z = "conv1D_compression_layers." + std::to_string(l);
        s->wcm = need(m, err, z + ".weight", {H, H, 1, c.length}, &rc); if (!s->wcm) return rc;
        s->bcm = need(m, err, z + ".bias", {H}, &rc); if (!s->bcm) return rc;
    }
    return DAN_OK;
}

// layer 1 by table (dan_kernels.h L0_*): conv1 is linear in the terms its input column is a sum of; sums in double
inline std::vector<float> layer0_table(const LayerSrc& s, const Tensor& emb, const Tensor& pe) {
    const int L = s.L;
    std::vector<float> tab(l0_tab_floats(L), 0.f);
    for (int t = 0; t < 3; ++t)
        for (int o = 0; o < CPAD; ++o) {
            for (int ta = 0; ta < VOCAB; ++ta)
                for (int tb = 0; tb < VOCAB; ++tb) {
                    double v = 0.0;
                    for (int e = 0; e < EMBED; ++e)
                        v += (double)s.Wf(o, e, t) * emb.data[(size_t)ta * EMBED + e] + (double)s.Wf(o, EMBED + e, t) * emb.data[(size_t)tb * EMBED + e];
                    tab[L0_TJ_OFF + ((size_t)t * L0_NTJ + ta * 10 + tb) * CPAD + o] = (float)v;
                }
            for (int k = 0; k < 5; ++k) tab[L0_WSC_OFF + ((size_t)k * 3 + t) * CPAD + o] = s.Wf(o, 2 * EMBED + k, t);
        }
    // the positional term of tap t at column w: sum_e (W[o][e][t] + W[o][20 + e][t]) pe[w][e]; PE[variant][w] = the taps whose
    // column w + t - 1 exists for a unit that has / lacks a left / right neighbour at w (and lies inside the window anyway)
    std::vector<double> pet((size_t)3 * L * CPAD);
    for (int t = 0; t < 3; ++t)
        for (int wcol = 0; wcol < L; ++wcol)
            for (int o = 0; o < CPAD; ++o) {
                double v = 0.0;
                for (int e = 0; e < EMBED; ++e) v += ((double)s.Wf(o, e, t) + (double)s.Wf(o, EMBED + e, t)) * pe.data[(size_t)wcol * EMBED + e];
                pet[((size_t)t * L + wcol) * CPAD + o] = v;
            }
    for (int var = 0; var < 3; ++var)
        for (int wcol = 0; wcol < L; ++wcol)
            for (int o = 0; o < CPAD; ++o) {
                double v = pet[((size_t)1 * L + wcol) * CPAD + o];
                if (var != 1 && wcol - 1 >= 0) v += pet[((size_t)0 * L + wcol - 1) * CPAD + o];
                if (var != 2 && wcol + 1 < L) v += pet[((size_t)2 * L + wcol + 1) * CPAD + o];
                tab[L0_PE_OFF + ((size_t)var * L + wcol) * CPAD + o] = (float)v;
            }
    return tab;
}

// the fp32 block of a layer (dan_kernels.h): MFMA fragments of the conv, its Winograd F(2,3) and F(4,3) forms, the residual and the bottleneck
inline void pack_layer_fp32(const LayerSrc& s, float* blk) {
    auto Wf = [&](int o, int cc, int t) { return s.Wf(o, cc, t); };
    pack_frag(blk + W_OFF, 3, s.l == 0 ? KG0 : KGC, KGC, Wf);
    if (s.l > 0) {
        // Winograd F(2,3) weight transform U = [g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2], formed in double
        auto Wu = [&](int o, int cc, int k) -> float {
            const double g0 = s.Wf(o, cc, 0), g1 = s.Wf(o, cc, 1), g2 = s.Wf(o, cc, 2);
            return k == 0 ? (float)g0 : k == 1 ? (float)((g0 + g1 + g2) * 0.5) : k == 2 ? (float)((g0 - g1 + g2) * 0.5) : (float)g2;
        };
        pack_frag(blk + WW_OFF, 4, KGC, KGC, Wu);
        // Winograd F(4,3) weight transform U = G g for the points 0, +-1, +-2, formed in double: G = [1/4, 0, 0], -1/6 [1, 1, 1],
        // -1/6 [1, -1, 1], [1/24, 1/12, 1/6], [1/24, -1/12, 1/6], [0, 0, 1]
        auto Wu43 = [&](int o, int cc, int k) -> float {
            const double g0 = s.Wf(o, cc, 0), g1 = s.Wf(o, cc, 1), g2 = s.Wf(o, cc, 2);
            switch (k) {
                case 0: return (float)(g0 / 4.0);
                case 1: return (float)(-(g0 + g1 + g2) / 6.0);
                case 2: return (float)(-(g0 - g1 + g2) / 6.0);
                case 3: return (float)(g0 / 24.0 + g1 / 12.0 + g2 / 6.0);
                case 4: return (float)(g0 / 24.0 - g1 / 12.0 + g2 / 6.0);
                default: return (float)g2;
            }
        };
        pack_frag(blk + W43_OFF, 6, KGC, KGC, Wu43);
    }
    if (s.wr) pack_frag(blk + WRES_OFF, 1, KGC, KGC, [&](int o, int cc, int) { return s.Wr(o, cc); });
    if (s.wb) pack_frag(blk + WBOT_OFF, 1, KGC, 2, [&](int o, int cc, int) { return s.Wb(o, cc); });
}

// the plain-bf16 blocks of a layer: 32x32x16 fragments of the eight-wave form (blkp), 16x16x32 of the sixteen-wave form (blkr)
inline void pack_layer_bf16p(const LayerSrc& s, const float* cst, char* blkp, char* blkr) {
    auto Wf = [&](int o, int cc, int t) { return s.Wf(o, cc, t); };
    auto Wr = [&](int o, int cc, int) { return s.Wr(o, cc); };
    auto Wb = [&](int o, int cc, int) { return s.Wb(o, cc); };
    pack_fragp((uint16_t*)(blkp + WP_CONV_OFF), 3, s.l == 0 ? P_KS0 : P_KSC, 4, Wf);
    pack_frag16<1>((uint16_t*)(blkr + WP_CONV_OFF), 3, s.l == 0 ? 2 : 4, 8, Wf);
    if (s.wr) {
        pack_fragp((uint16_t*)(blkp + WP_RES_OFF), 1, P_KSC, 4, Wr);
        pack_frag16<1>((uint16_t*)(blkr + WP_RES_OFF), 1, 4, 8, Wr);
    }
    if (s.wb) {
        pack_fragp((uint16_t*)(blkp + WP_BOT_OFF), 1, P_KSC, 1, Wb);
        pack_frag16<1>((uint16_t*)(blkr + WP_BOT_OFF), 1, 4, 2, Wb);
    }
    memcpy(blkp + WP_CST_OFF, cst, CST_FLOATS * sizeof(float));
    memcpy(blkr + WP_CST_OFF, cst, CST_FLOATS * sizeof(float));
}

// the bf16x3 block of a layer: hi / lo 16x16x32 fragments and the constants in this family's form
inline void pack_layer_bf16x(const LayerSrc& s, const float* cst, char* blkx) {
    pack_frag16<2>((uint16_t*)(blkx + WX_CONV_OFF), 3, s.l == 0 ? X_KS0 : X_KS, 8, [&](int o, int cc, int t) { return s.Wf(o, cc, t); });
    if (s.wr) pack_frag16<2>((uint16_t*)(blkx + WX_RES_OFF), 1, X_KS, 8, [&](int o, int cc, int) { return s.Wr(o, cc); });
    if (s.wb) pack_frag16<2>((uint16_t*)(blkx + WX_BOT_OFF), 1, X_KS, 2, [&](int o, int cc, int) { return s.Wb(o, cc); });
    float* cx = (float*)(blkx + WX_CST_OFF);
    memcpy(cx, cst, CST_FLOATS * sizeof(float));
    // this family's epilogue computes relu(acc + b) * sc + sh as max(acc, -b) * sc + (sh + b * sc) (dan_kernels_bf16x.hip):
    // the bias slot holds -b, the shift slot sh + b * sc (formed in double)
    for (int ch = 0; ch < CPAD; ++ch) {
        const double b = cx[CST_BIAS + ch];
        cx[CST_SHIFT + ch] = (float)((double)cx[CST_SHIFT + ch] + b * (double)cx[CST_SCALE + ch]);
        cx[CST_BIAS + ch] = (float)-b;
    }
}

// conv(pool): the weights of a layer behind a pool layer as [o][t * 128 + c] -- bf16-rounded for the plain-bf16 kernel (its oracle's
// "storage" mode), fp32 for bf16x3
inline void pack_conv_pool(const LayerSrc& s, bool round_bf16, float* wp) {
    for (int o = 0; o < CPAD; ++o)
        for (int t = 0; t < 3; ++t)
            for (int cc = 0; cc < CPAD; ++cc)
                wp[((size_t)o * 3 + t) * CPAD + cc] = round_bf16 ? bf16_float(bf16_bits(s.Wf(o, cc, t))) : s.Wf(o, cc, t);
}

// floats of a layer's highway compression weights: [g = 2L][tile 2][lane 64][4] = [pos][n 2][plane 2][lane 64][8 bf16]
inline size_t hw_layer_floats(int L) { return (size_t)L * 2 * 2 * 64 * 4; }

// highway compression weights of a layer: fp32 MFMA order (wc), the bias (bc) and, for launch_highway16, two bf16 planes (wc16 or null)
inline void pack_highway(const LayerSrc& s, float* wc, float* bc, uint16_t* wc16) {
    const int L = s.L;
    // k = p*32 + c, k-group g = 2p + (c >> 4):  packed[g][n][lane][s] = Wc[o][c][p]
    size_t i = 0;
    for (int g = 0; g < 2 * L; ++g)
        for (int n = 0; n < 2; ++n)
            for (int lane = 0; lane < 64; ++lane)
                for (int k = 0; k < 4; ++k) wc[i++] = s.Wc(16 * n + (lane & 15), 16 * (g & 1) + 4 * (lane >> 4) + k, g >> 1);
    for (int o = 0; o < s.H; ++o) bc[o] = s.bcm->data[o];
    if (!wc16) return;
    for (int pp = 0; pp < L; ++pp)
        for (int n = 0; n < 2; ++n)
            for (int lane = 0; lane < 64; ++lane)
                for (int s8 = 0; s8 < 8; ++s8) {
                    const float w = s.Wc(16 * n + (lane & 15), 8 * (lane >> 4) + s8, pp);
                    const uint16_t hi = bf16_bits(w);
                    const size_t base = (((size_t)pp * 2 + n) * 2) * 64 * 8;
                    wc16[base + (size_t)lane * 8 + s8] = hi;                                   // plane 0
                    wc16[base + 64 * 8 + (size_t)lane * 8 + s8] = bf16_bits(w - bf16_float(hi));   // plane 1
                }
}

// what packing needs to know about the kernel family that will read the blocks
struct PackFamily {
    int precision;                           // dan_config.precision: which per-layer blocks besides the fp32 one
    bool conv_pool;                          // the layer behind a pool layer also as conv(pool) weights
    bool hw_bf16;                            // the highway compression weights also as two bf16 planes
};

// Everything dan_finalize uploads, in host memory.  A vector a family does not read stays empty; emb, pe and fc0 point into the
// tensor map (fc0: precision 0 only, uploaded row by row at the padded stride).
struct Packed {
    unsigned res_mask = 0;
    const Tensor *emb = nullptr, *pe = nullptr, *fc0 = nullptr;
    std::vector<float> l0tab;                // precision 0: layer 1 by table
    std::vector<float> wl;                   // [layers][LAYER_STRIDE]: every precision (the source of every family's constants)
    std::vector<char> wlp, wlr, wlx;         // [layers][WP_LAYER_BYTES] twice (precision 2), [layers][WX_LAYER_BYTES] (precision 1)
    std::vector<float> wpool, zero;          // conv(pool): [segment][128][384] and 128 zeros
    std::vector<float> wc, bc, wc16;         // highway: [layers][hw_layer_floats], [layers][HPAD], the bf16 planes
    std::vector<uint16_t> w0x;               // precision >= 1: fc.0 as two bf16 planes [2][n0][F_stride] (hi, lo)
    std::vector<float> w1;                   // fc.1 [n1][n0_stride], zero padded
    std::vector<float> b0, b1, wh, bh;       // FC biases; the six heads as one matrix [NHEAD][n1] and one bias vector
};

// conv stack: one fixed-stride weight block per layer and family (dan_kernels.h); the fp32 block is packed at every precision and is
// the source of every family's constants.  seg_begin: first 0-based layer of every segment.
inline int pack_conv_stack(const dan_config& c, const TensorMap& m, const std::vector<int>& seg_begin, const PackFamily& fam,
                           Packed* out, std::string& err) {
    const int L = c.length, H = c.bottleneck, n_segments = (int)seg_begin.size();
    const bool is_x = fam.precision == 1, is_p = fam.precision == 2;
    const size_t hw_layer = hw_layer_floats(L);
    const size_t wpool_seg = (size_t)CPAD * 3 * CPAD;
    out->wl.assign((size_t)c.layers * LAYER_STRIDE, 0.f);
    out->wpool.assign(fam.conv_pool ? (size_t)n_segments * wpool_seg : 0, 0.f);
    out->wlp.assign(is_p ? (size_t)c.layers * WP_LAYER_BYTES : 0, 0);
    out->wlr.assign(out->wlp.size(), 0);
    out->wlx.assign(is_x ? (size_t)c.layers * WX_LAYER_BYTES : 0, 0);
    out->wc16.assign(fam.hw_bf16 && H > 0 ? (size_t)c.layers * hw_layer : 0, 0.f);
    out->wc.assign(H > 0 ? (size_t)c.layers * hw_layer : 0, 0.f);
    out->bc.assign((size_t)c.layers * HPAD, 0.f);
    if (fam.conv_pool && n_segments > 1) out->zero.assign(CPAD, 0.f);
    int rc = DAN_OK;
    out->res_mask = 0;
    for (int l = 0; l < c.layers; ++l) {
        float* blk = out->wl.data() + (size_t)l * LAYER_STRIDE;
        LayerSrc src;
        if ((rc = layer_source(c, m, err, l, blk + CST_OFF, &src, &out->res_mask))) return rc;
        pack_layer_fp32(src, blk);
        if (l == 0 && fam.precision == 0) out->l0tab = layer0_table(src, *out->emb, *out->pe);
        if (is_p) pack_layer_bf16p(src, blk + CST_OFF, out->wlp.data() + (size_t)l * WP_LAYER_BYTES, out->wlr.data() + (size_t)l * WP_LAYER_BYTES);
        if (is_x) pack_layer_bf16x(src, blk + CST_OFF, out->wlx.data() + (size_t)l * WX_LAYER_BYTES);
        if (fam.conv_pool && l > 0)
            for (int sg = 1; sg < n_segments; ++sg)
                if (seg_begin[sg] == l) pack_conv_pool(src, is_p, out->wpool.data() + (size_t)sg * wpool_seg);   // the layer behind a pool layer
        if (H > 0)
            pack_highway(src, out->wc.data() + (size_t)l * hw_layer, out->bc.data() + (size_t)l * HPAD,
                         fam.hw_bf16 ? (uint16_t*)(out->wc16.data() + (size_t)l * hw_layer) : nullptr);
    }
    return DAN_OK;
}

// FC stack + heads (model.py:362-377,406-415)
inline int pack_fc_heads(const dan_config& c, const TensorMap& m, const PackFamily& fam, Packed* out, std::string& err) {
    int rc = DAN_OK;
    const int n0 = c.fc_sizes[0], n1 = c.fc_sizes[1], F = feature_width(c);
    const size_t F_stride = (size_t)pad16(F), n0_stride = (size_t)pad16(n0);
    const Tensor* w0 = need(m, err, "fc.0.weight", {n0, F}, &rc); if (!w0) return rc;
    const Tensor* b0 = need(m, err, "fc.0.bias", {n0}, &rc); if (!b0) return rc;
    const Tensor* w1 = need(m, err, "fc.1.weight", {n1, n0}, &rc); if (!w1) return rc;
    const Tensor* b1 = need(m, err, "fc.1.bias", {n1}, &rc); if (!b1) return rc;
    if (fam.precision == 0) {
        out->fc0 = w0;
    } else {
        // the bf16 modes run FC1 (99.5 % of the FC stack's FLOPs) on the bf16 matrix cores with split operands: the weights as two
        // bf16 planes, hi = bf16(w), lo = bf16(w - hi) -- the bytes of the fp32 matrix
        const size_t plane = (size_t)n0 * F_stride;
        out->w0x.assign(2 * plane, 0);
        for (int o = 0; o < n0; ++o)
            for (int64_t k = 0; k < F; ++k) {
                const float w = w0->data[(size_t)o * F + k];
                const uint16_t hi = bf16_bits(w);
                out->w0x[(size_t)o * F_stride + k] = hi;
                out->w0x[plane + (size_t)o * F_stride + k] = bf16_bits(w - bf16_float(hi));
            }
    }
    out->w1.assign((size_t)n1 * n0_stride, 0.f);
    for (int o = 0; o < n1; ++o) memcpy(out->w1.data() + (size_t)o * n0_stride, w1->data.data() + (size_t)o * n0, (size_t)n0 * sizeof(float));
    out->b0 = b0->data; out->b1 = b1->data;
    static const struct { const char* name; int n; } heads[] = {{"fcHidden2BinTarget", 2}, {"fcHidden2VT", 3}, {"fcHidden2AF", 1},
                                                                 {"fcHidden2Coverage", 1}, {"fcHidden2VB", VOCAB}, {"fcHidden2VR", VOCAB}};
    out->wh.clear(); out->bh.clear();
    for (auto& hd : heads) {
        const Tensor* w = need(m, err, std::string(hd.name) + ".weight", {hd.n, n1}, &rc); if (!w) return rc;
        const Tensor* b = need(m, err, std::string(hd.name) + ".bias", {hd.n}, &rc); if (!b) return rc;
        out->wh.insert(out->wh.end(), w->data.begin(), w->data.end());
        out->bh.insert(out->bh.end(), b->data.begin(), b->data.end());
    }
    return DAN_OK;
}

// the whole network: embeddings + positional encoding (model.py:143-145,154-162), the conv stack, the FC stack and the heads
inline int pack_network(const dan_config& c, const TensorMap& m, const std::vector<int>& seg_begin, const PackFamily& fam, Packed* out,
                        std::string& err) {
    int rc = DAN_OK;
    out->emb = need(m, err, "embeddings.weight", {VOCAB, EMBED}, &rc); if (!out->emb) return rc;
    out->pe = need(m, err, "pe", {1, c.length, EMBED}, &rc); if (!out->pe) return rc;
    if ((rc = pack_conv_stack(c, m, seg_begin, fam, out, err))) return rc;
    return pack_fc_heads(c, m, fam, out, err);
}

}  // namespace dan
