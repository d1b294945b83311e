// Stand-alone CPU driver over dl4vc_amd/csrc/dan_pack.h (dan_finalize's host half).  For random tensors of small networks it packs
// at the three precisions and then READS every block back the other way round: for every (output channel, input channel, tap)
// of a block's padded extents it computes the element's index from the layout that dan_kernels.h / dan_pack.h document and
// compares it with the value expected there -- the checkpoint's weight (zero outside the real extents), a double evaluation of
// the stated transform for the Winograd and layer-1 table blocks, exactly bf16(w) and bf16(w - hi) for the bf16 blocks.  Every
// element no formula reaches must be 0.  Also: the constants, res_mask, the FC blocks and the two refusals with code and text.
// Every tensor is a heap vector that ends where its data ends (tools/asan_dan_pack.sh runs this under a sanitizer).
//   g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/dan_pack_main.cpp -o dan_pack_driver
#include "../dl4vc_amd/csrc/dan_pack.h"

#include <cstdio>
#include <cstdlib>

using namespace dan;

static long long g_checks = 0, g_bad = 0;

static void bad(const char* what, long long i, double got, double want) {
    if (g_bad++ < 20) printf("MISMATCH %s[%lld]: got %.9g, expected %.9g\n", what, i, got, want);
}
static void expect(bool ok, const char* what) {
    ++g_checks;
    if (!ok) bad(what, -1, 0, 1);
}

// a buffer being read back: which elements a formula has reached
template <class T>
struct Reader {
    const T* p; size_t n; const char* name; std::vector<char> seen;
    Reader(const T* p_, size_t n_, const char* name_) : p(p_), n(n_), name(name_), seen(n_, 0) {}
    void is(size_t i, T want) {
        ++g_checks;
        if (i >= n) { bad(name, (long long)i, -1, -1); return; }
        seen[i] = 1;
        if (!(p[i] == want)) bad(name, (long long)i, (double)p[i], (double)want);
    }
    void rest_is_zero() {
        for (size_t i = 0; i < n; ++i)
            if (!seen[i]) { ++g_checks; if (!(p[i] == 0)) bad(name, (long long)i, (double)p[i], 0.0); }
    }
};

// bf16 of x, round to nearest, ties to even (no NaN among the test's weights)
static uint16_t to_bf16(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    uint32_t top = u >> 16, low = u & 0xffffu;
    if (low > 0x8000u || (low == 0x8000u && (top & 1u))) ++top;
    return (uint16_t)top;
}
static float from_bf16(uint16_t b) { uint32_t u = (uint32_t)b << 16; float x; memcpy(&x, &u, 4); return x; }

static uint32_t g_rng = 12345;
static float rnd() { g_rng = g_rng * 1664525u + 1013904223u; return (float)((g_rng >> 8) & 0xffff) / 32768.f - 1.f; }

static void put(TensorMap& m, const std::string& name, std::vector<int64_t> shape, bool positive = false) {
    Tensor t;
    t.shape = shape;
    t.data.resize((size_t)t.numel());
    for (auto& v : t.data) v = positive ? 0.5f + 0.25f * (rnd() + 1.f) : rnd();
    m[name] = t;
}

static const struct { const char* name; int n; } HEADS[] = {{"fcHidden2BinTarget", 2}, {"fcHidden2VT", 3}, {"fcHidden2AF", 1},
                                                             {"fcHidden2Coverage", 1}, {"fcHidden2VB", 10}, {"fcHidden2VR", 10}};

// the network as this driver understands it from the configuration alone
struct Net {
    dan_config c;
    int in0, F;
    int cin(int l) const { return l == 0 ? in0 : c.c_init; }
    int cout(int l) const { return l + 1 == c.layers ? c.c_final : c.c_init; }
    bool residual(int l) const { return c.residual_start > 0 && l + 1 >= c.residual_start && !(l + 1 == c.layers && c.c_init != c.c_final); }
    // layer 1: the reference's channel behind canonical channel cc (-1: none); the 40 embedding channels, then q, strand, three flags
    int ref_channel(int cc) const {
        if (cc < 40) return cc;
        const int q = 40, s = q + (c.use_q ? 1 : 0), m = s + (c.use_strand ? 1 : 0);
        if (cc == 40) return c.use_q ? q : -1;
        if (cc == 41) return c.use_strand ? s : -1;
        if (cc <= 44) return c.use_mask ? m + (cc - 42) : -1;
        return -1;
    }
    std::vector<int> seg_begin() const {
        std::vector<int> b{0};
        for (int l1 = 1; l1 < c.layers; ++l1) if ((c.pool_layers_mask >> l1) & 1u) b.push_back(l1);
        return b;
    }
};

static TensorMap make_tensors(const Net& n) {
    const dan_config& c = n.c;
    TensorMap m;
    put(m, "embeddings.weight", {10, 20});
    put(m, "pe", {1, c.length, 20});
    for (int l = 0; l < c.layers; ++l) {
        const std::string s = std::to_string(l);
        put(m, "conv1D_layers." + s + ".weight", {n.cout(l), n.cin(l), 1, 3});
        put(m, "conv1D_layers." + s + ".bias", {n.cout(l)});
        if (c.use_bn) {
            put(m, "bn1D_layers." + s + ".weight", {n.cout(l)});
            put(m, "bn1D_layers." + s + ".bias", {n.cout(l)});
            put(m, "bn1D_layers." + s + ".running_mean", {n.cout(l)});
            put(m, "bn1D_layers." + s + ".running_var", {n.cout(l)}, true);
        }
        if (n.residual(l)) {
            const std::string q = "residual_conv_layers." + std::to_string(l + 1 - c.residual_start);
            put(m, q + ".weight", {n.cout(l), n.cout(l), 1, 1});
            put(m, q + ".bias", {n.cout(l)});
        }
        if (c.bottleneck > 0) {
            put(m, "conv1D_bottleneck_layers." + s + ".weight", {c.bottleneck, n.cout(l), 1, 1});
            put(m, "conv1D_bottleneck_layers." + s + ".bias", {c.bottleneck});
            put(m, "conv1D_compression_layers." + s + ".weight", {c.bottleneck, c.bottleneck, 1, c.length});
            put(m, "conv1D_compression_layers." + s + ".bias", {c.bottleneck});
        }
    }
    put(m, "fc.0.weight", {c.fc_sizes[0], n.F});
    put(m, "fc.0.bias", {c.fc_sizes[0]});
    put(m, "fc.1.weight", {c.fc_sizes[1], c.fc_sizes[0]});
    put(m, "fc.1.bias", {c.fc_sizes[1]});
    for (auto& hd : HEADS) {
        put(m, std::string(hd.name) + ".weight", {hd.n, c.fc_sizes[1]});
        put(m, std::string(hd.name) + ".bias", {hd.n});
    }
    return m;
}

// the weights of layer l read straight from the checkpoint tensors (zero outside the real extents)
struct Layer {
    const Net& n; const TensorMap& m; int l;
    const float *cw = nullptr, *rw = nullptr, *bw = nullptr, *mw = nullptr;
    Layer(const Net& n_, const TensorMap& m_, int l_) : n(n_), m(m_), l(l_) {
        cw = t("conv1D_layers." + s() + ".weight").data();
        if (n.residual(l)) rw = t("residual_conv_layers." + std::to_string(l + 1 - n.c.residual_start) + ".weight").data();
        if (n.c.bottleneck > 0) { bw = t("conv1D_bottleneck_layers." + s() + ".weight").data(); mw = t("conv1D_compression_layers." + s() + ".weight").data(); }
    }
    const std::vector<float>& t(const std::string& name) const { return m.at(name).data; }
    std::string s() const { return std::to_string(l); }
    float conv(int o, int cc, int tap) const {                 // cc: canonical channel
        const int ci = l == 0 ? n.ref_channel(cc) : (cc < n.cin(l) ? cc : -1);
        if (o >= n.cout(l) || ci < 0) return 0.f;
        return cw[((size_t)o * n.cin(l) + ci) * 3 + tap];
    }
    float res(int o, int cc) const {
        if (o >= n.cout(l) || cc >= n.cout(l)) return 0.f;
        return rw[(size_t)o * n.cout(l) + cc];
    }
    float bot(int o, int cc) const {
        if (o >= n.c.bottleneck || cc >= n.cout(l)) return 0.f;
        return bw[(size_t)o * n.cout(l) + cc];
    }
    float cmp(int o, int cc, int p) const {
        const int H = n.c.bottleneck;
        if (o >= H || cc >= H) return 0.f;
        return mw[((size_t)o * H + cc) * n.c.length + p];
    }
    // Winograd weight transforms, in double: F(2,3) for taps 4, F(4,3) for taps 6
    float wino(int o, int cc, int k, int taps) const {
        const double g0 = conv(o, cc, 0), g1 = conv(o, cc, 1), g2 = conv(o, cc, 2);
        if (taps == 4) {
            const double u[4] = {g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2};
            return (float)u[k];
        }
        const double u[6] = {g0 / 4.0, -(g0 + g1 + g2) / 6.0, -(g0 - g1 + g2) / 6.0, g0 / 24.0 + g1 / 12.0 + g2 / 6.0,
                             g0 / 24.0 - g1 / 12.0 + g2 / 6.0, g2};
        return (float)u[k];
    }
    // the constants [bias 128][scale 128][shift 128][bres 128][bbot 32]
    std::vector<float> constants() const {
        std::vector<float> k(CST_FLOATS, 0.f);
        const int co = n.cout(l);
        for (int o = 0; o < co; ++o) {
            k[o] = t("conv1D_layers." + s() + ".bias")[o];
            k[128 + o] = 1.f;
            if (n.c.use_bn) {
                const std::string q = "bn1D_layers." + s();
                const double sc = (double)t(q + ".weight")[o] / std::sqrt((double)t(q + ".running_var")[o] + 1e-5);
                k[128 + o] = (float)sc;
                k[256 + o] = (float)((double)t(q + ".bias")[o] - (double)t(q + ".running_mean")[o] * sc);
            }
            if (n.residual(l)) k[384 + o] = t("residual_conv_layers." + std::to_string(l + 1 - n.c.residual_start) + ".bias")[o];
        }
        for (int o = 0; o < n.c.bottleneck; ++o) k[512 + o] = t("conv1D_bottleneck_layers." + s() + ".bias")[o];
        return k;
    }
};

// ---- the layouts, as index formulas ---------------------------------------------------------------------------------------------
// fp32 16x16x4 fragments: [tap][kg][tile][lane 64][4], lane = (o & 15) + 16 ((c & 15) >> 2), s = c & 3
static size_t idx_f32(int o, int c, int tap, int kg, int tiles) {
    return ((((size_t)tap * kg + c / 16) * tiles + o / 16) * 64 + (o % 16) + 16 * ((c % 16) / 4)) * 4 + c % 4;
}
// bf16 32x32x16 fragments of 512 elements: fragment (ks * taps + t) * nq + q; row m of quarter q is channel 32 q + 16 ((m >> 2) & 1)
// + 4 (m >> 3) + (m & 3); lane = m + 32 (k-half), j = c & 7
static size_t idx_p(int o, int c, int tap, int taps, int nq) {
    const int r = o % 32, m = ((r % 16) / 4) * 8 + (r / 16) * 4 + r % 4;
    return (((size_t)(c / 16) * taps + tap) * nq + o / 32) * 512 + (size_t)(m + 32 * ((c % 16) / 8)) * 8 + c % 8;
}
// bf16 16x16x32 fragments: fragment (((ks * taps + t) * n_ct + ct) * planes + plane); row r of tile ct is channel 32 (ct >> 1) +
// 8 (r >> 2) + 4 (ct & 1) + (r & 3); lane = r + 16 (k-quarter), j = c & 7
static size_t idx_16(int o, int c, int tap, int taps, int n_ct, int planes, int plane) {
    const int rem = o % 32, ct = 2 * (o / 32) + (rem % 8) / 4, r = 4 * (rem / 8) + rem % 4;
    return ((((size_t)(c / 32) * taps + tap) * n_ct + ct) * planes + plane) * 512 + (size_t)(r + 16 * ((c % 32) / 8)) * 8 + c % 8;
}

template <class W>
static void read_f32(Reader<float>& rd, size_t base, int taps, int kg, int tiles, W w) {
    for (int o = 0; o < 16 * tiles; ++o)
        for (int c = 0; c < 16 * kg; ++c)
            for (int t = 0; t < taps; ++t) rd.is(base + idx_f32(o, c, t, kg, tiles), w(o, c, t));
}
template <class W>
static void read_p(Reader<uint16_t>& rd, size_t base, int taps, int ksteps, int nq, W w) {
    for (int o = 0; o < 32 * nq; ++o)
        for (int c = 0; c < 16 * ksteps; ++c)
            for (int t = 0; t < taps; ++t) rd.is(base + idx_p(o, c, t, taps, nq), to_bf16(w(o, c, t)));
}
template <class W>
static void read_16(Reader<uint16_t>& rd, size_t base, int taps, int ksteps, int n_ct, int planes, W w) {
    for (int o = 0; o < 16 * n_ct; ++o)
        for (int c = 0; c < 32 * ksteps; ++c)
            for (int t = 0; t < taps; ++t) {
                const float v = w(o, c, t);
                const uint16_t hi = to_bf16(v);
                rd.is(base + idx_16(o, c, t, taps, n_ct, planes, 0), hi);
                if (planes == 2) rd.is(base + idx_16(o, c, t, taps, n_ct, planes, 1), to_bf16(v - from_bf16(hi)));
            }
}
template <class T>
static void read_floats(Reader<T>& rd, size_t base_bytes, const std::vector<float>& want) {   // fp32 constants inside a block of T
    for (size_t i = 0; i < want.size(); ++i) {
        T part[sizeof(float) / sizeof(T)];
        memcpy(part, &want[i], sizeof(float));
        for (size_t k = 0; k < sizeof(float) / sizeof(T); ++k) rd.is(base_bytes / sizeof(T) + i * (sizeof(float) / sizeof(T)) + k, part[k]);
    }
}

static void check_network(const Net& n, int precision) {
    const dan_config& c = n.c;
    const TensorMap m = make_tensors(n);
    const std::vector<int> seg = n.seg_begin();
    const PackFamily fam{precision, precision != 0, precision == 2};
    Packed pk;
    std::string err;
    const int rc = pack_network(c, m, seg, fam, &pk, err);
    expect(rc == 0 && err.empty(), "pack_network");
    if (rc) { printf("pack_network: %d %s\n", rc, err.c_str()); return; }
    const int L = c.length, H = c.bottleneck, layers = c.layers;
    unsigned mask = 0;
    for (int l = 0; l < layers; ++l) if (n.residual(l)) mask |= 1u << l;
    expect(pk.res_mask == mask, "res_mask");
    expect(pk.emb == &m.at("embeddings.weight") && pk.pe == &m.at("pe"), "emb / pe");

    // ---- fp32 blocks (every precision): [layer][LAYER_STRIDE]
    expect(pk.wl.size() == (size_t)layers * LAYER_STRIDE, "wl size");
    Reader<float> wl(pk.wl.data(), pk.wl.size(), "wl");
    for (int l = 0; l < layers; ++l) {
        const Layer y(n, m, l);
        const size_t b = (size_t)l * LAYER_STRIDE;
        read_f32(wl, b + 0, 3, l == 0 ? 3 : 8, 8, [&](int o, int cc, int t) { return y.conv(o, cc, t); });
        if (l > 0) {
            read_f32(wl, b + 70208, 4, 8, 8, [&](int o, int cc, int k) { return y.wino(o, cc, k, 4); });
            read_f32(wl, b + 135744, 6, 8, 8, [&](int o, int cc, int k) { return y.wino(o, cc, k, 6); });
        }
        if (n.residual(l)) read_f32(wl, b + 49152, 1, 8, 8, [&](int o, int cc, int) { return y.res(o, cc); });
        if (H > 0) read_f32(wl, b + 65536, 1, 8, 2, [&](int o, int cc, int) { return y.bot(o, cc); });
        read_floats(wl, (b + 69632) * sizeof(float), y.constants());
    }
    wl.rest_is_zero();

    // ---- layer 1 by table (precision 0): TJ [tap 3][101][128] | W_sc [5][tap 3][128] | PE [variant 3][column][128]
    expect(pk.l0tab.size() == (precision == 0 ? (size_t)40704 + (size_t)3 * L * 128 : 0), "l0tab size");
    if (precision == 0) {
        const Layer y(n, m, 0);
        const std::vector<float>&emb = m.at("embeddings.weight").data, &pe = m.at("pe").data;
        Reader<float> tab(pk.l0tab.data(), pk.l0tab.size(), "l0tab");
        for (int t = 0; t < 3; ++t)
            for (int o = 0; o < 128; ++o) {
                for (int tok = 0; tok < 10; ++tok)
                    for (int ref = 0; ref < 10; ++ref) {
                        double v = 0.0;
                        for (int e = 0; e < 20; ++e) v += (double)y.conv(o, e, t) * emb[tok * 20 + e] + (double)y.conv(o, 20 + e, t) * emb[ref * 20 + e];
                        tab.is(((size_t)t * 101 + 10 * tok + ref) * 128 + o, (float)v);
                    }
                for (int k = 0; k < 5; ++k) tab.is(38784 + ((size_t)k * 3 + t) * 128 + o, y.conv(o, 40 + k, t));
            }
        auto pos = [&](int t, int w, int o) {                    // the positional term of tap t at column w
            double v = 0.0;
            for (int e = 0; e < 20; ++e) v += ((double)y.conv(o, e, t) + (double)y.conv(o, 20 + e, t)) * pe[(size_t)w * 20 + e];
            return v;
        };
        for (int var = 0; var < 3; ++var)                        // 0: both neighbours, 1: no left neighbour, 2: no right neighbour
            for (int w = 0; w < L; ++w)
                for (int o = 0; o < 128; ++o) {
                    double v = pos(1, w, o);
                    if (var != 1 && w > 0) v += pos(0, w - 1, o);
                    if (var != 2 && w + 1 < L) v += pos(2, w + 1, o);
                    tab.is(40704 + ((size_t)var * L + w) * 128 + o, (float)v);
                }
        tab.rest_is_zero();
    }

    // ---- plain bf16 (precision 2): 32x32x16 blocks (wlp) and 16x16x32 blocks (wlr), [layer][WP_LAYER_BYTES]
    expect(pk.wlp.size() == (precision == 2 ? (size_t)layers * WP_LAYER_BYTES : 0) && pk.wlr.size() == pk.wlp.size(), "wlp / wlr size");
    if (precision == 2) {
        Reader<uint16_t> p((const uint16_t*)pk.wlp.data(), pk.wlp.size() / 2, "wlp"), r((const uint16_t*)pk.wlr.data(), pk.wlr.size() / 2, "wlr");
        for (int l = 0; l < layers; ++l) {
            const Layer y(n, m, l);
            const size_t b = (size_t)l * WP_LAYER_BYTES / 2;
            auto cv = [&](int o, int cc, int t) { return y.conv(o, cc, t); };
            auto rs = [&](int o, int cc, int) { return y.res(o, cc); };
            auto bt = [&](int o, int cc, int) { return y.bot(o, cc); };
            read_p(p, b + 0, 3, l == 0 ? 3 : 8, 4, cv);
            read_16(r, b + 0, 3, l == 0 ? 2 : 4, 8, 1, cv);
            if (n.residual(l)) { read_p(p, b + 98304 / 2, 1, 8, 4, rs); read_16(r, b + 98304 / 2, 1, 4, 8, 1, rs); }
            if (H > 0) { read_p(p, b + 131072 / 2, 1, 8, 1, bt); read_16(r, b + 131072 / 2, 1, 4, 2, 1, bt); }
            read_floats(p, b * 2 + 139264, y.constants());
            read_floats(r, b * 2 + 139264, y.constants());
        }
        p.rest_is_zero();
        r.rest_is_zero();
    }

    // ---- bf16x3 (precision 1): hi / lo 16x16x32 blocks, [layer][WX_LAYER_BYTES]; bias slot -b, shift slot sh + b sc
    expect(pk.wlx.size() == (precision == 1 ? (size_t)layers * WX_LAYER_BYTES : 0), "wlx size");
    if (precision == 1) {
        Reader<uint16_t> x((const uint16_t*)pk.wlx.data(), pk.wlx.size() / 2, "wlx");
        for (int l = 0; l < layers; ++l) {
            const Layer y(n, m, l);
            const size_t b = (size_t)l * WX_LAYER_BYTES / 2;
            read_16(x, b + 0, 3, l == 0 ? 2 : 4, 8, 2, [&](int o, int cc, int t) { return y.conv(o, cc, t); });
            if (n.residual(l)) read_16(x, b + 196608 / 2, 1, 4, 8, 2, [&](int o, int cc, int) { return y.res(o, cc); });
            if (H > 0) read_16(x, b + 262144 / 2, 1, 4, 2, 2, [&](int o, int cc, int) { return y.bot(o, cc); });
            std::vector<float> k = y.constants();
            for (int ch = 0; ch < 128; ++ch) {
                const double bias = k[ch];
                k[256 + ch] = (float)((double)k[256 + ch] + bias * (double)k[128 + ch]);
                k[ch] = (float)-bias;
            }
            read_floats(x, b * 2 + 278528, k);
        }
        x.rest_is_zero();
    }

    // ---- conv(pool) (precisions 1 and 2): [segment][o 128][tap 3][c 128] of the layer behind each pool layer; 128 zeros
    expect(pk.wpool.size() == (precision != 0 ? seg.size() * 128 * 3 * 128 : 0), "wpool size");
    expect(pk.zero.size() == (precision != 0 && seg.size() > 1 ? 128u : 0u), "zero size");
    if (precision != 0) {
        Reader<float> wp(pk.wpool.data(), pk.wpool.size(), "wpool");
        for (size_t sg = 1; sg < seg.size(); ++sg) {
            const Layer y(n, m, seg[sg]);
            for (int o = 0; o < 128; ++o)
                for (int t = 0; t < 3; ++t)
                    for (int cc = 0; cc < 128; ++cc) {
                        const float w = y.conv(o, cc, t);
                        wp.is(((sg * 128 + o) * 3 + t) * 128 + cc, precision == 2 ? from_bf16(to_bf16(w)) : w);
                    }
        }
        wp.rest_is_zero();
        for (float z : pk.zero) expect(z == 0.f, "zero");
    }

    // ---- highway: fp32 [layer][g = 2 pos + (c >> 4)][tile 2][lane 64][4], bias [layer][32], bf16 planes [layer][pos][tile 2][plane 2][lane 64][8]
    const size_t hwl = (size_t)L * 1024;
    expect(pk.wc.size() == (H > 0 ? layers * hwl : 0) && pk.bc.size() == (size_t)layers * 32, "wc / bc size");
    expect(pk.wc16.size() == (H > 0 && precision == 2 ? layers * hwl : 0), "wc16 size");
    Reader<float> wc(pk.wc.data(), pk.wc.size(), "wc"), bc(pk.bc.data(), pk.bc.size(), "bc");
    Reader<uint16_t> w16((const uint16_t*)pk.wc16.data(), pk.wc16.size() * 2, "wc16");
    for (int l = 0; l < layers && H > 0; ++l) {
        const Layer y(n, m, l);
        for (int o = 0; o < 32; ++o)
            for (int cc = 0; cc < 32; ++cc)
                for (int p = 0; p < L; ++p) {
                    const float w = y.cmp(o, cc, p);
                    wc.is(l * hwl + (((size_t)(2 * p + cc / 16) * 2 + o / 16) * 64 + o % 16 + 16 * ((cc % 16) / 4)) * 4 + cc % 4, w);
                    if (precision == 2) {
                        const uint16_t hi = to_bf16(w);
                        const size_t lane = o % 16 + 16 * (cc / 8), e = ((size_t)p * 2 + o / 16) * 2;
                        w16.is(l * hwl * 2 + ((e + 0) * 64 + lane) * 8 + cc % 8, hi);
                        w16.is(l * hwl * 2 + ((e + 1) * 64 + lane) * 8 + cc % 8, to_bf16(w - from_bf16(hi)));
                    }
                }
        for (int o = 0; o < H; ++o) bc.is((size_t)l * 32 + o, m.at("conv1D_compression_layers." + std::to_string(l) + ".bias").data[o]);
    }
    wc.rest_is_zero(); bc.rest_is_zero(); w16.rest_is_zero();

    // ---- FC stack and heads
    const int n0 = c.fc_sizes[0], n1 = c.fc_sizes[1];
    const size_t Fs = ((size_t)n.F + 15) / 16 * 16, n0s = ((size_t)n0 + 15) / 16 * 16;
    const std::vector<float>&w0 = m.at("fc.0.weight").data, &w1 = m.at("fc.1.weight").data;
    expect(pk.fc0 == (precision == 0 ? &m.at("fc.0.weight") : nullptr), "fc0");
    expect(pk.w0x.size() == (precision == 0 ? 0 : 2 * n0 * Fs), "w0x size");
    if (precision != 0) {
        Reader<uint16_t> x(pk.w0x.data(), pk.w0x.size(), "w0x");
        for (int o = 0; o < n0; ++o)
            for (int k = 0; k < n.F; ++k) {
                const float w = w0[(size_t)o * n.F + k];
                const uint16_t hi = to_bf16(w);
                x.is(o * Fs + k, hi);
                x.is(n0 * Fs + o * Fs + k, to_bf16(w - from_bf16(hi)));
            }
        x.rest_is_zero();
    }
    expect(pk.w1.size() == n1 * n0s, "w1 size");
    Reader<float> r1(pk.w1.data(), pk.w1.size(), "w1");
    for (int o = 0; o < n1; ++o) for (int k = 0; k < n0; ++k) r1.is(o * n0s + k, w1[(size_t)o * n0 + k]);
    r1.rest_is_zero();
    expect(pk.b0 == m.at("fc.0.bias").data && pk.b1 == m.at("fc.1.bias").data, "fc biases");
    std::vector<float> wh, bh;
    for (auto& hd : HEADS) {
        const Tensor &w = m.at(std::string(hd.name) + ".weight"), &b = m.at(std::string(hd.name) + ".bias");
        wh.insert(wh.end(), w.data.begin(), w.data.end());
        bh.insert(bh.end(), b.data.begin(), b.data.end());
    }
    expect(wh.size() == (size_t)27 * n1 && pk.wh == wh && pk.bh == bh, "heads");
}

// a missing tensor and a wrong shape are refused with their codes and texts, whichever tensor it is
static void check_refusals(const Net& n) {
    const TensorMap m = make_tensors(n);
    const PackFamily fam{0, false, false};
    for (const auto& kv : m) {
        TensorMap less = m;
        less.erase(kv.first);
        Packed pk;
        std::string err;
        expect(pack_network(n.c, less, n.seg_begin(), fam, &pk, err) == DAN_ERR_MISSING_TENSOR, "missing: code");
        expect(err == "missing tensor '" + kv.first + "'", "missing: text");

        TensorMap wrong = m;
        Tensor& t = wrong[kv.first];
        std::string got, want;
        for (auto s : t.shape) want += std::to_string(s) + ",";
        t.shape.back() += 1;
        t.data.resize((size_t)t.numel());
        for (auto s : t.shape) got += std::to_string(s) + ",";
        err.clear();
        expect(pack_network(n.c, wrong, n.seg_begin(), fam, &pk, err) == DAN_ERR_SHAPE, "shape: code");
        expect(err == "tensor '" + kv.first + "' has shape (" + got + ") but the configuration needs (" + want + ")", "shape: text");
    }
}

static Net net(int reads, int length, int layers, int c_init, int c_final, unsigned pool_mask, int residual_start, int bn, int q, int strand,
               int mask, int bottleneck, int fc0, int fc1) {
    Net n{};
    dan_config& c = n.c;
    c.reads = reads; c.length = length; c.layers = layers; c.c_init = c_init; c.c_final = c_final; c.dil_mid = 2; c.dil_final = 2;
    c.pool_layers_mask = pool_mask; c.residual_start = residual_start; c.use_bn = bn; c.use_q = q; c.use_strand = strand; c.use_mask = mask;
    c.bottleneck = bottleneck; c.fc_sizes[0] = fc0; c.fc_sizes[1] = fc1;
    n.in0 = 40 + q + strand + 3 * mask;
    n.F = 2 * c_final * length + layers * bottleneck * reads;
    return n;
}

int main() {
    const Net nets[] = {
        //  R    L  layers ci   cf  pool          res bn q  s  m   H  fc0 fc1
        net(2,   8, 1,     16,  16, 0,            0,  0, 0, 0, 0,  0, 16, 16),
        net(3,  16, 3,     33,  16, 1u << 2,      2,  1, 1, 1, 1,  8, 32, 16),
        net(2,  16, 7,    128, 128, 1u << 2 | 1u << 5, 3, 1, 1, 0, 0, 32, 32, 16),
        net(1, 209, 3,     16,  33, 0,            2,  0, 0, 0, 1, 32, 24, 10),
        net(2,   8, 3,    128, 128, 1u << 1,      3,  0, 0, 1, 0,  0, 17, 16),
    };
    for (const Net& n : nets)
        for (int precision = 0; precision < 3; ++precision) check_network(n, precision);
    check_refusals(nets[1]);
    printf("%s: %lld checks, %lld mismatches\n", g_bad ? "FAILED" : "ok", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
