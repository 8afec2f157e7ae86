// net_load.hip -- parameter blob -> device weights of an az_net: the blob layouts, the packing of
// every layer into the kernels' formats (arithmetic in weight_pack.h; allocation and upload here), the
// same load from a blob in device memory (kernels in weight_pack.hip), random initialisation and the
// weight entry points of include/az_engine.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/az_engine.h"
#include "engine_internal.h"
#include "net.h"
#include "net_host.h"
#include "weight_pack.h"
#include "weight_pack_dev.h"

namespace {

using namespace wpack;

uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

size_t count_params(const az_net_desc& d) {
    const size_t F = d.channels, Ci = d.in_planes, HC = d.head_channels, PP = (size_t)d.pool * d.pool;
    size_t n = 0;
    auto conv = [&](size_t co, size_t ci, size_t k) { n += co * ci * k * k + (d.conv_bias ? co : 0) + 4 * co; };
    conv(F, Ci, 3);
    for (int i = 0; i < d.blocks; ++i) { conv(F, F, 3); conv(F, F, 3); }
    conv(HC, F, 1);
    n += (size_t)d.action_size * HC * PP + d.action_size;
    conv(HC, F, 1);
    n += (size_t)d.fc_hidden * HC * PP + d.fc_hidden;
    n += (size_t)d.fc_hidden + 1;
    return n;
}

// Blob layout of a rand-wire net: (count, init kind, fan_in) per state entry in the reference's
// state_dict order (oracle/randwire_oracle.param_shapes; kinds as az_net_init_random).
struct PSpec { size_t n; int kind; int fan_in; };
std::vector<PSpec> rw_spec(const az_net_desc& d, const std::vector<RwBlock>& rwb) {
    const int C = d.channels, R = C / 16, HC = d.head_channels, PP = d.pool * d.pool;
    std::vector<PSpec> s;
    auto conv = [&](int co, int ci, int k) { s.push_back({(size_t)co * ci * k * k, 0, ci * k * k}); };
    auto bn = [&](int co) { for (int kd = 2; kd <= 5; ++kd) s.push_back({(size_t)co, kd, 1}); };
    auto lin = [&](int o, int i) { s.push_back({(size_t)o * i, 0, i}); s.push_back({(size_t)o, 1, i}); };
    conv(C, d.in_planes, 3); bn(C);
    for (const RwBlock& b : rwb) {
        for (int v : b.plan.order)
            if (!b.plan.preds[v].empty()) { conv(C, (int)b.plan.preds[v].size() * C, 1); bn(C); }
        for (size_t k = 0; k < b.plan.order.size(); ++k) {
            conv(C, C, 3); bn(C); conv(C, C, 3); bn(C);
            lin(R, C); lin(C, R);
        }
        if (b.plan.outputs.size() > 1) { conv(C, (int)b.plan.outputs.size() * C, 1); bn(C); }
    }
    conv(HC, C, 1); bn(HC); lin(d.action_size, HC * PP);
    conv(HC, C, 1); bn(HC); lin(d.fc_hidden, HC * PP); lin(1, d.fc_hidden);
    return s;
}

// A weight buffer of net n, allocated from n->weights where it is still missing: a load after one
// that failed part-way allocates the rest, so the pool always ends up in the loader's order.
#define WBUF(p, cnt) do { if (!(p)) { if (int r_ = n->weights.alloc(&(p), (cnt))) return r_; } } while (0)

// The buffers of one layer [N][K = taps * C], in the order every loader allocates them: fp32 weights and
// bias; with `split` the bf16 hi / lo and fp16 copies and, for a 3x3 layer over whole 16-channel chunks,
// the five chunk-blocked piece sets (v5 / v6 / v7 convs; the fp16 pieces of AZ_PREC_F16X3) with bx / sx.
bool layer_blocked(int taps, int C) { return taps == 9 && C % 16 == 0; }
int alloc_layer(az_net* n, Layer& L, int N, int K, int taps, int C, bool split) {
    L.N = N; L.K = K; L.Kpad = (K + 31) / 32 * 32; L.taps = taps; L.C = C;
    const size_t nw = (size_t)N * K;
    WBUF(L.W, nw); WBUF(L.b, (size_t)N);
    if (split) {
        WBUF(L.Whi, nw); WBUF(L.Wlo, nw);
        WBUF(L.Wh16, nw);
        if (layer_blocked(taps, C)) {
            WBUF(L.Wbk_bf, nw); WBUF(L.Wbk_h, nw); WBUF(L.Wbk_lo, nw);
            WBUF(L.Wbk_fh, nw); WBUF(L.Wbk_fl, nw); WBUF(L.bx, (size_t)N); WBUF(L.sx, (size_t)N);
        }
    }
    return 0;
}
// k_smallnet's sets over L layers of F channels, and both FC layers as NC rows of K (wpack::fc_rows)
int alloc_smallnet(az_net* n, size_t L, size_t F) {
    const size_t ne = L * 9 * F * F, nb = L * F;
    WBUF(n->sm_W, ne); WBUF(n->sm_Wf, ne); WBUF(n->sm_Wxh, ne); WBUF(n->sm_Wxl, ne); WBUF(n->sm_b, nb);
    WBUF(n->sm_Wfh, ne); WBUF(n->sm_Wfl, ne); WBUF(n->sm_bx, nb); WBUF(n->sm_sx, nb);
    return 0;
}
int alloc_fc_rows(az_net* n, size_t NC, size_t K) {
    WBUF(n->fcx_hi, NC * K); WBUF(n->fcx_lo, NC * K);
    WBUF(n->fcf_hi, NC * K); WBUF(n->fcf_lo, NC * K); WBUF(n->fcf_rs, NC);
    return 0;
}

int upload_layer(az_net* n, Layer& L, const std::vector<float>& W, const std::vector<float>& b, int N, int K, int taps,
                 int C, bool split) {
    if (W.size() != (size_t)N * K || b.size() != (size_t)N) return az_fail(AZ_ERR_STATE, "layer size mismatch");
    if (int r = alloc_layer(n, L, N, K, taps, C, split)) return r;
    HIPCHK(hipMemcpy(L.W, W.data(), W.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(L.b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
    if (split) {
        std::vector<uint16_t> hi(W.size()), lo(W.size());
        split_bf16(W.data(), W.size(), hi.data(), lo.data());
        HIPCHK(hipMemcpy(L.Whi, hi.data(), hi.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(L.Wlo, lo.data(), lo.size() * 2, hipMemcpyHostToDevice));
        std::vector<uint16_t> h16(W.size());
        to_f16(W.data(), W.size(), h16.data());
        HIPCHK(hipMemcpy(L.Wh16, h16.data(), h16.size() * 2, hipMemcpyHostToDevice));
        if (layer_blocked(taps, C)) {
            std::vector<uint16_t> fh(W.size()), fl(W.size());
            std::vector<float> bx(N), sx(N);
            pow2_split_rows(W.data(), N, (size_t)9 * C, b.data(), fh.data(), fl.data(), bx.data(), sx.data());
            HIPCHK(hipMemcpy(L.Wbk_bf, chunk_blocked(hi, N, C).data(), W.size() * 2, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.Wbk_h, chunk_blocked(h16, N, C).data(), W.size() * 2, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.Wbk_lo, chunk_blocked(lo, N, C).data(), W.size() * 2, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.Wbk_fh, chunk_blocked(fh, N, C).data(), W.size() * 2, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.Wbk_fl, chunk_blocked(fl, N, C).data(), W.size() * 2, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.bx, bx.data(), N * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.sx, sx.data(), N * 4, hipMemcpyHostToDevice));
        }
    }
    return 0;
}

int load_heads(az_net* n, ParamCursor& pc);

int net_load(az_net* n, const float* blob) {
    const az_net_desc& d = n->d;
    ParamCursor pc{blob};
    const int F = d.channels;
    std::vector<float> W, b;
    const NetPacks pk = net_packs(net_shape(d, false));
    // k_smallnet weights: every 3x3 layer as [tap][n][c] over 64 channels (input conv zero-padded):
    // fp16 for k_smallnet_g, bf16 hi / lo parts for k_smallnet_x3 (AZ_PREC_BF16X3), scaled fp16 hi / lo
    // pieces for k_smallnet_x3<.., 2> (AZ_PREC_F16X3).  Decided by the shape alone, like every other
    // piece set: az_net_set_precision only switches the dispatch, so a load packs what any precision the
    // shape accepts will read, and the weight pool (net_weight_buffers) is the same whatever precision
    // the net had at any load
    // every layer's pieces (fp16, bf16 hi / lo, scaled fp16 hi / lo) are made from its [n][tap][c] rows, then
    // gathered to [tap][n][c]
    std::vector<uint16_t> smw, smh, sml, sfh, sfl;
    std::vector<float> smb, sbx, ssx;
    auto sm_add = [&](const std::vector<float>& Wl, const std::vector<float>& bl, int cl) {
        const size_t nw = Wl.size();
        std::vector<uint16_t> w16(nw), hi(nw), lo(nw), fh(nw), fl(nw);
        std::vector<float> bx(F), sx(F);
        to_f16(Wl.data(), nw, w16.data());
        split_bf16(Wl.data(), nw, hi.data(), lo.data());
        pow2_split_rows(Wl.data(), F, (size_t)9 * cl, bl.data(), fh.data(), fl.data(), bx.data(), sx.data());
        smallnet_append(smw, w16, F, cl); smallnet_append(smh, hi, F, cl); smallnet_append(sml, lo, F, cl);
        smallnet_append(sfh, fh, F, cl); smallnet_append(sfl, fl, F, cl);
        smb.insert(smb.end(), bl.begin(), bl.end());
        sbx.insert(sbx.end(), bx.begin(), bx.end());
        ssx.insert(ssx.end(), sx.begin(), sx.end());
    };
    fold_conv(pc, F, d.in_planes, 3, n->cin_pad, d.conv_bias, W, b);
    if (int r = upload_layer(n, n->in, W, b, F, 9 * n->cin_pad, 9, n->cin_pad, pk.in16)) return r;  // 16-bit copies: g8 input conv
    if (pk.in32) {
        std::vector<float> W32((size_t)F * 9 * 32, 0.0f);   // [F][9][32]: channels 16..31 zero
        for (size_t ot = 0; ot < (size_t)F * 9; ++ot) std::copy(&W[ot * 16], &W[ot * 16] + 16, &W32[ot * 32]);
        if (int r = upload_layer(n, n->in32, W32, b, F, 9 * 32, 9, 32, true)) return r;
    }
    if (pk.sm) sm_add(W, b, n->cin_pad);
    n->blk.resize(2 * d.blocks);
    for (int i = 0; i < 2 * d.blocks; ++i) {
        fold_conv(pc, F, F, 3, F, d.conv_bias, W, b);
        if (int r = upload_layer(n, n->blk[i], W, b, F, 9 * F, 9, F, pk.trunk16)) return r;
        if (pk.sm) sm_add(W, b, F);
    }
    if (pk.sm) {
        const size_t ne = smw.size();
        if (int r = alloc_smallnet(n, 2 * d.blocks + 1, F)) return r;
        HIPCHK(hipMemcpy(n->sm_W, smw.data(), ne * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_Wf, frag_major(smw, F).data(), ne * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_Wxh, frag_major(smh, F).data(), ne * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_Wxl, frag_major(sml, F).data(), ne * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_Wfh, frag_major(sfh, F).data(), ne * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_Wfl, frag_major(sfl, F).data(), ne * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_bx, sbx.data(), sbx.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_sx, ssx.data(), ssx.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->sm_b, smb.data(), smb.size() * 4, hipMemcpyHostToDevice));
    }
    if (int r = load_heads(n, pc)) return r;
    if (pc.off != n->nparams) return az_fail(AZ_ERR_ARG, "parameter blob size mismatch (%zu vs %zu)", pc.off, n->nparams);
    n->loaded = true;
    return 0;
}

// policy head: 1x1 conv + BN, FC over the flattened (c, y, x) pooled map; value head likewise
int load_heads(az_net* n, ParamCursor& pc) {
    const az_net_desc& d = n->d;
    const int F = d.channels, HC = d.head_channels, PP = d.pool * d.pool;
    std::vector<float> W, b;
    fold_conv(pc, HC, F, 1, F, d.conv_bias, W, b);
    if (int r = upload_layer(n, n->pconv, W, b, HC, F, 1, F, false)) return r;
    std::vector<float> hW = W, hb = b;                 // the combined head conv, policy rows first
    auto fc = [&](int out, int hc, int pp, std::vector<float>& Wt, std::vector<float>& bt) {
        const float* w = pc.take((size_t)out * hc * pp);
        const float* bb = pc.take(out);
        fc_perm(w, out, hc, pp, Wt);
        bt.assign(bb, bb + out);
    };
    fc(d.action_size, HC, PP, W, b);
    if (int r = upload_layer(n, n->pfc, W, b, d.action_size, HC * PP, 1, HC * PP, false)) return r;
    fold_conv(pc, HC, F, 1, F, d.conv_bias, W, b);
    if (int r = upload_layer(n, n->vconv, W, b, HC, F, 1, F, false)) return r;
    hW.insert(hW.end(), W.begin(), W.end());
    hb.insert(hb.end(), b.begin(), b.end());
    if (int r = upload_layer(n, n->hconv, hW, hb, 2 * HC, F, 1, F, false)) return r;
    fc(d.fc_hidden, HC, PP, W, b);
    if (int r = upload_layer(n, n->vfc1, W, b, d.fc_hidden, HC * PP, 1, HC * PP, false)) return r;
    {
        const float* w = pc.take(d.fc_hidden);
        const float* bb = pc.take(1);
        W.assign(w, w + d.fc_hidden);
        b.assign(bb, bb + 1);
        if (int r = upload_layer(n, n->vfc2, W, b, 1, d.fc_hidden, 1, d.fc_hidden, false)) return r;
    }
    // both FC layers as one matrix for k_fc_heads_x3 (wpack::fc_rows)
    {
        const int K = HC * PP, A = d.action_size, H = d.fc_hidden;
        std::vector<float> Wp((size_t)A * K), Wv((size_t)H * K);
        HIPCHK(hipMemcpy(Wp.data(), n->pfc.W, Wp.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(Wv.data(), n->vfc1.W, Wv.size() * 4, hipMemcpyDeviceToHost));
        const FcRows f = fc_rows(Wp.data(), A, Wv.data(), H, K);
        if (int r = alloc_fc_rows(n, f.NC, K)) return r;
        HIPCHK(hipMemcpy(n->fcx_hi, f.hi.data(), f.hi.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->fcx_lo, f.lo.data(), f.lo.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->fcf_hi, f.fh.data(), f.fh.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->fcf_lo, f.fl.data(), f.fl.size() * 2, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(n->fcf_rs, f.rs.data(), f.rs.size() * 4, hipMemcpyHostToDevice));
    }
    return 0;
}

// DDW-RandWire blob (rw_spec order): input conv, per block the routers (nodes() order, in-degree
// > 0), the nodes' residual blocks incl. SE, the output router; then the heads.
int net_load_rw(az_net* n, const float* blob) {
    const az_net_desc& d = n->d;
    const int F = d.channels, R = F / 16;
    ParamCursor pc{blob};
    std::vector<float> W, b;
    const NetPacks pk = net_packs(net_shape(d, true));
    fold_conv(pc, F, d.in_planes, 3, n->cin_pad, false, W, b);
    if (int r = upload_layer(n, n->in, W, b, F, 9 * n->cin_pad, 9, n->cin_pad, pk.in16)) return r;
    auto raw = [&](float** dst, size_t cnt) -> int {
        WBUF(*dst, cnt);
        HIPCHK(hipMemcpy(*dst, pc.take(cnt), cnt * 4, hipMemcpyHostToDevice));
        return 0;
    };
    for (RwBlock& blk : n->rwb) {
        const azrw::Plan& pl = blk.plan;
        for (int v : pl.order) {
            const int deg = (int)pl.preds[v].size();
            if (!deg) continue;
            fold_conv(pc, F, deg * F, 1, deg * F, false, W, b);
            if (int r = upload_layer(n, blk.node[v].router, W, b, F, deg * F, 1, deg * F, false)) return r;
        }
        for (int v : pl.order) {
            RwNode& nd = blk.node[v];
            const bool h16 = pk.trunk16;    // 16-bit weight copies: the node convs on conv3x3_v4
            fold_conv(pc, F, F, 3, F, false, W, b);
            if (int r = upload_layer(n, nd.c1, W, b, F, 9 * F, 9, F, h16)) return r;
            fold_conv(pc, F, F, 3, F, false, W, b);
            if (int r = upload_layer(n, nd.c2, W, b, F, 9 * F, 9, F, h16)) return r;
            if (int r = raw(&nd.w1, (size_t)R * F)) return r;
            if (int r = raw(&nd.b1, R)) return r;
            if (int r = raw(&nd.w2, (size_t)F * R)) return r;
            if (int r = raw(&nd.b2, F)) return r;
        }
        const int no = (int)pl.outputs.size();
        if (no > 1) {
            fold_conv(pc, F, no * F, 1, no * F, false, W, b);
            if (int r = upload_layer(n, blk.out_router, W, b, F, no * F, 1, no * F, false)) return r;
        }
    }
    if (int r = load_heads(n, pc)) return r;
    if (pc.off != n->nparams) return az_fail(AZ_ERR_ARG, "parameter blob size mismatch (%zu vs %zu)", pc.off, n->nparams);
    n->loaded = true;
    return 0;
}

// ---- the same loads from a blob in device memory (az_net_load_weights_device): the walks above with
// the kernels of weight_pack.hip on stream st in place of the host loops and uploads.  They share the
// allocation helpers, so a first load leaves the pool in the same order, and write every byte of every
// buffer (the host's zero padding included).  No host work per element, nothing waits before the end.
#define WPCHK(x)                                                                                         \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) return az_fail(AZ_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

struct ConvSrc { const float *w, *cb, *g, *be, *mu, *var; };   // one conv + BN of the blob (device pointers)
ConvSrc take_conv(ParamCursor& pc, int co, int ci, int taps, bool has_bias) {
    ConvSrc s;
    s.w = pc.take((size_t)co * ci * taps);
    s.cb = has_bias ? pc.take(co) : nullptr;
    s.g = pc.take(co); s.be = pc.take(co); s.mu = pc.take(co); s.var = pc.take(co);
    return s;
}
wpdev::Fold fold_of(const ConvSrc& s, int co, int ci, int taps, int cpad, float* W, float* b) {
    return wpdev::Fold{s.w, s.cb, s.g, s.be, s.mu, s.var, co, ci, taps, cpad, W, b};
}

// fold_conv + upload_layer: ci input channels of the blob folded into C (>= ci) channels per tap
int dev_layer(az_net* n, Layer& L, const ConvSrc& s, int N, int ci, int taps, int C, bool split, hipStream_t st) {
    if (int r = alloc_layer(n, L, N, taps * C, taps, C, split)) return r;
    WPCHK(wpdev::fold(st, fold_of(s, N, ci, taps, C, L.W, L.b)));
    if (!split) return 0;
    wpdev::Rows rp{};
    rp.W = L.W; rp.b = L.b; rp.N = N; rp.taps = taps; rp.C = C;
    rp.hi = L.Whi; rp.lo = L.Wlo; rp.h16 = L.Wh16;
    if (layer_blocked(taps, C)) {
        rp.bk_bf = L.Wbk_bf; rp.bk_h = L.Wbk_h; rp.bk_lo = L.Wbk_lo; rp.bk_fh = L.Wbk_fh; rp.bk_fl = L.Wbk_fl;
        rp.bx = L.bx; rp.sx = L.sx;
    }
    WPCHK(wpdev::rows(st, rp));
    return 0;
}

// layer l of the k_smallnet sets from the folded layer L (sm_add, smallnet_append and frag_major)
int dev_smallnet_layer(az_net* n, const Layer& L, int l, hipStream_t st) {
    wpdev::Rows rp{};
    rp.W = L.W; rp.b = L.b; rp.N = L.N; rp.taps = 9; rp.C = L.C;
    rp.sm_w = n->sm_W; rp.sm_wf = n->sm_Wf; rp.sm_xh = n->sm_Wxh; rp.sm_xl = n->sm_Wxl; rp.sm_fh = n->sm_Wfh; rp.sm_fl = n->sm_Wfl;
    rp.sm_b = n->sm_b; rp.sm_bx = n->sm_bx; rp.sm_sx = n->sm_sx;
    rp.sm_l = l; rp.F = n->d.channels;
    WPCHK(wpdev::rows(st, rp));
    return 0;
}

int dev_load_heads(az_net* n, ParamCursor& pc, hipStream_t st) {
    const az_net_desc& d = n->d;
    const int F = d.channels, HC = d.head_channels, PP = d.pool * d.pool, K = HC * PP, A = d.action_size, H = d.fc_hidden;
    // an FC layer [out][hc][pp] + bias: fc_perm and the raw bias
    auto fc = [&](Layer& L, int out) -> int {
        const float* w = pc.take((size_t)out * K);
        const float* bb = pc.take(out);
        if (int r = alloc_layer(n, L, out, K, 1, K, false)) return r;
        WPCHK(wpdev::fold(st, wpdev::Fold{w, nullptr, nullptr, nullptr, nullptr, nullptr, out, HC, PP, HC, L.W, nullptr}));
        WPCHK(wpdev::copy_f32(st, bb, L.b, out));
        return 0;
    };
    const ConvSrc ps = take_conv(pc, HC, F, 1, d.conv_bias);
    if (int r = dev_layer(n, n->pconv, ps, HC, F, 1, F, false, st)) return r;
    if (int r = fc(n->pfc, A)) return r;
    const ConvSrc vs = take_conv(pc, HC, F, 1, d.conv_bias);
    if (int r = dev_layer(n, n->vconv, vs, HC, F, 1, F, false, st)) return r;
    if (int r = alloc_layer(n, n->hconv, 2 * HC, F, 1, F, false)) return r;   // the combined head conv, policy rows first
    WPCHK(wpdev::fold(st, fold_of(ps, HC, F, 1, F, n->hconv.W, n->hconv.b)));
    WPCHK(wpdev::fold(st, fold_of(vs, HC, F, 1, F, n->hconv.W + (size_t)HC * F, n->hconv.b + HC)));
    if (int r = fc(n->vfc1, H)) return r;
    {
        const float* w = pc.take(H);
        const float* bb = pc.take(1);
        if (int r = alloc_layer(n, n->vfc2, 1, H, 1, H, false)) return r;
        WPCHK(wpdev::copy_f32(st, w, n->vfc2.W, H));
        WPCHK(wpdev::copy_f32(st, bb, n->vfc2.b, 1));
    }
    // both FC layers as one matrix (wpack::fc_rows): the padded rows zero with scale 1
    const int NTP = (A + 63) / 64, NTV = (H + 63) / 64, NC = (NTP + NTV) * 64;
    if (int r = alloc_fc_rows(n, NC, K)) return r;
    auto put = [&](const Layer& L, int rows, int r0, int r1) -> int {   // rows r0 .. r0 + rows from L, zero up to r1
        const size_t o = (size_t)r0 * K, z = (size_t)(r0 + rows) * K, nz = (size_t)(r1 - r0 - rows) * K;
        wpdev::Rows rp{};
        rp.W = L.W; rp.N = rows; rp.taps = 1; rp.C = K;
        rp.hi = n->fcx_hi + o; rp.lo = n->fcx_lo + o; rp.fh = n->fcf_hi + o; rp.fl = n->fcf_lo + o; rp.sx = n->fcf_rs + r0;
        WPCHK(wpdev::rows(st, rp));
        for (uint16_t* p : {n->fcx_hi, n->fcx_lo, n->fcf_hi, n->fcf_lo}) WPCHK(wpdev::fill_u16(st, p + z, nz, 0));
        WPCHK(wpdev::fill_f32(st, n->fcf_rs + r0 + rows, (size_t)(r1 - r0 - rows), 1.0f));
        return 0;
    };
    if (int r = put(n->pfc, A, 0, NTP * 64)) return r;
    if (int r = put(n->vfc1, H, NTP * 64, NC)) return r;
    return 0;
}

int net_load_dev(az_net* n, const float* d_blob, hipStream_t st) {
    const az_net_desc& d = n->d;
    ParamCursor pc{d_blob};
    const int F = d.channels;
    const NetPacks pk = net_packs(net_shape(d, false));
    const ConvSrc in = take_conv(pc, F, d.in_planes, 9, d.conv_bias);
    if (int r = dev_layer(n, n->in, in, F, d.in_planes, 9, n->cin_pad, pk.in16, st)) return r;
    if (pk.in32)   // [F][9][32]: the same conv folded into 32 channels
        if (int r = dev_layer(n, n->in32, in, F, d.in_planes, 9, 32, true, st)) return r;
    n->blk.resize(2 * d.blocks);
    for (int i = 0; i < 2 * d.blocks; ++i) {
        const ConvSrc s = take_conv(pc, F, F, 9, d.conv_bias);
        if (int r = dev_layer(n, n->blk[i], s, F, F, 9, F, pk.trunk16, st)) return r;
    }
    if (pk.sm) {
        if (int r = alloc_smallnet(n, 2 * d.blocks + 1, F)) return r;
        if (int r = dev_smallnet_layer(n, n->in, 0, st)) return r;
        for (int i = 0; i < 2 * d.blocks; ++i)
            if (int r = dev_smallnet_layer(n, n->blk[i], i + 1, st)) return r;
    }
    if (int r = dev_load_heads(n, pc, st)) return r;
    if (pc.off != n->nparams) return az_fail(AZ_ERR_ARG, "parameter blob size mismatch (%zu vs %zu)", pc.off, n->nparams);
    n->loaded = true;
    return 0;
}

int net_load_rw_dev(az_net* n, const float* d_blob, hipStream_t st) {
    const az_net_desc& d = n->d;
    const int F = d.channels, R = F / 16;
    ParamCursor pc{d_blob};
    const NetPacks pk = net_packs(net_shape(d, true));
    if (int r = dev_layer(n, n->in, take_conv(pc, F, d.in_planes, 9, false), F, d.in_planes, 9, n->cin_pad, pk.in16, st)) return r;
    auto raw = [&](float** dst, size_t cnt) -> int {
        WBUF(*dst, cnt);
        WPCHK(wpdev::copy_f32(st, pc.take(cnt), *dst, cnt));
        return 0;
    };
    for (RwBlock& blk : n->rwb) {
        const azrw::Plan& pl = blk.plan;
        for (int v : pl.order) {
            const int deg = (int)pl.preds[v].size();
            if (!deg) continue;
            if (int r = dev_layer(n, blk.node[v].router, take_conv(pc, F, deg * F, 1, false), F, deg * F, 1, deg * F, false, st)) return r;
        }
        for (int v : pl.order) {
            RwNode& nd = blk.node[v];
            if (int r = dev_layer(n, nd.c1, take_conv(pc, F, F, 9, false), F, F, 9, F, pk.trunk16, st)) return r;
            if (int r = dev_layer(n, nd.c2, take_conv(pc, F, F, 9, false), F, F, 9, F, pk.trunk16, st)) return r;
            if (int r = raw(&nd.w1, (size_t)R * F)) return r;
            if (int r = raw(&nd.b1, R)) return r;
            if (int r = raw(&nd.w2, (size_t)F * R)) return r;
            if (int r = raw(&nd.b2, F)) return r;
        }
        const int no = (int)pl.outputs.size();
        if (no > 1)
            if (int r = dev_layer(n, blk.out_router, take_conv(pc, F, no * F, 1, false), F, no * F, 1, no * F, false, st)) return r;
    }
    if (int r = dev_load_heads(n, pc, st)) return r;
    if (pc.off != n->nparams) return az_fail(AZ_ERR_ARG, "parameter blob size mismatch (%zu vs %zu)", pc.off, n->nparams);
    n->loaded = true;
    return 0;
}

// The host copy of the canonical blob after a device load: fetched when first asked for.
int refresh_host_blob(az_net* n) {
    if (!n->host_stale) return 0;
    n->host_blob.resize(n->nparams);
    HIPCHK(hipSetDevice(n->e->device));
    HIPCHK(hipMemcpyAsync(n->host_blob.data(), n->d_blob, n->nparams * 4, hipMemcpyDeviceToHost, n->e->stream));
    HIPCHK(hipStreamSynchronize(n->e->stream));
    n->host_stale = false;
    return 0;
}

}  // namespace

size_t net_blob_params(const az_net* n) {
    if (!n->rw) return count_params(n->d);
    size_t total = 0;
    for (const PSpec& ps : rw_spec(n->d, n->rwb)) total += ps.n;
    return total;
}

// ---- net internals for dist.hip (engine_internal.h), C++ linkage
int net_weight_buffers(az_net* n, std::vector<DevPool::Buf>& out) {
    if (!n->loaded) {
        // no load completed: a load of zero weights allocates every weight buffer still missing, which
        // a broadcast then overwrites (host work once per net, no device traffic beyond the uploads)
        std::vector<float> zero(n->nparams, 0.0f);
        if (int r = n->rw ? net_load_rw(n, zero.data()) : net_load(n, zero.data())) return r;
        HIPCHK(hipDeviceSynchronize());
        n->loaded = false;
    }
    out = n->weights.bufs;
    return 0;
}
const std::vector<float>& net_host_blob(az_net* n) {
    if (refresh_host_blob(n)) n->host_blob.clear();   // the callers take a blob of another size as "not loaded"
    return n->host_blob;
}
size_t net_param_count(az_net* n) { return n->nparams; }
az_engine* net_engine(az_net* n) { return n->e; }
std::mutex& net_mutex(az_net* n) { return n->mu; }
void net_adopt_blob(az_net* n, const float* blob) {
    n->host_blob.assign(blob, blob + n->nparams);
    n->host_stale = false;
    n->loaded = true;
}

extern "C" {

int az_net_num_params(az_net* n, size_t* count) {
    if (!n || !count) return az_fail(AZ_ERR_ARG, "null argument");
    *count = n->nparams;
    return 0;
}

int az_net_load_weights(az_net* n, const float* blob, size_t count) {
    if (!n || !blob) return az_fail(AZ_ERR_ARG, "null argument");
    if (count != n->nparams) return az_fail(AZ_ERR_ARG, "expected %zu parameters, got %zu", n->nparams, count);
    std::lock_guard<std::mutex> lk(n->mu);
    HIPCHK(hipSetDevice(n->e->device));
    if (int r = n->rw ? net_load_rw(n, blob) : net_load(n, blob)) return r;
    HIPCHK(hipDeviceSynchronize());   // null-stream uploads done before the non-blocking stream reads them
    n->host_blob.assign(blob, blob + count);
    n->host_stale = false;
    return 0;
}

int az_net_load_weights_device(az_net* n, const float* d_blob, size_t count) {
    if (!n || !d_blob) return az_fail(AZ_ERR_ARG, "null argument");
    if (count != n->nparams) return az_fail(AZ_ERR_ARG, "expected %zu parameters, got %zu", n->nparams, count);
    std::lock_guard<std::mutex> lk(n->mu);
    HIPCHK(hipSetDevice(n->e->device));
    hipStream_t st = n->e->stream;
    if (!n->d_blob)
        if (int r = n->blob.alloc(&n->d_blob, n->nparams)) return r;
    // with az_net_profile on: HIP events around the pack launches (az_diag_net_pack_ms)
    struct Events {
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    } tm;
    n->pack_ms = -1.0;
    if (n->prof) {
        for (hipEvent_t& e : tm.ev) HIPCHK(hipEventCreate(&e));
        HIPCHK(hipEventRecord(tm.ev[0], st));
    }
    if (int r = n->rw ? net_load_rw_dev(n, d_blob, st) : net_load_dev(n, d_blob, st)) return r;
    if (d_blob != n->d_blob) WPCHK(wpdev::copy_f32(st, d_blob, n->d_blob, count));
    if (n->prof) HIPCHK(hipEventRecord(tm.ev[1], st));
    HIPCHK(hipStreamSynchronize(st));   // the caller may overwrite d_blob; forwards on this stream are ordered anyway
    if (n->prof) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, tm.ev[0], tm.ev[1]));
        n->pack_ms = ms;
    }
    n->host_stale = true;
    return 0;
}

int az_diag_net_pack_ms(az_net* n, double* ms) {
    if (!n || !ms) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(n->mu);
    *ms = n->pack_ms;
    return 0;
}

// Diagnostics of the weight pool (tests/test_gpu_weight_publish.py): bytes that no forward reads are
// part of what a load must produce, since a broadcast sends whole buffers.
int az_diag_net_fill_weights(az_net* n, int byte) {
    if (!n) return az_fail(AZ_ERR_ARG, "null net");
    std::lock_guard<std::mutex> lk(n->mu);
    HIPCHK(hipSetDevice(n->e->device));
    std::vector<DevPool::Buf> bufs;
    if (int r = net_weight_buffers(n, bufs)) return r;
    for (const DevPool::Buf& b : bufs) HIPCHK(hipMemsetAsync(b.p, byte & 0xff, b.bytes, n->e->stream));
    HIPCHK(hipStreamSynchronize(n->e->stream));
    return 0;
}

int az_diag_net_compare_weights(az_net* a, az_net* b, int* buffer, size_t* byte) {
    if (!a || !b || !buffer || !byte || a == b) return az_fail(AZ_ERR_ARG, "bad argument");
    if (a->e->device != b->e->device) return az_fail(AZ_ERR_ARG, "nets on different devices");
    std::lock_guard<std::mutex> la(a->mu);
    std::lock_guard<std::mutex> lb(b->mu);
    HIPCHK(hipSetDevice(a->e->device));
    const std::vector<DevPool::Buf>&A = a->weights.bufs, &B = b->weights.bufs;
    if (A.size() != B.size()) return az_fail(AZ_ERR_ARG, "the nets differ (%zu and %zu weight buffers)", A.size(), B.size());
    *buffer = -1;
    *byte = 0;
    std::vector<uint8_t> ha, hb;
    for (size_t i = 0; i < A.size(); ++i) {
        if (A[i].bytes != B[i].bytes) return az_fail(AZ_ERR_ARG, "the nets differ (buffer %zu)", i);
        ha.resize(A[i].bytes); hb.resize(B[i].bytes);
        HIPCHK(hipMemcpyAsync(ha.data(), A[i].p, A[i].bytes, hipMemcpyDeviceToHost, a->e->stream));
        HIPCHK(hipMemcpyAsync(hb.data(), B[i].p, B[i].bytes, hipMemcpyDeviceToHost, a->e->stream));
        HIPCHK(hipStreamSynchronize(a->e->stream));
        const auto mm = std::mismatch(ha.begin(), ha.end(), hb.begin());
        if (mm.first != ha.end()) {
            *buffer = (int)i;
            *byte = (size_t)(mm.first - ha.begin());
            // az_last_error then shows the 16-byte line around the difference, a's then b's
            char hex[2][40];
            const size_t l0 = *byte / 16 * 16, l1 = std::min(l0 + 16, ha.size());
            for (int s = 0; s < 2; ++s) {
                const std::vector<uint8_t>& h = s ? hb : ha;
                for (size_t k = l0; k < l1; ++k) snprintf(hex[s] + 2 * (k - l0), 3, "%02x", h[k]);
            }
            return az_fail(0, "weight buffer %zu of %zu bytes differs at byte %zu: %s / %s", i, ha.size(), *byte, hex[0], hex[1]);
        }
    }
    return 0;
}

int az_net_get_weights(az_net* n, float* blob, size_t count) {
    if (!n || !blob) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(n->mu);
    if (!n->loaded) return az_fail(AZ_ERR_STATE, "weights not loaded");
    if (count != n->nparams) return az_fail(AZ_ERR_ARG, "expected %zu parameters, got %zu", n->nparams, count);
    if (int r = refresh_host_blob(n)) return r;
    std::copy(n->host_blob.begin(), n->host_blob.end(), blob);
    return 0;
}

// Counter-based init; tests/nn_weights.py restates it in numpy (same fp32 ops).
int az_net_init_random(az_net* n, uint64_t seed) {
    if (!n) return az_fail(AZ_ERR_ARG, "null net");
    const az_net_desc& d = n->d;
    std::vector<float> blob(n->nparams);
    size_t off = 0;
    int tensor = 0;
    auto fill = [&](size_t cnt, int kind, int fan_in) {
        // kind: 0 weight U(-1,1)/sqrt(fan_in); 1 bias U(-1,1)/sqrt(fan_in); 2 bn gamma 1+0.1u;
        //       3 bn beta 0.1u; 4 bn mean 0.1u; 5 bn var 1+0.25(u+1)
        const float bound = 1.0f / std::sqrt((float)fan_in);
        for (size_t i = 0; i < cnt; ++i) {
            const uint64_t r = splitmix64(seed ^ ((uint64_t)tensor << 40) ^ (uint64_t)i);
            const float u = (float)(int32_t)(r >> 40) * (1.0f / 8388608.0f) - 1.0f;
            float v;
            switch (kind) {
                case 0: case 1: v = u * bound; break;
                case 2: v = 1.0f + 0.1f * u; break;
                case 3: case 4: v = 0.1f * u; break;
                default: v = 1.0f + 0.25f * (u + 1.0f); break;
            }
            blob[off + i] = v;
        }
        off += cnt;
        ++tensor;
    };
    if (n->rw) {
        for (const PSpec& ps : rw_spec(d, n->rwb)) fill(ps.n, ps.kind, ps.fan_in);
        if (off != n->nparams) return az_fail(AZ_ERR_STATE, "init size mismatch");
        return az_net_load_weights(n, blob.data(), blob.size());
    }
    const int F = d.channels, HC = d.head_channels, PP = d.pool * d.pool;
    auto conv = [&](int co, int ci, int k) {
        fill((size_t)co * ci * k * k, 0, ci * k * k);
        if (d.conv_bias) fill(co, 1, ci * k * k);
        fill(co, 2, 1); fill(co, 3, 1); fill(co, 4, 1); fill(co, 5, 1);
    };
    conv(F, d.in_planes, 3);
    for (int i = 0; i < d.blocks; ++i) { conv(F, F, 3); conv(F, F, 3); }
    conv(HC, F, 1);
    fill((size_t)d.action_size * HC * PP, 0, HC * PP); fill(d.action_size, 1, HC * PP);
    conv(HC, F, 1);
    fill((size_t)d.fc_hidden * HC * PP, 0, HC * PP); fill(d.fc_hidden, 1, HC * PP);
    fill(d.fc_hidden, 0, d.fc_hidden); fill(1, 1, d.fc_hidden);
    if (off != n->nparams) return az_fail(AZ_ERR_STATE, "init size mismatch");
    return az_net_load_weights(n, blob.data(), blob.size());
}

}  // extern "C"
