// net_host.hip -- the device network behind the az_net_* entry points of include/az_engine.h:
// creation (buffers, shape and precision checks), the forward dispatched on the net's plan
// (net_plan.h), profiling.  The weights are loaded by net_load.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/az_engine.h"
#include "engine_internal.h"
#include "net.h"
#include "net_host.h"
#include "tree.h"

namespace {

NetPlan plan_of(const az_net* n) {
    return net_plan(net_shape(n->d, n->rw), n->d.precision, az_conv_flags(), az_device_lds_limit());
}

GemmArgs gemm_args(const Layer& L, const float* A, int lda, float* C, int ldc, const float* res, int M, int H, int W,
                   const int* m_limit, int rows_per_sample) {
    GemmArgs p{};
    p.A = A; p.lda = lda; p.B = L.W; p.ldb = L.K; p.C = C; p.ldc = ldc; p.bias = L.b; p.res = res;
    p.M = M; p.N = L.N; p.K = L.K; p.Kpad = L.Kpad; p.taps = L.taps; p.Cch = L.C; p.H = H; p.W = W;
    p.m_limit = m_limit; p.rows_per_sample = rows_per_sample;
    return p;
}

// What every 3x3 conv of a forward of B boards shares (C input channels, the net's channels out, ReLU,
// the zeroed tail behind the full capacity); the caller states operands, outputs and residuals.
ConvBf16Args conv_args(const az_net* n, int B, const int* nb, int C) {
    ConvBf16Args a{};
    a.M = B * n->HW; a.N = n->d.channels; a.C = C; a.H = n->d.board_size; a.W = n->d.board_size;
    a.m_limit = nb; a.rows_per_sample = n->HW; a.relu = 1;
    a.a_tail = n->act_elems * 2;
    a.zero = n->zero; a.ovf = n->ovf;
    a.stamp = -1;
    return a;
}

// K slices for an FC layer of B rows: enough blocks to cover the chip (a 128 x 128 f32 tile is
// bound by the CU's f32 MFMA rate), slices of >= 64 K
constexpr int FC_MAX_SPLITS = 64;
int fc_splits(int B, int K) {
    const int tiles = (B + 127) / 128 * 2;
    int s = 1;
    while (s < FC_MAX_SPLITS && tiles * s < 512 && K / (2 * s) >= 64) s *= 2;
    return s;
}

}  // namespace

int net_input_path(const az_net* n) { return plan_of(n).input; }

namespace {

// Router of a rand-wire node: relu(BN(conv1x1(concat(ins)))) as ONE GEMM over K = deg F whose
// k-slice j is read straight from input j's buffer (the device table `dins`, same k order as the
// reference's torch::cat); BN folded into the weights and bias.
void rw_router(const az_net* n, int trunk, const Layer& L, const float* const* dins, float* out, int rows, const int* nb,
               hipStream_t st) {
    const int F = n->d.channels, H = n->d.board_size;
    GemmArgs p{};
    p.Am = dins; p.lda = F; p.B = L.W; p.ldb = L.K; p.C = out; p.ldc = F; p.bias = L.b;
    p.M = rows; p.N = F; p.K = L.K; p.Kpad = L.Kpad; p.taps = 1; p.Cch = F; p.H = H; p.W = H;
    p.m_limit = nb; p.rows_per_sample = n->HW;
    if (trunk == NET_TRUNK_RW_V4_FP16) az_launch_gemm_h16_relu(p, st);   // fp16 operands, fp32 accumulation
    else az_launch_gemm_f32(p, ACT_RELU, false, st);
}

// DDW-RandWire trunk (ddw_randwire_resnet.cpp:321-384 per block): input nodes on the block input,
// the others in topological order on their router's output (or their single predecessor's
// output), the block output (output router or the single sink) into the h0 / h1 ping-pong.
float* trunk_rw(az_net* n, int trunk, int B, const int* nb, hipStream_t st) {
    const az_net_desc& d = n->d;
    const int F = d.channels, H = d.board_size, HW = n->HW, rows = B * HW, R = F / 16;
    float* x = n->h0;
    bool conv_err = false;
    for (const RwBlock& blk : n->rwb) {
        const azrw::Plan& pl = blk.plan;
        auto node = [&](int v, const float* in) {
            const RwNode& nd = blk.node[v];
            if (trunk == NET_TRUNK_RW_F32) {
                GemmArgs g1 = gemm_args(nd.c1, in, F, n->t, F, nullptr, rows, H, H, nb, HW);
                GemmArgs g2 = gemm_args(nd.c2, n->t, F, n->rw_t2, F, nullptr, rows, H, H, nb, HW);
                if (n->rw_ws) { g1.part = g2.part = n->rw_ws; g1.splits = g2.splits = n->rw_splits; }
                az_launch_gemm_f32(g1, ACT_RELU, false, st);
                az_launch_gemm_f32(g2, ACT_NONE, false, st);
            } else {
                // conv3x3_v4: conv1 -> 16-bit t, conv2 -> fp32 y; the residual stream, routers and SE stay
                // fp32.  fp16 operands (mode 2), or fp32-faithful: operands split into bf16 hi + lo, three
                // MFMAs per product (mode 0); fp32 accumulation in both
                const bool x3 = trunk == NET_TRUNK_RW_V4_X3;
                if (x3) az_launch_split_bf16(in, n->hh[0], n->hl[0], (size_t)rows * F, nb, HW, F, st);
                else az_launch_to_f16(in, n->hh[0], (size_t)rows * F, nb, HW, F, st, n->ovf);
                ConvBf16Args a = conv_args(n, B, nb, F);
                a.Ahi = n->hh[0]; a.Chi = n->th; a.bias = nd.c1.b;
                ConvBf16Args c = a;
                c.Ahi = n->th; c.Chi = n->hh[1]; c.Cf = n->rw_t2; c.bias = nd.c2.b; c.relu = 0;
                if (x3) {
                    a.Alo = n->hl[0]; a.Bhi = nd.c1.Whi; a.Blo = nd.c1.Wlo; a.Bblk = nd.c1.Wbk_bf; a.Clo = n->tl;
                    c.Alo = n->tl; c.Bhi = nd.c2.Whi; c.Blo = nd.c2.Wlo; c.Bblk = nd.c2.Wbk_bf; c.Clo = n->hl[1];
                } else {
                    a.Bhi = nd.c1.Wh16; a.Bblk = nd.c1.Wbk_h;
                    c.Bhi = nd.c2.Wh16; c.Bblk = nd.c2.Wbk_h;
                }
                if (az_conv_nhwc16_launch(a, x3 ? 0 : 2, st) || az_conv_nhwc16_launch(c, x3 ? 0 : 2, st)) conv_err = true;
            }
            az_launch_se_residual(n->rw_t2, in, n->rw_out[v], nd.w1, nd.b1, nd.w2, nd.b2, B, HW, F, R, nb, st);
        };
        for (int v : pl.inputs) node(v, x);
        for (int v : pl.topo) {
            const auto& pr = pl.preds[v];
            if (pr.empty() || std::find(pl.inputs.begin(), pl.inputs.end(), v) != pl.inputs.end()) continue;
            if (pr.size() == 1) { node(v, n->rw_out[pr[0]]); continue; }
            rw_router(n, trunk, blk.node[v].router, blk.node[v].ins, n->rw_in, rows, nb, st);
            node(v, n->rw_in);
        }
        float* y = x == n->h0 ? n->h1 : n->h0;
        if (pl.outputs.size() > 1) {
            rw_router(n, trunk, blk.out_router, blk.outs, y, rows, nb, st);
        } else {
            (void)hipMemcpyAsync(y, n->rw_out[pl.outputs[0]], (size_t)rows * F * 4, hipMemcpyDeviceToDevice, st);
        }
        x = y;
    }
    return conv_err ? nullptr : x;
}

// Diagnostic (az_diag_set_poison): with a byte value >= 0, every activation / workspace buffer of a
// net (not the zeroed tails, not the weights) is filled with that byte before each forward, so a
// kernel that reads memory its forward never wrote gives a result that depends on the byte
// (0xff: NaN in every float format) -- the tests compare forwards under two poisons bitwise
int g_poison = -1;
int poison_net(az_net* n, hipStream_t st, bool inputs) {
    if (g_poison < 0) return 0;
    for (const DevPool::Buf& b : n->acts.bufs) {
        const bool in = b.p == (void*)n->x0 || b.p == (void*)n->in_nchw;
        if (in == inputs) HIPCHK(hipMemsetAsync(b.p, g_poison, b.bytes, st));
    }
    return 0;
}

// The FC layers of both heads from the head feature maps pp / vp ([B][P*P][HC]; cell stride xs,
// default HC: pp / vp may be the two halves of the combined head-conv output).
int net_heads_fc(az_net* n, const NetPlan& pl, int B, const int* nb, float* logits, float* value, hipStream_t st,
                 const float* pp = nullptr, const float* vp = nullptr, int xs = 0) {
    const az_net_desc& d = n->d;
    const int HK = d.head_channels * n->P2;
    if (!pp) { pp = n->pp; vp = n->vp; xs = d.head_channels; }
    // Both FC heads: k_fc_heads (split-K partials of both FCs in one GEMM) + k_fc_finish (per board)
    if (pl.heads != NET_HEADS_GENERIC) {
        FcHeadArgs fa{};
        fa.pp = pp; fa.vp = vp; fa.hc = d.head_channels; fa.xs = xs;
        fa.Wp = n->pfc.W; fa.bp = n->pfc.b; fa.Wv1 = n->vfc1.W; fa.bv1 = n->vfc1.b; fa.wv2 = n->vfc2.W; fa.bv2 = n->vfc2.b;
        fa.logits = logits; fa.hid = n->v1; fa.value = value;
        fa.part = n->ws; fa.m_limit = nb;
        fa.B = B; fa.K = HK; fa.A = d.action_size; fa.H = d.fc_hidden;
        fa.S = az_fc_heads_splits(d.max_batch, HK, d.action_size, d.fc_hidden);   // from the capacity: batch-size independent
        // the split-operand products (k_fc_heads_x3) where the plan takes them
        if (pl.heads == NET_HEADS_X3_BF16) { fa.Wx_hi = n->fcx_hi; fa.Wx_lo = n->fcx_lo; fa.pt = 1; }
        if (pl.heads == NET_HEADS_X3_FP16) { fa.Wx_hi = n->fcf_hi; fa.Wx_lo = n->fcf_lo; fa.pt = 2; fa.rs = n->fcf_rs; fa.ovf = n->ovf; }
        if (fa.pt) fa.S = az_fc_heads_splits_x3(d.max_batch, HK, d.action_size, d.fc_hidden);
        az_launch_fc_heads(fa, st);
        HIPCHK(hipGetLastError());
        return 0;
    }
    // generic shapes: split-K partials (deterministic reductions); the value head's FC1 partials
    // are reduced, ReLU'd and dotted with FC2 by one kernel per board
    if (xs != d.head_channels) return az_fail(AZ_ERR_ARG, "net_heads_fc: strided head maps need k_fc_heads");
    GemmArgs pf = gemm_args(n->pfc, n->pp, HK, logits, d.action_size, nullptr, B, 1, 1, nb, 1);
    GemmArgs v1 = gemm_args(n->vfc1, n->vp, HK, n->v1, d.fc_hidden, nullptr, B, 1, 1, nb, 1);
    const int splits = fc_splits(d.max_batch, HK);
    pf.part = n->ws; pf.splits = splits;
    v1.part = n->ws + (size_t)B * d.action_size * splits; v1.splits = splits;
    if (splits > 1) az_launch_gemm_f32(pf, ACT_NONE, false, st);
    else { pf.part = nullptr; az_launch_gemm_f32(pf, ACT_NONE, false, st); }
    az_launch_gemm_f32_partials(v1, st);
    az_launch_value_head(v1.part, splits, n->vfc1.b, n->vfc2.W, n->vfc2.b, n->v1, value, B, d.fc_hidden, nb, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// Profiling: counts the forward (in trunk-conv equivalents: bench.py's per-conv rate) and, on a
// sampled one, stamps the trunk's start; true when the closing stamp is due behind the trunk.
bool prof_open(az_net* n, hipStream_t st) {
    if (!n->prof || n->d.blocks < 1) return false;
    n->prof_launches += 2 * n->d.blocks;
    n->prof_forwards += 1;
    if (n->prof_tick++ % prof_every() != 0 || !n->pc.room(2)) return false;
    n->prof_sampled += 1;
    n->pc.stamp(st);
    return true;
}

// NET_TRUNK_SMALL: input conv, trunk, pool and the two head 1x1 convs in one launch (smallnet.hip)
int forward_small(az_net* n, const NetPlan& pl, const float* x0, int B, const int* nb, float* logits, float* value,
                  hipStream_t st, const LeafRecs* lr) {
    const az_net_desc& d = n->d;
    const bool sampled = prof_open(n, st);
    SmallNetArgs sa{};
    sa.x0 = x0; sa.m_limit = nb; sa.ovf = n->ovf;
    if (lr) {
        if (lr->go) return az_fail(AZ_ERR_ARG, "smallnet: Gomoku leaf records only");
        sa.x0 = nullptr; sa.rec = lr->rec; sa.gidx = lr->gidx; sa.rec_n = lr->n; sa.rec_identity = lr->identity;
    }
    sa.W = n->sm_W; sa.Wf = n->sm_Wf; sa.bias = n->sm_b;
    if (d.precision == AZ_PREC_BF16X3) { sa.Wxh = n->sm_Wxh; sa.Wxl = n->sm_Wxl; sa.pt = 1; }   // k_smallnet_x3
    if (d.precision == AZ_PREC_F16X3) {
        sa.Wxh = n->sm_Wfh; sa.Wxl = n->sm_Wfl; sa.pt = 2; sa.bias = n->sm_bx; sa.osc = n->sm_sx;
    }
    sa.Wpc = n->pconv.W; sa.bpc = n->pconv.b; sa.Wvc = n->vconv.W; sa.bvc = n->vconv.b;
    sa.pp = n->pp; sa.vp = n->vp;
    sa.H = d.board_size; sa.blocks = d.blocks; sa.residual = d.residual; sa.HC = d.head_channels; sa.P = d.pool;
    sa.stamps = az_smallnet_stamps_mode();   // diagnostic phase stamps (az_diag_set_smallnet_stamps)
    if (az_smallnet_launch(sa, B, st)) return az_fail(AZ_ERR_ARG, "smallnet: unsupported shape");
    if (sampled) n->pc.stamp(st);
    return net_heads_fc(n, pl, B, nb, logits, value, st);
}

// The int8 remainder planes of the g8 trunk live in the (otherwise idle) lo buffers
int8_t* g8_q(const az_net* n, int i) { return reinterpret_cast<int8_t*>(n->hl[i]); }

// NET_IN_G8: input planes -> g8 16-bit in th (0/1 planes are exact), then the input conv on the g8
// kernel into hh[0]; plan.in32: the planes as 32 channels (groups 2-3 zero) for the zero-padded layer
int input_g8(az_net* n, const NetPlan& pl, const float* x0, int B, const int* nb, hipStream_t st, const LeafRecs* lr) {
    const bool f16 = n->d.precision == AZ_PREC_FP16;
    const int mode = f16 ? 2 : 1, H = n->d.board_size;
    const Layer& IN = pl.in32 ? n->in32 : n->in;
    const int cin = pl.in32 ? 32 : n->cin_pad;
    if (lr) {
        if (n->cin_pad != 16) return az_fail(AZ_ERR_ARG, "leaf records carry 16 planes");
        az_launch_rec_to_g8(lr->rec, lr->gidx, n->th, lr->go, H, nb, B, mode, st, cin / 8);
    } else {
        az_launch_to_g8(x0, n->th, nullptr, n->cin_pad, n->HW, nb, B, mode, st, cin);
    }
    ConvBf16Args a = conv_args(n, B, nb, cin);
    a.Ahi = n->th; a.Bblk = f16 ? IN.Wbk_h : IN.Wbk_bf; a.bias = IN.b;
    a.Chi = n->hh[0]; a.Cq = g8_q(n, 0);
    if (az_conv_g8_launch(a, mode, st)) return az_fail(AZ_ERR_ARG, "g8 input conv: unsupported shape");
    return 0;
}

// NET_TRUNK_GEMM_F32: the fp32 NHWC stream from h0; returns the trunk's output
float* trunk_gemm_f32(az_net* n, int B, const int* nb, hipStream_t st) {
    const az_net_desc& d = n->d;
    const int H = d.board_size, F = d.channels, HW = n->HW, rows = B * HW;
    float *h = n->h0, *other = n->h1;
    for (int i = 0; i < d.blocks; ++i) {
        az_launch_gemm_f32(gemm_args(n->blk[2 * i], h, F, n->t, F, nullptr, rows, H, H, nb, HW), ACT_RELU, false, st);
        az_launch_gemm_f32(gemm_args(n->blk[2 * i + 1], n->t, F, other, F, d.residual ? h : nullptr, rows, H, H, nb, HW),
                           ACT_RELU, d.residual != 0, st);
        std::swap(h, other);
    }
    return h;
}

// NET_TRUNK_G8X3, the fp32-faithful trunk: every activation as g8 hi + lo planes (bf16 or fp16
// pieces), three MFMAs per product (conv3x3_v9x3 / v7x3).  From the fp32 h0 to the planes hh / hl[*cur].
int trunk_g8x3(az_net* n, int B, const int* nb, hipStream_t st, int* cur) {
    const az_net_desc& d = n->d;
    const int F = d.channels, pt = d.precision == AZ_PREC_F16X3 ? 2 : 1;
    az_launch_to_g8x3(n->h0, n->hh[0], n->hl[0], F, n->HW, nb, B, st, pt, n->ovf);
    int c = 0;
    for (int i = 0; i < 2 * d.blocks; ++i) {
        const Layer& L = n->blk[i];
        const bool second = i & 1;
        ConvBf16Args a = conv_args(n, B, nb, F);
        a.Ahi = second ? n->th : n->hh[c]; a.Alo = second ? n->tl : n->hl[c];
        a.Bblk = L.Wbk_bf; a.Bblk_lo = L.Wbk_lo; a.bias = L.b; a.pt = pt;
        if (pt == 2) { a.Bblk = L.Wbk_fh; a.Bblk_lo = L.Wbk_fl; a.oscale = L.sx; a.bias = L.bx; }
        a.Chi = second ? n->hh[c ^ 1] : n->th; a.Clo = second ? n->hl[c ^ 1] : n->tl;
        if (second && d.residual) { a.Rhi = n->hh[c]; a.Rlo = n->hl[c]; }
        a.stamp = i;
        if (az_conv_v7x3_launch(a, st)) return az_fail(AZ_ERR_ARG, "bf16x3 trunk conv: unsupported shape");
        if (second) c ^= 1;
    }
    *cur = c;
    return 0;
}

// NET_TRUNK_G8: 16-bit g8 planes with int8 remainders (conv3x3_v5 / v6 / v7 by the launch), from
// the input conv's hh[0] to the planes hh[*cur] / g8_q(*cur)
int trunk_g8(az_net* n, int B, const int* nb, hipStream_t st, int* cur) {
    const az_net_desc& d = n->d;
    const bool f16 = d.precision == AZ_PREC_FP16;
    int c = 0;
    for (int i = 0; i < 2 * d.blocks; ++i) {
        const Layer& L = n->blk[i];
        const bool second = i & 1;
        ConvBf16Args a = conv_args(n, B, nb, d.channels);
        a.Ahi = second ? n->th : n->hh[c];
        a.Bblk = f16 ? L.Wbk_h : L.Wbk_bf; a.bias = L.b;
        a.Chi = second ? n->hh[c ^ 1] : n->th;
        if (second) a.Cq = g8_q(n, c ^ 1);
        if (second && d.residual) { a.Rhi = n->hh[c]; a.Rq = g8_q(n, c); }
        a.stamp = i;
        if (az_conv_g8_launch(a, f16 ? 2 : 1, st)) return az_fail(AZ_ERR_ARG, "g8 trunk conv: unsupported shape");
        if (second) c ^= 1;
    }
    *cur = c;
    return 0;
}

// NET_TRUNK_NHWC16: 16-bit NHWC operands from the fp32 h0 -- bf16 (conv3x3_v4 / v3 / conv3x3_bf16),
// bf16 hi + lo (AZ_PREC_BF16X3 off the g8 boards) or fp16 (conv3x3_v4) with the fp32 residual
// stream; returns the trunk's fp32 output
float* trunk_nhwc16(az_net* n, int B, const int* nb, hipStream_t st) {
    const az_net_desc& d = n->d;
    const int F = d.channels, HW = n->HW, rows = B * HW;
    const bool f16 = d.precision == AZ_PREC_FP16, split = d.precision == AZ_PREC_BF16X3;
    float *h = n->h0, *other = n->h1;
    if (f16) az_launch_to_f16(h, n->hh[0], (size_t)rows * F, nb, HW, F, st, n->ovf);
    else az_launch_split_bf16(h, n->hh[0], split ? n->hl[0] : nullptr, (size_t)rows * F, nb, HW, F, st);
    int cur = 0;
    for (int i = 0; i < d.blocks; ++i) {
        const Layer& L1 = n->blk[2 * i];
        const Layer& L2 = n->blk[2 * i + 1];
        ConvBf16Args a = conv_args(n, B, nb, F);
        a.Ahi = n->hh[cur]; a.Bhi = f16 ? L1.Wh16 : L1.Whi; a.Bblk = f16 ? L1.Wbk_h : L1.Wbk_bf;
        a.Chi = n->th; a.bias = L1.b;
        if (split) { a.Alo = n->hl[cur]; a.Blo = L1.Wlo; a.Clo = n->tl; }
        a.stamp = 2 * i;
        ConvBf16Args b2 = a;
        b2.Ahi = n->th; b2.Bhi = f16 ? L2.Wh16 : L2.Whi; b2.Bblk = f16 ? L2.Wbk_h : L2.Wbk_bf;
        b2.Chi = n->hh[cur ^ 1]; b2.bias = L2.b;
        if (split) { b2.Alo = n->tl; b2.Blo = L2.Wlo; b2.Clo = n->hl[cur ^ 1]; }
        b2.stamp = 2 * i + 1;
        if (f16) {
            // fp16 conv operands, fp32 residual stream (an fp16 stream doubles the logit error)
            b2.Rf = d.residual ? h : nullptr;
            b2.Cf = other;
            if (az_conv_nhwc16_launch(a, 2, st) || az_conv_nhwc16_launch(b2, 2, st)) return nullptr;
            std::swap(h, other);
        } else {
            if (d.residual) { b2.Rhi = n->hh[cur]; b2.Rlo = split ? n->hl[cur] : nullptr; }
            b2.Cf = (i == d.blocks - 1) ? other : nullptr;
            if (az_conv_nhwc16_launch(a, split ? 0 : 1, st) || az_conv_nhwc16_launch(b2, split ? 0 : 1, st)) return nullptr;
        }
        cur ^= 1;
    }
    return d.blocks > 0 && !f16 ? other : h;
}

}  // namespace

// Forward of B samples (B = capacity; *nb = active samples, device side) from the
// NHWC16 input x0 -> logits [B][A], value [B].  lr (optional; only where
// net_input_path != NET_IN_GEMM): the planes come from leaf records instead of x0.
// Three stages on the net's plan: the input stage, one function per trunk family, the tail.
int net_forward(az_net* n, const float* x0, int B, const int* nb, float* logits, float* value, hipStream_t st,
                const LeafRecs* lr) {
    const az_net_desc& d = n->d;
    const int H = d.board_size, HW = n->HW, F = d.channels, P = d.pool, PP = n->P2, HC = d.head_channels;
    const NetPlan pl = plan_of(n);
    if (lr && pl.input == NET_IN_GEMM) return az_fail(AZ_ERR_ARG, "net_forward: this net cannot read leaf records");
    if (int r = poison_net(n, st, false)) return r;
    if (pl.no_forward) return az_fail(AZ_ERR_ARG, "%s", pl.no_forward);
    if (pl.trunk == NET_TRUNK_SMALL) return forward_small(n, pl, x0, B, nb, logits, value, st, lr);

    if (pl.input == NET_IN_G8) {
        if (int r = input_g8(n, pl, x0, B, nb, st, lr)) return r;
    } else {
        az_launch_gemm_f32(gemm_args(n->in, x0, n->cin_pad, n->h0, F, nullptr, B * HW, H, H, nb, HW), ACT_RELU, false, st);
    }

    const bool sampled = prof_open(n, st);
    const bool g8 = pl.trunk == NET_TRUNK_G8 || pl.trunk == NET_TRUNK_G8X3;
    float* h = nullptr;   // the trunk's output: fp32 NHWC, or on the g8 families the planes hh / hl[cur]
    int cur = 0, r = 0;
    switch (pl.trunk) {
        case NET_TRUNK_G8: r = trunk_g8(n, B, nb, st, &cur); break;
        case NET_TRUNK_G8X3: r = trunk_g8x3(n, B, nb, st, &cur); break;
        case NET_TRUNK_NHWC16: h = trunk_nhwc16(n, B, nb, st); break;
        case NET_TRUNK_GEMM_F32: h = trunk_gemm_f32(n, B, nb, st); break;
        default: h = trunk_rw(n, pl.trunk, B, nb, st); break;
    }
    if (r) return r;
    if (!g8 && !h) return az_fail(AZ_ERR_ARG, "trunk conv: unsupported shape");
    if (sampled) n->pc.stamp(st);

    // the tail -- pool and both head 1x1 convs: one launch on the g8 paths (k_pool_heads_g8, bitwise
    // what k_pool_g8 + gemm_f32 give)
    if (g8) {
        // k_pool_g8 modes: 1 bf16 / 2 fp16 planes + int8 remainders, 0 bf16 / 3 fp16 hi + lo planes
        const int mode = pl.trunk == NET_TRUNK_G8 ? (d.precision == AZ_PREC_FP16 ? 2 : 1) : (d.precision == AZ_PREC_F16X3 ? 3 : 0);
        if (!pl.tail_fused) az_launch_pool_g8(n->hh[cur], g8_q(n, cur), n->pool, B, F, H, P, nb, mode, st);
        else if (az_launch_pool_heads_g8(n->hh[cur], g8_q(n, cur), n->hconv.W, n->hconv.b, n->hpv, B, F, H, P, 2 * HC, nb, mode, st))
            return az_fail(AZ_ERR_HIP, "k_pool_heads_g8 launch failed");
    } else {
        az_launch_pool(h, n->pool, B, H, H, F, P, nb, st);
    }
    if (pl.head_conv_fused)
        // both head 1x1 convs as one GEMM (2 HC outputs; every output is the same k-ordered fp32
        // chain as in two launches), read by the FC heads with a 2 HC cell stride
        az_launch_gemm_f32(gemm_args(n->hconv, n->pool, F, n->hpv, 2 * HC, nullptr, B * PP, 1, 1, nb, PP), ACT_RELU, false, st);
    if (pl.tail_fused || pl.head_conv_fused) return net_heads_fc(n, pl, B, nb, logits, value, st, n->hpv, n->hpv + HC, 2 * HC);
    az_launch_gemm_f32(gemm_args(n->pconv, n->pool, F, n->pp, HC, nullptr, B * PP, 1, 1, nb, PP), ACT_RELU, false, st);
    az_launch_gemm_f32(gemm_args(n->vconv, n->pool, F, n->vp, HC, nullptr, B * PP, 1, 1, nb, PP), ACT_RELU, false, st);
    return net_heads_fc(n, pl, B, nb, logits, value, st);
}

// The fp16 range guard's flag of a net (sticky on the device until read here): AZ_ERR_RANGE once set.
int check_ovf(az_net* n, int ovf) {
    if (!ovf) return 0;
    HIPCHK(hipMemsetAsync(n->ovf, 0, 4, n->e->stream));
    HIPCHK(hipStreamSynchronize(n->e->stream));
    return az_fail(AZ_ERR_RANGE, "fp16 activation overflow (|x| > 65504) in the network forward: its outputs are invalid; "
                                 "use AZ_PREC_BF16X3 for nets with activations of this magnitude");
}

// What az_net_create* / az_net_set_precision answer for a precision on this description: the plan's refusal
static int check_precision(const az_net_desc& d, bool rw, int precision) {
    const NetPlan pl = net_plan(net_shape(d, rw), precision, 0, 0);
    return pl.status ? az_fail(pl.status, "%s", pl.message) : 0;
}

static int net_create(az_engine* e, const az_net_desc* d, az_net** out, bool rw,
                      const std::vector<azrw::Plan>* plans = nullptr) {
    if (!e || !d || !out) return az_fail(AZ_ERR_ARG, "null argument");
    if (d->board_size < 2 || d->board_size * d->board_size > AZ_MAXA || d->in_planes < 1 || d->in_planes > 128 ||
        d->channels < 4 || d->channels % 4 || d->blocks < 0 || d->action_size < 1 || d->action_size > 8192 ||
        d->head_channels < 1 || d->head_channels % 4 || d->pool < 1 || d->fc_hidden < 1 || d->fc_hidden % 4 ||
        d->max_batch < 1)
        return az_fail(AZ_ERR_ARG, "unsupported network description");
    if (int r = check_precision(*d, rw, d->precision)) return r;
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device));
    auto* n = new az_net();
    n->e = e;
    n->d = *d;
    n->HW = d->board_size * d->board_size;
    n->P2 = d->pool * d->pool;
    n->cin_pad = net_shape(*d, rw).cin_pad;
    n->rw = rw;
    if (rw) {
        n->rwb.resize(d->blocks);
        for (int i = 0; i < d->blocks; ++i) {
            n->rwb[i].plan = plans ? (*plans)[i] : azrw::plan(i);
            n->rwb[i].node.resize(n->rwb[i].plan.preds.size());
        }
    }
    n->nparams = net_blob_params(n);
    const size_t B = d->max_batch, rows = B * n->HW, F = d->channels;
    n->act_elems = rows * F;
    int r = 0;
    auto A_ = [&](float** p, size_t cnt) { if (!r) r = n->acts.alloc(p, cnt); };
    // 16-bit activation planes carry a zeroed tail (AZ_ACT_TAIL elements): the v6 conv points the
    // DMA of halo padding rows there
    auto H_ = [&](uint16_t** p, size_t cnt) {
        if (r) return;
        r = n->acts.alloc(p, cnt, AZ_ACT_TAIL);
        if (!r && hipMemset(*p + cnt, 0, AZ_ACT_TAIL * 2) != hipSuccess) r = az_fail(AZ_ERR_HIP, "hipMemset");
    };
    A_(&n->x0, rows * n->cin_pad);
    A_(&n->h0, rows * F); A_(&n->h1, rows * F); A_(&n->t, rows * F);
    if (F % 32 == 0) {
        H_(&n->hh[0], rows * F); H_(&n->hh[1], rows * F); H_(&n->hl[0], rows * F); H_(&n->hl[1], rows * F);
        H_(&n->th, rows * F); H_(&n->tl, rows * F);
    }
    A_(&n->pool, B * n->P2 * F);
    A_(&n->pp, B * n->P2 * d->head_channels); A_(&n->vp, B * n->P2 * d->head_channels);
    A_(&n->hpv, B * n->P2 * 2 * d->head_channels);
    A_(&n->v1, B * d->fc_hidden);
    {   // split-K workspace: gemm_f32 partials, or k_fc_heads' [<= 16 slices][B padded to 64][64-column tiles]
        const size_t nc = (size_t)((d->action_size + 63) / 64 + (d->fc_hidden + 63) / 64) * 64;
        A_(&n->ws, std::max((size_t)B * (d->action_size + d->fc_hidden) * FC_MAX_SPLITS, 16 * ((size_t)B + 63) / 64 * 64 * nc));
    }
    A_(&n->logits, B * d->action_size); A_(&n->value, B); A_(&n->soft, B * d->action_size);
    A_(&n->in_nchw, B * d->in_planes * n->HW);
    if (rw) {
        size_t nodes = 0;
        for (const RwBlock& blk : n->rwb) nodes = std::max(nodes, blk.node.size());
        n->rw_out.assign(nodes, nullptr);
        for (float*& p : n->rw_out) A_(&p, rows * F);
        A_(&n->rw_t2, rows * F); A_(&n->rw_in, rows * F);
        // Small capacities leave most CUs idle (one 128 x 128 f32 tile of a K = 9F conv is ~60 us
        // of one CU): split K so the node convs cover the chip.  Chosen from max_batch, so a
        // board's summation order never depends on the batch it arrives in.
        {
            const int bn = F <= 64 ? 64 : 128, nk = (int)((9 * F + 31) / 32);
            const long tiles = (long)((rows + 127) / 128) * (long)((F + bn - 1) / bn);
            while (n->rw_splits < 8 && tiles * n->rw_splits < 256 && nk / (2 * n->rw_splits) >= 4) n->rw_splits *= 2;
            if (n->rw_splits > 1) A_(&n->rw_ws, (size_t)n->rw_splits * rows * F);
        }
        // routers read their inputs straight from the node buffers: per router a device table
        auto table = [&](const std::vector<int>& ids, const float*** dst) {
            if (r || ids.size() < 2) return;
            std::vector<const float*> t;
            for (int u : ids) t.push_back(n->rw_out[u]);
            if (n->misc.alloc(dst, t.size()) ||
                hipMemcpy((void*)*dst, t.data(), t.size() * sizeof(float*), hipMemcpyHostToDevice) != hipSuccess)
                r = az_fail(AZ_ERR_OOM, "router input table");
        };
        for (RwBlock& blk : n->rwb) {
            for (size_t v = 0; v < blk.node.size(); ++v) table(blk.plan.preds[v], &blk.node[v].ins);
            table(blk.plan.outputs, &blk.outs);
        }
    }
    if (!r) r = n->misc.alloc(&n->d_nb, 1);
    if (!r) r = n->misc.alloc(&n->ovf, 1);
    if (!r && hipMemset(n->ovf, 0, 4) != hipSuccess) r = az_fail(AZ_ERR_HIP, "memset");
    if (!r) r = n->misc.alloc(&n->zero, 128);
    if (!r && hipMemset(n->zero, 0, 256) != hipSuccess) r = az_fail(AZ_ERR_HIP, "memset");
    // the memsets above run on the null stream, the forwards on the engine's non-blocking stream,
    // which does not wait for it: finish them here
    if (!r && hipDeviceSynchronize() != hipSuccess) r = az_fail(AZ_ERR_HIP, "hipDeviceSynchronize");
    if (r) { az_net_destroy(n); return r; }
    *out = n;
    return 0;
}


// Every rand-wire create path: the precision, then the shapes the node kernels assume
// (k_se_residual: C % 16 == 0 for its float4 channel quads, C <= 1024 and R = C / 16 <= 64 for
// its fixed LDS arrays; no conv bias; the reference's adaptive pool to min(8, board)).
static int check_rw_desc(const az_net_desc& d) {
    if (int r = check_precision(d, true, d.precision)) return r;
    if (d.conv_bias) return az_fail(AZ_ERR_ARG, "rand-wire convolutions carry no bias (conv_bias = 0)");
    if (d.channels < 16 || d.channels % 16 || d.channels > 1024)
        return az_fail(AZ_ERR_ARG, "rand-wire channels: a multiple of 16 in [16, 1024]");
    if (d.pool != std::min(8, d.board_size)) return az_fail(AZ_ERR_ARG, "rand-wire heads pool to min(8, board)");
    return 0;
}

static int net_host_forward(az_net* n, const float* planes, int B, float* logits, float* value, bool soft) {
    if (!n || !planes || B < 1 || B > n->d.max_batch) return az_fail(AZ_ERR_ARG, "bad batch (1..%d)", n ? n->d.max_batch : 0);
    if (!n->loaded) return az_fail(AZ_ERR_STATE, "weights not loaded");
    std::lock_guard<std::mutex> lk(n->mu);
    HIPCHK(hipSetDevice(n->e->device));
    hipStream_t st = n->e->stream;
    const int A = n->d.action_size;
    if (int r = poison_net(n, st, true)) return r;
    HIPCHK(hipMemcpyAsync(n->in_nchw, planes, (size_t)B * n->d.in_planes * n->HW * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(n->d_nb, &B, 4, hipMemcpyHostToDevice, st));
    az_launch_pack_input(n->in_nchw, n->x0, B, n->d.in_planes, n->HW, n->cin_pad, st);
    if (int r = net_forward(n, n->x0, B, n->d_nb, n->logits, n->value, st)) return r;
    const float* pol = n->logits;
    if (soft) { az_launch_softmax_rows(n->logits, n->soft, B, A, st); pol = n->soft; }
    HIPCHK(hipGetLastError());
    if (logits) HIPCHK(hipMemcpyAsync(logits, pol, (size_t)B * A * 4, hipMemcpyDeviceToHost, st));
    if (value) HIPCHK(hipMemcpyAsync(value, n->value, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    int ovf = 0;
    HIPCHK(hipMemcpyAsync(&ovf, n->ovf, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return check_ovf(n, ovf);
}

extern "C" {

int az_diag_set_poison(int byte) { g_poison = byte < 0 ? -1 : (byte & 0xff); return 0; }

int az_net_create(az_engine* e, const az_net_desc* d, az_net** out) { return net_create(e, d, out, false); }

int az_net_create_randwire(az_engine* e, const az_net_desc* d, az_net** out) {
    if (!d) return az_fail(AZ_ERR_ARG, "null argument");
    if (int r = check_rw_desc(*d)) return r;
    return net_create(e, d, out, true);
}

// Explicit wiring (e.g. the Python DDWRandWireResNet's networkx graphs, python/alphazero/models/
// ddw_randwire.py:56-116): per block  n, order[n], then for node v = 0..n-1: deg_v, preds[deg_v],
// then n_out, outputs[n_out].  Inputs are the in-degree-0 nodes in `order`; the compute order is
// any topological order (a node's output depends only on its inputs).
int az_net_create_randwire_graphs(az_engine* e, const az_net_desc* d, const int* g, size_t n_ints, az_net** out) {
    if (!d || !g) return az_fail(AZ_ERR_ARG, "null argument");
    if (int r = check_rw_desc(*d)) return r;
    std::vector<azrw::Plan> plans(std::max(0, d->blocks));
    size_t k = 0;
    auto next = [&](int& v) { if (k >= n_ints) return false; v = g[k++]; return true; };
    for (int b = 0; b < d->blocks; ++b) {
        azrw::Plan& pl = plans[b];
        int n = 0;
        if (!next(n) || n < 1 || n > 1024) return az_fail(AZ_ERR_ARG, "block %d: bad node count", b);
        pl.order.resize(n);
        std::vector<char> seen(n, 0);
        for (int& v : pl.order) {
            if (!next(v) || v < 0 || v >= n || seen[v]) return az_fail(AZ_ERR_ARG, "block %d: order is not a permutation", b);
            seen[v] = 1;
        }
        pl.preds.assign(n, {});
        std::vector<int> indeg(n, 0);
        std::vector<std::vector<int>> succ(n);
        for (int v = 0; v < n; ++v) {
            int deg = 0;
            if (!next(deg) || deg < 0 || deg > 64) return az_fail(AZ_ERR_ARG, "block %d node %d: bad degree", b, v);
            for (int j = 0; j < deg; ++j) {
                int u = 0;
                if (!next(u) || u < 0 || u >= n) return az_fail(AZ_ERR_ARG, "block %d node %d: bad predecessor", b, v);
                pl.preds[v].push_back(u);
                succ[u].push_back(v);
            }
            indeg[v] = deg;
        }
        int no = 0;
        if (!next(no) || no < 1 || no > n) return az_fail(AZ_ERR_ARG, "block %d: bad output count", b);
        pl.outputs.resize(no);
        for (int& v : pl.outputs)
            if (!next(v) || v < 0 || v >= n) return az_fail(AZ_ERR_ARG, "block %d: bad output node", b);
        for (int v : pl.order)
            if (pl.preds[v].empty()) pl.inputs.push_back(v);
        std::vector<int> q = pl.inputs;   // Kahn over `order`
        for (size_t h = 0; h < q.size(); ++h)
            for (int w : succ[q[h]])
                if (--indeg[w] == 0) q.push_back(w);
        if ((int)q.size() != n) return az_fail(AZ_ERR_ARG, "block %d: the wiring has a cycle", b);
        pl.topo = q;
    }
    if (k != n_ints) return az_fail(AZ_ERR_ARG, "graph description: %zu ints read, %zu given", k, n_ints);
    return net_create(e, d, out, true, &plans);
}

int az_randwire_graph(int block, int* order, int* topo, int* inputs, int* n_inputs, int* outputs, int* n_outputs,
                      int* pred_off, int* preds, int preds_cap) {
    if (block < 0 || !order || !topo || !inputs || !n_inputs || !outputs || !n_outputs || !pred_off || !preds)
        return az_fail(AZ_ERR_ARG, "null argument / negative block");
    const azrw::Plan pl = azrw::plan(block);
    const int nn = (int)pl.order.size();
    std::copy(pl.order.begin(), pl.order.end(), order);
    std::copy(pl.topo.begin(), pl.topo.end(), topo);
    std::copy(pl.inputs.begin(), pl.inputs.end(), inputs);
    std::copy(pl.outputs.begin(), pl.outputs.end(), outputs);
    *n_inputs = (int)pl.inputs.size();
    *n_outputs = (int)pl.outputs.size();
    int k = 0;
    for (int v = 0; v < nn; ++v) {
        pred_off[v] = k;
        for (int u : pl.preds[v]) {
            if (k >= preds_cap) return az_fail(AZ_ERR_CAPACITY, "preds_cap %d too small", preds_cap);
            preds[k++] = u;
        }
    }
    pred_off[nn] = k;
    return 0;
}

void az_net_destroy(az_net* n) {
    if (!n) return;
    (void)hipSetDevice(n->e->device);
    delete n;   // its pools free every device buffer
}

int az_net_set_precision(az_net* n, int precision) {
    if (!n) return az_fail(AZ_ERR_ARG, "null net");
    if (int r = check_precision(n->d, n->rw, precision)) return r;
    n->d.precision = precision;
    return 0;
}

int az_net_trunk_kernel(az_net* n, char* name, int len) {
    if (!n || !name || len < 1) return az_fail(AZ_ERR_ARG, "null net / name");
    const az_net_desc& d = n->d;
    const int prec = d.precision;
    const bool f16 = prec == AZ_PREC_FP16;
    const char* res = d.residual ? "true" : "false";
    const NetPlan pl = plan_of(n);
    if (!n->rw && d.blocks < 1) { snprintf(name, len, "gemm_f32"); return 0; }   // no trunk convs
    if (pl.no_forward) return az_fail(AZ_ERR_ARG, "AZ_PREC_F16X3: no fp16-piece trunk for this net");
    // the trunk's convs as net_forward builds them at the net's capacity
    ConvBf16Args a = conv_args(n, d.max_batch, nullptr, d.channels);
    a.pt = prec == AZ_PREC_F16X3 ? 2 : 1;
    int r = 0;
    switch (pl.trunk) {
        // the rand-wire labels carry v4's schedule argument, the NHWC16 ones do not: kept as they are
        case NET_TRUNK_RW_V4_FP16: snprintf(name, len, "conv3x3_v4<2, 128, 1>"); break;
        case NET_TRUNK_RW_V4_X3: snprintf(name, len, "conv3x3_v4<0, 128, 0>"); break;
        case NET_TRUNK_SMALL:   // as rocprofv3 names them
            if (f16) snprintf(name, len, "k_smallnet_g<%d, 8, %s>", d.board_size, res);
            else snprintf(name, len, "k_smallnet_x3<%d, 8, %s, %d>", d.board_size, res, a.pt);
            break;
        case NET_TRUNK_G8X3: r = conv_plan_name(az_conv_x3_plan(a), name, len); break;
        case NET_TRUNK_G8: r = conv_plan_name(az_conv_g8_plan(a, f16 ? 2 : 1), name, len); break;
        case NET_TRUNK_NHWC16: r = conv_plan_name(az_conv_nhwc16_plan(a, f16 ? 2 : prec == AZ_PREC_BF16X3 ? 0 : 1), name, len); break;
        default: snprintf(name, len, "gemm_f32"); break;
    }
    return r ? az_fail(AZ_ERR_ARG, "no trunk kernel for this net") : 0;
}

// Diagnostic: the net's plan (net_plan.h) as one line, e.g. "in=g8/in32 trunk=g8 tail=fused heads=x3-bf16".
int az_diag_net_plan(az_net* n, char* out, int len) {
    if (!n || !out || len < 1) return az_fail(AZ_ERR_ARG, "null net / buffer");
    HIPCHK(hipSetDevice(n->e->device));
    net_plan_line(plan_of(n), out, len);
    return 0;
}

int az_net_profile(az_net* n, int enable) {
    if (!n) return az_fail(AZ_ERR_ARG, "null net");
    std::lock_guard<std::mutex> lk(n->mu);
    n->prof = enable != 0;
    if (n->prof) {
        HIPCHK(hipSetDevice(n->e->device));
        if (int r = n->pc.enable(n->misc)) return r;
    }
    n->pc.used = 0; n->prof_launches = 0; n->prof_forwards = 0; n->prof_tick = 0; n->prof_sampled = 0;
    return 0;
}

int az_net_profile_read(az_net* n, double* trunk_ms, int64_t* trunk_launches, int64_t* forwards) {
    if (!n) return az_fail(AZ_ERR_ARG, "null net");
    std::lock_guard<std::mutex> lk(n->mu);
    HIPCHK(hipSetDevice(n->e->device));
    HIPCHK(hipStreamSynchronize(n->e->stream));
    double ms = 0.0;
    const std::vector<double> t = n->pc.read_ms();
    for (size_t i = 0; i + 1 < t.size(); i += 2) ms += t[i + 1] - t[i];
    // the sampled forwards' trunk time scaled to every profiled forward
    if (trunk_ms) *trunk_ms = n->prof_sampled ? ms * (double)n->prof_forwards / (double)n->prof_sampled : 0.0;
    if (trunk_launches) *trunk_launches = n->prof_launches;
    if (forwards) *forwards = n->prof_forwards;
    return 0;
}

int az_net_forward(az_net* n, const float* planes, int B, float* logits, float* value) {
    return net_host_forward(n, planes, B, logits, value, false);
}

int az_net_predict_batch(az_net* n, const float* planes, int B, float* policy, float* value) {
    return net_host_forward(n, planes, B, policy, value, true);
}

}  // extern "C"
