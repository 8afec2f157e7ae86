// net_plan.h -- how a network runs, derived once from its description: the shape predicates of the
// kernels, the forward's route (input stage, trunk family, tail, head FCs, refusals) and the weight
// sets a load packs for it.  Plain host C++ without HIP (as weight_pack.h): net_host.hip dispatches on
// the plan, net_load.hip packs what net_packs names, the launchers call the same predicates, and
// tests/test_net_plan_cpu.py reads the whole table without a GPU.
//
// The plan picks the kernel family; the instantiation for one launch (v6 / v7 by the batch, the v7
// tile rows and ring, v3 / v4 / conv3x3_bf16, v9x3 / v7x3 by the width, v4's one-board variant) is
// conv_plan.h's, which also holds the conv kernels' shape predicates and the conv flag bits.
#pragma once
#include <cstddef>
#include <cstdio>

#include "../../include/az_engine.h"
#include "conv_plan.h"

// ---- shape predicates of the fused kernels (the conv kernels': conv_plan.h)

// k_smallnet: 15x15, 64 filters, 16 input planes, heads of 32 channels; its biases sit in LDS rows
// (smallnet.hip asserts both constants against SF and SmGeom<15>::MAXL)
constexpr int AZ_SMALLNET_F = 64;
constexpr int AZ_SMALLNET_MAX_BLOCKS = 15;
inline bool az_smallnet_supported(int H, int C, int cin_pad, int pool, int head_channels) {
    return H == 15 && C == AZ_SMALLNET_F && cin_pad == 16 && pool >= 1 && pool <= 8 && 2 * head_channels == AZ_SMALLNET_F &&
           head_channels % 4 == 0;
}

// k_pool_heads_g8: 32-channel slices, at most 64 cells, both heads' 1x1 convs = 64 outputs; its dynamic
// LDS (the board's pooled-cell partial sums + two 64 x 33 weight tiles) within the device's limit per
// workgroup (68.9 KB at 19x19 fits gfx950's 160 KB, not a 64 KB part)
inline size_t az_pool_heads_lds(int H) { return ((size_t)H * H * 36 + 2 * 64 * 33) * sizeof(float); }
inline bool az_pool_heads_supported(int C, int H, int P, int N, size_t lds_limit) {
    return C % 32 == 0 && P * P <= 64 && N == 64 && H * H <= 361 && az_pool_heads_lds(H) <= lds_limit;
}

// ---- the route

// The az_net_desc fields the route depends on.  cin_pad: input channels padded to 16 (the search's
// plane records); more than 16 planes on a net of 128-channel halves pad to 32 so the v6 conv takes
// the input layer as whole 32-channel chunks.
struct NetShape {
    int board, in_planes, channels, blocks, head_channels, pool, max_batch;
    bool rw;          // DDW-RandWire trunk
    int cin_pad;
};
inline NetShape net_shape(const az_net_desc& d, bool rw) {
    NetShape s{d.board_size, d.in_planes, d.channels, d.blocks, d.head_channels, d.pool, d.max_batch, rw, 0};
    s.cin_pad = (d.in_planes + 15) / 16 * 16;
    if (s.cin_pad > 16 && d.channels % 128 == 0) s.cin_pad = (d.in_planes + 31) / 32 * 32;
    return s;
}

// The weight sets a load builds beside the f32 layers and the FC piece rows (which every net gets).
// By the shape alone: az_net_set_precision only switches the dispatch, so a load packs what any
// precision the shape accepts will read.
struct NetPacks {
    bool sm;        // k_smallnet's sets (sm_*): fp16, bf16 hi / lo and scaled fp16 hi / lo pieces
    bool in16;      // 16-bit split + chunk-blocked copies of the input conv
    bool in32;      // the input conv zero-padded from 16 to 32 channels (g8 boards other than 15x15)
    bool trunk16;   // 16-bit split + chunk-blocked copies of every 3x3 trunk / node conv
};
inline NetPacks net_packs(const NetShape& s) {
    const int H = s.board, F = s.channels;
    NetPacks k{};
    k.trunk16 = F % 32 == 0;
    if (s.rw) return k;
    k.sm = az_smallnet_supported(H, F, s.cin_pad, s.pool, s.head_channels) && s.blocks <= AZ_SMALLNET_MAX_BLOCKS;
    k.in16 = F % 32 == 0;
    k.in32 = s.cin_pad == 16 && H != 15 && az_conv_g8_supported(H, H, F, F) && az_conv_g8_supported(H, H, 32, F);
    return k;
}

// How the forward reads its input planes: NET_IN_SMALL (k_smallnet), NET_IN_G8 (k_to_g8 + the g8
// input conv) -- both can build board b's planes from the search's leaf record gidx[b]
// (leaf_planes.h), so the search hands its leaves over without a plane batch -- or NET_IN_GEMM (f32
// input conv on x0).
enum { NET_IN_GEMM = 0, NET_IN_SMALL = 1, NET_IN_G8 = 2 };
enum {
    NET_TRUNK_GEMM_F32 = 0,   // gemm_f32 on the fp32 NHWC stream
    NET_TRUNK_SMALL,          // k_smallnet_g / k_smallnet_x3: input conv, trunk, pool and head convs in one launch
    NET_TRUNK_G8,             // conv3x3_v5 / v6 / v7 on 16-bit g8 planes
    NET_TRUNK_G8X3,           // conv3x3_v7x3 / v9x3 on g8 hi / lo planes
    NET_TRUNK_NHWC16,         // conv3x3_v4 / v3 / conv3x3_bf16: bf16, bf16 split, fp16 with the fp32 residual stream
    NET_TRUNK_RW_F32,         // rand-wire nodes on gemm_f32
    NET_TRUNK_RW_V4_FP16,     // rand-wire nodes on conv3x3_v4, fp16 operands
    NET_TRUNK_RW_V4_X3        // rand-wire nodes on conv3x3_v4, bf16 hi / lo operands
};
enum {
    NET_HEADS_GENERIC = 0,    // split-K gemm_f32 per FC layer
    NET_HEADS_F32,            // k_fc_heads, exact f32 products
    NET_HEADS_X3_BF16,        // k_fc_heads_x3, bf16 pieces
    NET_HEADS_X3_FP16         // k_fc_heads_x3, scaled fp16 pieces
};

struct NetPlan {
    int input;              // NET_IN_*
    bool in32;              // NET_IN_G8: the zero-padded 32-channel input layer (else the net's own)
    int trunk;              // NET_TRUNK_*; NET_TRUNK_G8 always comes with NET_IN_G8
    bool tail_fused;        // pool + both head 1x1 convs in k_pool_heads_g8
    bool head_conv_fused;   // else: both head 1x1 convs as one GEMM (hconv), or one GEMM each
    int heads;              // NET_HEADS_*
    // what az_net_create* / az_net_set_precision answer: 0, or the status with its message
    int status;
    char message[224];
    // a net they accept whose forward is refused all the same (AZ_ERR_ARG with this text), or null
    const char* no_forward;
};

namespace net_plan_detail {

inline void refuse(NetPlan& p, const char* msg) {
    p.status = AZ_ERR_ARG;
    snprintf(p.message, sizeof p.message, "%s", msg);
}

// The precisions a shape is created at / switched to.
inline void refusal(const NetShape& s, int prec, NetPlan& p) {
    const int H = s.board, F = s.channels;
    if (s.rw) {
        // AZ_PREC_F32 (the reference module's arithmetic, any shape), or on 15x15 with channels % 64 == 0
        // the conv3x3_v4 node convs: AZ_PREC_BF16X3 (fp32-faithful split operands, fp32 routers) or
        // AZ_PREC_FP16 (fp16 operands, fp16-operand routers); what passes here passes the plain checks
        if (prec != AZ_PREC_F32 && !((prec == AZ_PREC_FP16 || prec == AZ_PREC_BF16X3) && az_conv_v4_supported(H, H, F, F)))
            refuse(p, "rand-wire nets: AZ_PREC_F32, or AZ_PREC_BF16X3 / AZ_PREC_FP16 on 15x15 with channels % 64 == 0");
        return;
    }
    if (prec < 0 || prec > 4) {
        p.status = AZ_ERR_ARG;
        snprintf(p.message, sizeof p.message, "bad precision %d", prec);
        return;
    }
    if (prec == AZ_PREC_F16X3) {
        // the fp16-piece kernels: conv3x3_v9x3 / v7x3 (az_conv_v7_shape_supported at the capacity, but
        // for the zeroed-tail reach, which only the forward applies) or k_smallnet_x3; a net without
        // blocks passes here as well
        const bool trunk = az_g8_board(H) && F % 128 == 0 && az_act_range_ok((size_t)s.max_batch * H * H * F * 2) &&
                           az_weight_range_ok(F, F);
        if (!trunk && !net_packs(s).sm && s.blocks > 0)
            return refuse(p, "AZ_PREC_F16X3 needs an 8/9/13/15/19 board with channels % 128 == 0 (and under 2 GiB "
                             "per activation buffer), or the 15x15 64-channel net; use AZ_PREC_BF16X3 or AZ_PREC_F32");
    }
    if (prec != AZ_PREC_F32 && F % 32) return refuse(p, "bf16/fp16 trunk needs channels % 32 == 0");
    if (prec == AZ_PREC_FP16 && !az_conv_v4_supported(H, H, F, F) && !az_conv_g8_supported(H, H, F, F))
        refuse(p, "AZ_PREC_FP16 trunk needs 15x15 boards and channels % 64 == 0, or an 8/9/13/15/19 board "
                  "and channels % 128 == 0");
}

}  // namespace net_plan_detail

// conv_flags: az_conv_flags() (CONV_F_KEEP_POOL keeps k_pool_g8 + the head GEMMs, CONV_F_FC_F32 the
// f32 k_fc_heads); lds_limit: the device's LDS per workgroup.
inline NetPlan net_plan(const NetShape& s, int prec, int conv_flags, size_t lds_limit) {
    NetPlan p{};
    net_plan_detail::refusal(s, prec, p);
    const int H = s.board, F = s.channels, HK = s.head_channels * s.pool * s.pool;
    const bool x3 = prec == AZ_PREC_BF16X3 || prec == AZ_PREC_F16X3, h16 = prec == AZ_PREC_BF16 || prec == AZ_PREC_FP16;
    const bool bf = (x3 || h16) && F % 32 == 0;
    const NetPacks k = net_packs(s);
    p.input = NET_IN_GEMM;
    if (s.rw) {
        // below 128 boards of capacity v4 has too few tiles (one per two boards) and the K-split f32
        // GEMM is faster (chosen by capacity: batch-size independent)
        p.trunk = prec == AZ_PREC_FP16 ? NET_TRUNK_RW_V4_FP16
                  : prec == AZ_PREC_BF16X3 && s.max_batch >= 128 ? NET_TRUNK_RW_V4_X3 : NET_TRUNK_RW_F32;
    } else if (k.sm && (prec == AZ_PREC_FP16 || x3) && s.blocks > 0) {
        p.input = NET_IN_SMALL;
        p.trunk = NET_TRUNK_SMALL;
    } else if (bf && h16 && az_conv_g8_supported(H, H, F, F)) {
        // 16 planes on a board whose g8 conv needs 32-channel chunks: in32 (15x15 keeps 16 channels on
        // conv3x3_v5: 126 us per 2048-board launch against 146 us for conv3x3_v6 on the zero-padded 32,
        // profiles/r05_fused_tail_ab.txt).  One of the two always serves a g8 net: cin_pad is 16 or a
        // multiple of 32 there
        const bool own = k.in16 && az_conv_g8_supported(H, H, s.cin_pad, F);
        p.trunk = NET_TRUNK_G8;
        if (own || k.in32) { p.input = NET_IN_G8; p.in32 = !own; }
    } else if (bf && x3 && s.blocks >= 1 && az_conv_v7_shape_supported(H, H, F, F, (size_t)s.max_batch * H * H * F * 2)) {
        p.trunk = NET_TRUNK_G8X3;
    } else {
        p.trunk = bf ? NET_TRUNK_NHWC16 : NET_TRUNK_GEMM_F32;
    }
    if (prec == AZ_PREC_F16X3 && p.trunk != NET_TRUNK_G8X3 && p.trunk != NET_TRUNK_SMALL)
        p.no_forward = "AZ_PREC_F16X3: no fp16-piece trunk for this shape";
    p.tail_fused = (p.trunk == NET_TRUNK_G8 || p.trunk == NET_TRUNK_G8X3) && HK % 32 == 0 &&
                   az_pool_heads_supported(F, H, s.pool, 2 * s.head_channels, lds_limit) && !(conv_flags & CONV_F_KEEP_POOL);
    p.head_conv_fused = p.trunk != NET_TRUNK_SMALL && !p.tail_fused && HK % 32 == 0;
    // split-operand FC products at 5x the f32 MFMA rate: the throughput precisions (fp16 / bf16 trunk)
    // in bf16 pieces (~2^-16 per product; their trunk error is 30x larger), AZ_PREC_F16X3 in scaled fp16
    // pieces (~2^-21, as its trunk).  AZ_PREC_BF16X3 and F32 keep exact f32 products (bf16 pieces would
    // add ~2.5e-5 at trained-scale logits).  Below 512 boards of capacity the f32 pair is the faster
    // one (C2, 256 boards: k_fc_heads 10.6 us vs k_fc_heads_x3 12.0 -- both latency-bound chains of L2
    // round trips at 0.5 GFLOP)
    const bool fx = !(conv_flags & CONV_F_FC_F32) && s.max_batch >= 512;
    p.heads = HK % 32 ? NET_HEADS_GENERIC
              : fx && h16 ? NET_HEADS_X3_BF16 : fx && prec == AZ_PREC_F16X3 ? NET_HEADS_X3_FP16 : NET_HEADS_F32;
    return p;
}

// One line for az_diag_net_plan, e.g. "in=g8/in32 trunk=g8 tail=fused heads=x3-bf16"; a refused
// precision reads "refused: <message>".
inline void net_plan_line(const NetPlan& p, char* out, int len) {
    static const char* const in[] = {"gemm", "small", "g8"};
    static const char* const trunk[] = {"gemm_f32", "small", "g8", "g8x3", "nhwc16", "rw_f32", "rw_v4_fp16", "rw_v4_x3"};
    static const char* const heads[] = {"generic", "f32", "x3-bf16", "x3-fp16"};
    if (p.status) { snprintf(out, len, "refused: %s", p.message); return; }
    snprintf(out, len, "in=%s%s trunk=%s tail=%s heads=%s%s", in[p.input], p.input == NET_IN_G8 ? (p.in32 ? "/in32" : "/in") : "",
             trunk[p.trunk], p.trunk == NET_TRUNK_SMALL ? "trunk" : p.tail_fused ? "fused" : p.head_conv_fused ? "hconv" : "convs",
             heads[p.heads], p.no_forward ? " no-forward" : "");
}
