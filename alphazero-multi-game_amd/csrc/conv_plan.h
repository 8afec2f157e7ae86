// conv_plan.h -- the one place a trunk conv launch is decided: the shape predicates of the conv
// kernels, the conv flag bits, and per kernel family (g8, nhwc16, x3) the plan of one launch -- kernel,
// geometry, tile rows, ring, variant, grid -- with the label that names it.  Plain host C++ without
// HIP (as net_plan.h, which builds the forward's route on these predicates): the launchers in
// conv_bf16.hip / conv_v7.hip only execute a plan, az_net_trunk_kernel prints the same plan's name, and
// tests/test_conv_plan_cpu.py reads the whole table without a GPU.
#pragma once
#include <cstddef>
#include <cstdio>

// ---- the conv flag bits (az_diag_set_conv_flags / az_diag_conv_flags; bench.py --conv-flags, the
// tools and the tests pass the numbers, so the values are fixed).  Every bit but the two defaults
// selects a variant kept for A/B measurement inside one process (tools/net_bench.py --flags) or as the
// reference of a bitwise test; each changes the schedule, never a result bit.
//
//  bit                      selects                                               why the default is what it is
//  CONV_F_V6_AT_15    0x4   15x15 layers with C % 32 == 0 that v7 leaves run on   default on: 16x16x32 MFMAs; the 16-plane input
//                           conv3x3_v6 (off: conv3x3_v5)                          layer stays on v5, 126 vs 146 us per 2048-board
//                                                                                 launch (profiles/r05_fused_tail_ab.txt)
//  CONV_F_DENSE_15    0x8   DENSE tiles at 15x15 (v6 and v7); the other boards    B = 2048, --flags 0x4,0xc: dense 19x19 -3.1 %,
//                           are always DENSE                                      13x13 -4.0 %, 9x9 -14 %, 8x8 -20 % trunk time, 15x15
//                                                                                 +8.7 % (two padded boards fill a 512-row v6 tile at
//                                                                                 88 % and 2048 boards are exactly 8 rounds)
//  CONV_F_NO_V7       0x100 conv3x3_v6 / v5 wherever v7 would run                 the bitwise suites' reference
//  CONV_F_V7_ONLY_15  0x200 from 1024 boards on, v7 at 15x15 only                 default on
//  CONV_F_V7_PAD_15   0x400 v7's padded 15x17 tile at 15x15 (default SLIM)
//  CONV_F_V7_ANY_BATCH 0x800 v7 below 1024 boards too                             15x15, B = 256: v6 61 us, v7 65 (one or two rounds)
//  CONV_F_V6_SMALL    0x1000 v6 for the other boards below 1024 boards            v7's 128 / 64-row tiles fill the CUs there: 128
//                                                                                 boards of 8x8 0.0237 vs 0.0644 ms, 19x19 0.0594 vs
//                                                                                 0.0747 (profiles/r04_small_batch_tiles_192.txt)
//  CONV_F_V7_PER_TAP  0x2000 the SLIM tile keeps v7's per-tap main loop (weight   read by the kernel: a wave-uniform branch between
//                           ring in LDS, one barrier per tap), not the            the two compiled loops
//                           row-streamed one
//  CONV_F_V7_OLD_TAIL 0x4000 the row-streamed loop's unpeeled tile tail (the last read by the kernel.  (A residual L2 prefetch in the
//                           chunk reloads itself, the residual join reads global  main loop measured 0.6 % slower and was removed; a
//                           memory)                                               cross-row fragment prefetch and a mid-row barrier
//                                                                                 1.5-2 % slower)
//  CONV_F_V7_OLD_EPILOGUE 0x8000 the row-streamed loop ends in the shared tile    read by the kernel.  B = 2048, fp16, lean against
//                           epilogue (per-element pointer tests, 64-bit store     shared in one process: 0.4244 vs 0.4592 ms per
//                           addresses), not its own lean one                      launch, reversed 0.4249 vs 0.4618 (-7.6 / -8.0 %,
//                                                                                 spread 0.0115; profiles/r10_v7_epilogue_ab.txt)
//  CONV_F_V7_TM     0x70000 force v7's DENSE tile rows: 1 = 256, 2 = 128,         conv_v7_tm below
//                           3 = 64, 4 = 192
//  CONV_F_V7_RING3  0x80000 3-slot weight ring for tiles of at most 128 rows      conv_v7_ring below
//  CONV_F_KEEP_POOL 0x400000 k_pool_g8 + the head GEMMs, not the fused tail       net_plan.h
//  CONV_F_FC_F32  0x8000000 the f32 k_fc_heads, not k_fc_heads_x3                 net_plan.h
//  CONV_F_V7X3   0x10000000 conv3x3_v7x3 where v9x3 would run (N % 256 == 0)
//  CONV_F_V9_TAP_BARRIER 0x20000000  v9x3: the tap barrier at the tap start, not after unit U0 (bf16 pieces only)
//  CONV_F_V9_KEEP_FRAG   0x40000000  v9x3: the SLIM tile's dead 16th fragment stays in waves 4-7 (bf16 pieces only)
enum : int {
    CONV_F_V6_AT_15 = 0x4, CONV_F_DENSE_15 = 0x8, CONV_F_NO_V7 = 0x100, CONV_F_V7_ONLY_15 = 0x200, CONV_F_V7_PAD_15 = 0x400,
    CONV_F_V7_ANY_BATCH = 0x800, CONV_F_V6_SMALL = 0x1000, CONV_F_V7_PER_TAP = 0x2000, CONV_F_V7_OLD_TAIL = 0x4000,
    CONV_F_V7_OLD_EPILOGUE = 0x8000, CONV_F_V7_TM = 0x70000, CONV_F_V7_TM_SHIFT = 16, CONV_F_V7_RING3 = 0x80000, CONV_F_KEEP_POOL = 0x400000,
    CONV_F_FC_F32 = 0x08000000, CONV_F_V7X3 = 0x10000000, CONV_F_V9_TAP_BARRIER = 0x20000000,
    CONV_F_V9_KEEP_FRAG = 0x40000000,
    CONV_F_DEFAULT = CONV_F_V6_AT_15 | CONV_F_V7_ONLY_15   // 0x204
};

// ---- shape predicates of the conv kernels (the launchers add their pointer checks)

// zeroed 16-bit elements behind every g8 activation buffer (512 KB): the v6 / v7 convs point the DMA
// of halo padding rows there
constexpr size_t AZ_ACT_TAIL = 262144;

// boards with a G8Geom instantiation
inline bool az_g8_board(int H) { return H == 8 || H == 9 || H == 13 || H == 15 || H == 19; }
// the g8 trunk (conv3x3_v5 at 15x15 / v6 / v7): square boards, 128-channel output halves, 16-channel
// chunks (v5, 15x15) or 32 (v6)
inline bool az_conv_g8_supported(int H, int W, int C, int N) {
    if (H != W || !az_g8_board(H) || N % 128 != 0 || C < 16) return false;
    return H == 15 ? C % 16 == 0 : C % 32 == 0;
}
inline bool az_conv_v4_supported(int H, int W, int C, int N) { return H == 15 && W == 15 && C % 16 == 0 && N % 64 == 0; }

// conv3x3_v6 / v7 / v7x3 / v9x3 address activations and weights through 32-bit buffer ranges, and
// their padding offset walks C / 32 chunk steps of 4 HW 16 B into the zeroed tail
inline bool az_act_range_ok(size_t a_tail) { return a_tail + AZ_ACT_TAIL * 2 < ((size_t)1 << 31); }
inline bool az_weight_range_ok(int C, int N) { return (size_t)9 * C * N * 2 < ((size_t)1 << 31); }
inline bool az_tail_reach_ok(int H, int C) { return (size_t)(C / 32) * 4 * ((size_t)H * H) * 16 + 16 <= AZ_ACT_TAIL * 2; }
// the shapes conv3x3_v7 and the x3 convs (v7x3 / v9x3) take; a_tail: bytes in front of the zeroed tail
inline bool az_conv_v7_shape_supported(int H, int W, int C, int N, size_t a_tail) {
    return H == W && az_g8_board(H) && C % 64 == 0 && N % 128 == 0 && az_act_range_ok(a_tail) && az_tail_reach_ok(H, C) &&
           az_weight_range_ok(C, N);
}

// What the decisions read of one launch's ConvBf16Args (net.h conv_shape): the sizes and which
// optional outputs and residuals are present.
struct ConvShape {
    int H, W, C, N, M;
    size_t a_tail;            // bytes in front of the activations' zeroed tail (0: M * C * 2, g8 family only)
    int rows_per_sample, relu;
    int pt;                   // x3 family: pieces 1 = bf16 (0 reads as 1), 2 = fp16
    bool Cf, Clo, Cq, Rq, Rhi, Rlo;
};

// conv3x3_v7 takes the layer: a ReLU, no fp32 output, no lo plane
inline bool conv_v7_supported(const ConvShape& s) {
    return s.relu && !s.Cf && !s.Clo && az_conv_v7_shape_supported(s.H, s.W, s.C, s.N, s.a_tail);
}
// conv3x3_v7x3 / v9x3 (the g8 hi / lo planes): the shapes of conv3x3_v7; a residual needs both of its
// planes (az_conv_v7x3_launch checks the planes that must be there)
inline bool conv_x3_supported(const ConvShape& s) {
    if (!s.relu || s.Cf || s.Cq || s.Rq || s.Rhi != s.Rlo) return false;
    return s.a_tail >= (size_t)s.M * s.C * 2 && az_conv_v7_shape_supported(s.H, s.W, s.C, s.N, s.a_tail);
}

// ---- the plan of one launch

enum { CONV_NONE = 0, CONV_BF16, CONV_V3, CONV_V4, CONV_V5, CONV_V6, CONV_V7, CONV_V7X3, CONV_V9X3 };
// tile geometries of v6 (PAD / DENSE) and v7 / v7x3 / v9x3 (conv_v7.hip Geom7)
enum { GEO_PAD = 0, GEO_SLIM = 1, GEO_DENSE = 2 };

struct ConvPlan {
    int kernel;               // CONV_*; CONV_NONE: no kernel takes the shape, the launch is refused
    int mode;                 // operands: 0 bf16 hi + lo (three MFMAs per product), 1 bf16, 2 fp16
    int pt;                   // v7x3 / v9x3: pieces 1 bf16, 2 fp16
    int board, geo;           // v6 / v7 / v7x3 / v9x3: the board template argument and GEO_*
    int tm, ring;             // v7 / v7x3 / v9x3: MFMA rows of a tile; v7: weight-ring slots
    int bm, bn;               // v3: the tile pair
    int bnt, sched, boards, nt;   // v4: channels per block, schedule, boards per block, threads
    int var;                  // v9x3: the variant template argument
    bool stagger;             // v9x3: the first-round start offsets apply
    int rows, cols;           // a block covers rows of M (one tile), the grid has cols blocks along N
    unsigned grid, block;     // the launch: blocks and threads (no kernel takes dynamic LDS)
};

namespace conv_plan_detail {

// grid of the g8 kernels: the XCD-aware tile / half mapping needs whole groups of 8 tiles
inline void grid_g8(ConvPlan& p, const ConvShape& s, long tiles, int block) {
    p.cols = s.N / 128;
    p.grid = (unsigned)((tiles + 7) / 8 * 8 * p.cols);
    p.block = block;
}

// The DENSE tile rows of a conv3x3_v7 launch: 256 unless the launch is under two rounds of blocks
// (two blocks per CU), where 192 / 128 / 64-row tiles spread the work over more CUs.
inline int conv_v7_tm(const ConvShape& s, int flags) {
    const int force = (flags & CONV_F_V7_TM) >> CONV_F_V7_TM_SHIFT;
    if (force) return force == 1 ? 256 : force == 2 ? 128 : force == 3 ? 64 : 192;
    const long rows = (long)s.M;
    const int halves = s.N / 128;
    const long boards = rows / ((long)s.H * s.W);
    auto blocks = [&](int tm) { return ((rows + tm - 1) / tm + 7) / 8 * 8 * halves; };
    // below 1024 boards (conv_plan_g8's small-batch branch) 19x19 -- and 13x13 once 128-row tiles fill
    // the CUs -- take 128-row tiles on the 3-slot ring (conv_v7_ring) at every size, including
    // those whose 256-row tiles would make 1024 blocks: 19x19 128 boards 0.0594 ms (192-row: 0.0620),
    // 256: 0.1106 (0.1160), 384: 0.1645 (256-row: 0.1887), 512: 0.2111 (0.2268; v6 0.2107), 768:
    // 0.3085 (0.3392) (profiles/r05_small_batch_ring3.txt)
    if (boards < 1024 && (s.H == 19 || (s.H == 13 && blocks(128) >= 512))) return 128;
    if (blocks(256) >= 1024) return 256;
    if (blocks(128) >= 512) return 128;
    return 64;
}

// Weight-ring slots of a DENSE conv3x3_v7 launch with tiles under 256 rows: 3 (three blocks per CU)
// for the automatic 128-row tiles or with CONV_F_V7_RING3, else 4 (two blocks per CU).  128-row
// tiles, 4 -> 3 slots: 19x19 128 boards 0.0620 (192-row) -> 0.0594 ms, 13x13 256 0.0709 -> 0.0592,
// 13x13 512 0.1230 -> 0.1092, 9x9 512 0.0700 -> 0.0578, 8x8 512 0.0444 -> 0.0436; the 64-row tiles
// measured within +-2 % (8x8 128 0.0217 vs 0.0221, 9x9 256 0.0360 vs 0.0353) and keep 4
// (profiles/r05_small_batch_ring3.txt)
inline int conv_v7_ring(int tm, int flags) {
    if (tm > 128) return 4;
    if (flags & CONV_F_V7_RING3) return 3;
    return (tm == 128 && !(flags & CONV_F_V7_TM)) ? 3 : 4;
}

// conv3x3_v7 / v7x3 / v9x3 tiles: DENSE tiles are tm consecutive pixels of the batch, else one board
inline long tiles7(ConvPlan& p, const ConvShape& s) {
    const long boards = s.M / (s.H * s.W);
    p.rows = p.geo == GEO_DENSE ? p.tm : s.H * s.W;
    return p.geo == GEO_DENSE ? (boards * s.H * s.W + p.tm - 1) / p.tm : boards;
}

inline ConvPlan v7(ConvPlan p, const ConvShape& s, int geo, int flags) {
    p.kernel = CONV_V7;
    p.geo = geo;
    p.tm = geo == GEO_DENSE ? conv_v7_tm(s, flags) : 256;
    p.ring = geo == GEO_DENSE ? conv_v7_ring(p.tm, flags) : 4;
    grid_g8(p, s, tiles7(p, s), 256);
    return p;
}

}  // namespace conv_plan_detail

// The g8 family (NET_TRUNK_G8 and its input conv; mode 1 bf16 / 2 fp16): conv3x3_v7, v6 or v5.
inline ConvPlan conv_plan_g8(ConvShape s, int mode, int flags) {
    using namespace conv_plan_detail;
    ConvPlan p{};
    p.mode = mode;
    p.board = s.H;
    if (s.a_tail == 0) s.a_tail = (size_t)s.M * s.C * 2;
    if ((mode != 1 && mode != 2) || s.H != s.W || !az_conv_g8_supported(s.H, s.W, s.C, s.N)) return p;
    // conv3x3_v7 (conv_v7.hip, two 256-thread blocks per CU, epilogue from registers) takes every
    // layer it supports (trunk convs: C % 64 == 0) from 1024 boards on.  15x15 below 1024 boards: a
    // launch is one or two rounds of blocks and v6 is faster; the other boards take v7's small DENSE
    // tiles there (next branch).  15x15 tile geometry: SLIM, every other board DENSE.
    const int boards = s.M / (s.H * s.W);
    const bool v7_ok = conv_v7_supported(s);
    if (!(flags & CONV_F_NO_V7) && (s.H == 15 || !(flags & CONV_F_V7_ONLY_15)) &&
        (boards >= 1024 || (flags & CONV_F_V7_ANY_BATCH)) && v7_ok)
        return v7(p, s, (s.H != 15 || (flags & CONV_F_DENSE_15)) ? GEO_DENSE : (flags & CONV_F_V7_PAD_15) ? GEO_PAD : GEO_SLIM,
                  flags);
    // Small batches on the DENSE boards (the per-rank shards of the 8-GPU C4 / C5 configs): v6's
    // 512-row tiles leave most CUs idle (C5 net, 128 boards: 32 blocks), conv3x3_v7 with 128 / 64-row
    // tiles (conv_v7_tm) fills them; 19x19 on 128-row tiles with three blocks per CU: 0.1106 vs 0.1375
    // ms at 256 boards (profiles/r04_small_batch_tiles_192.txt, r05_small_batch_ring3.txt)
    if (!(flags & (CONV_F_NO_V7 | CONV_F_V6_SMALL)) && s.H != 15 && boards < 1024 && v7_ok) return v7(p, s, GEO_DENSE, flags);
    if (s.a_tail < (size_t)s.M * s.C * 2) return p;
    if (s.H != 15 || ((flags & CONV_F_V6_AT_15) && s.C % 32 == 0)) {
        // v6: the padding offset walks (C/32) chunk steps of 4*HW*16 B into the zeroed tail, and the
        // buffer descriptor's 32-bit range must cover the activations plus that tail; conv3x3_v6
        // always applies the ReLU
        if (s.C % 32 != 0 || !az_act_range_ok(s.a_tail) || !az_tail_reach_ok(s.H, s.C) || !s.relu) return p;
        p.kernel = CONV_V6;
        // DENSE tiles: any 512 consecutive pixels; the padded 15x15 grid: two boards per 512-row tile
        p.geo = (s.H != 15 || (flags & CONV_F_DENSE_15)) ? GEO_DENSE : GEO_PAD;
        p.rows = p.geo == GEO_DENSE ? 512 : 2 * 225;
        grid_g8(p, s, p.geo == GEO_DENSE ? ((long)boards * s.H * s.W + 511) / 512 : (boards + 1) / 2, 512);
        return p;
    }
    p.kernel = CONV_V5;           // 15x15, 16-channel chunks: two boards per block
    p.rows = 2 * 225;
    grid_g8(p, s, (boards + 1) / 2, 512);
    return p;
}

// The nhwc16 family (NET_TRUNK_NHWC16 and the rand-wire node convs; mode 0 bf16 hi + lo / 1 bf16 /
// 2 fp16): conv3x3_v4 on 15x15 boards, else v3 (N % 256 == 0 or N == 64, C % 32 == 0), else
// conv3x3_bf16 (128 x 128 register-staged tiles, any shape).  fp16 operands have v4 only.
inline ConvPlan conv_plan_nhwc16(const ConvShape& s, int mode, int flags) {
    (void)flags;                  // no variant bit reaches this family
    ConvPlan p{};
    p.mode = mode;
    if (mode < 0 || mode > 2) return p;
    if (s.rows_per_sample == 225 && az_conv_v4_supported(s.H, s.W, s.C, s.N)) {
        const int boards = s.M / 225;
        p.kernel = CONV_V4;
        p.bnt = s.N % 128 == 0 ? 128 : 64;
        p.block = 512;
        if (mode == 0 && p.bnt == 64 && boards <= 512) {   // one board per block: fill the CUs at small batches
            p.sched = 1; p.boards = 1; p.nt = 512;
        } else {                  // bf16 hi + lo keeps the single-buffered schedule: the double buffer spills at 256 VGPRs
            p.sched = mode == 0 ? 0 : 1; p.boards = 2; p.nt = 512;
        }
        p.rows = p.boards * 225;
        p.cols = s.N / p.bnt;
        p.grid = (unsigned)((boards + p.boards - 1) / p.boards * p.cols);
        return p;
    }
    if (mode == 2) return p;
    if (s.C % 32 == 0 && (s.N % 256 == 0 || s.N == 64)) {
        p.kernel = CONV_V3;
        p.bm = s.N % 256 == 0 ? 128 : 256;
        p.bn = s.N % 256 == 0 ? 256 : 64;
        p.block = s.N % 256 == 0 ? 512 : 256;
    } else {
        p.kernel = CONV_BF16;
        p.bm = p.bn = 128;
        p.block = 256;
    }
    p.rows = p.bm;
    p.cols = (s.N + p.bn - 1) / p.bn;
    p.grid = (unsigned)((s.M + p.bm - 1) / p.bm * p.cols);
    return p;
}

// The x3 family (NET_TRUNK_G8X3; pieces s.pt): conv3x3_v9x3 takes every layer with N % 256 == 0, else
// conv3x3_v7x3; 15x15 boards on the SLIM tile, every other board DENSE (as conv3x3_v7's defaults).
inline ConvPlan conv_plan_x3(const ConvShape& s, int flags) {
    using namespace conv_plan_detail;
    ConvPlan p{};
    p.pt = s.pt == 2 ? 2 : 1;
    p.board = s.H;
    if (!conv_x3_supported(s)) return p;
    p.geo = s.H == 15 ? GEO_SLIM : GEO_DENSE;
    p.tm = 256;
    const long tiles = tiles7(p, s);
    if (s.N % 256 == 0 && !(flags & CONV_F_V7X3)) {
        p.kernel = CONV_V9X3;
        // fp16 pieces (AZ_PREC_F16X3) run the default variant only
        p.var = p.pt == 2 ? 3 : ((flags & CONV_F_V9_TAP_BARRIER) ? 0 : 1) | ((flags & CONV_F_V9_KEEP_FRAG) ? 0 : 2);
        p.cols = s.N / 256;
        p.grid = (unsigned)(tiles * p.cols);
        p.block = 512;
        // the first-round stagger (az_diag_set_v9_stagger) only on launches of >= 1024 blocks (several
        // rounds), where a one-off delay of the last-started CU is amortised
        p.stagger = p.grid >= 1024;
        return p;
    }
    p.kernel = CONV_V7X3;
    grid_g8(p, s, tiles, 256);
    return p;
}

// The plan's kernel as bench.py's roofline label names it; -1 for CONV_NONE.
inline int conv_plan_name(const ConvPlan& p, char* out, int len) {
    static const char* const geo[3] = {"PAD", "SLIM", "DENSE"};
    const char* const ops = p.mode == 0 ? "split" : "bf16";
    switch (p.kernel) {
        case CONV_BF16: snprintf(out, len, "conv3x3_bf16<%s>", ops); return 0;
        case CONV_V3: snprintf(out, len, "conv3x3_v3<%s, %d, %d>", ops, p.bm, p.bn); return 0;
        case CONV_V4: snprintf(out, len, "conv3x3_v4<%d, %d>", p.mode, p.bnt); return 0;
        case CONV_V5: snprintf(out, len, "conv3x3_v5<%d, 8>", p.mode); return 0;
        case CONV_V6: snprintf(out, len, "conv3x3_v6<%d, %d%s>", p.mode, p.board, p.geo == GEO_DENSE ? ", DENSE" : ""); return 0;
        case CONV_V7:
            if (p.ring != 4) snprintf(out, len, "conv3x3_v7<%d, %d, %s, %d, %d>", p.mode, p.board, geo[p.geo], p.tm, p.ring);
            else if (p.tm != 256) snprintf(out, len, "conv3x3_v7<%d, %d, %s, %d>", p.mode, p.board, geo[p.geo], p.tm);
            else snprintf(out, len, "conv3x3_v7<%d, %d, %s>", p.mode, p.board, geo[p.geo]);
            return 0;
        case CONV_V7X3:
        case CONV_V9X3:
            snprintf(out, len, "%s<%d, %s%s>", p.kernel == CONV_V9X3 ? "conv3x3_v9x3" : "conv3x3_v7x3", p.board, geo[p.geo],
                     p.pt == 2 ? ", f16" : "");
            return 0;
        default: return -1;
    }
}
