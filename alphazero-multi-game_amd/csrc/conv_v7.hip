// conv_v7.hip -- 3x3 trunk convolution of the g8 residual stream (fp16 / bf16 MFMA, gfx950).
//
//   out[b][n][pix] = relu( sum_{tap,c} A[b][c][pix + tap] * W[n][tap][c] + bias[n] (+ res) )
//
// Same data formats as conv3x3_v6 (conv_bf16.hip): activations in the g8 layout
// [board][C/8][pixel][8] 16-bit with an int8 remainder plane of the residual stream, weights
// chunk-blocked [C/16][9][2][N][8], zero padding read from the zeroed tail behind every
// activation buffer (AZ_ACT_TAIL).  What changes is the shape of the work:
//
//  * a 256-thread block (4 waves) owns a 256-row output tile x 128 channels and needs 72 KB of
//    LDS (halo of one 32-channel chunk double-buffered, 2 x 20 KB; a 4-slot ring of per-tap
//    weight tiles, 4 x 8 KB), so TWO blocks share a CU.  The scheduler interleaves them: while one
//    block sits in a barrier or in its epilogue, the other block's waves keep the SIMD's matrix
//    pipe busy (v6 runs one 512-thread block per CU and its epilogue leaves the pipes idle);
//  * the MFMA operands are swapped (weights as the 16-row operand, activations as the 16-column
//    one), so a lane's accumulator holds 4 consecutive output CHANNELS of one pixel: the epilogue
//    joins the residual, applies the ReLU, splits the result into 16 bits + int8 remainder and
//    stores straight from registers -- no LDS staging, no block barrier, each wave on its own;
//  * one barrier per tap.  Weight tiles land 4 taps ahead; each barrier certifies the NEXT tap's
//    tile, so every fragment of tap s+1 is read during tap s's MFMAs (no read latency after a
//    barrier).  The halo of chunk c+1 is fetched during taps 0..4 of chunk c;
//  * the SLIM 15x15 tile (the C3 trunk) runs a row-streamed main loop instead: the halo row pitch is
//    one fragment, so each of 17 fragment rows x 3 column shifts is read from LDS once and multiplied
//    into up to three output fragments; a wave owns the whole board x 32 channels and holds its tap
//    weights of the chunk in registers, loaded straight from the packed weights.  There is one
//    barrier per chunk (see the loop).  Its blocks own 80 KB: the halo double buffer (2 x 20 KB) and
//    40 KB into which a 2nd conv's residual tile is fetched by LDS-DMA during the main loop (the last
//    five of its 15 fragment rows go into the halo buffer the peeled last chunk leaves idle), so the
//    epilogue's join reads LDS and the residual's HBM traffic is spread over the tile's MFMA time.
//    It ends in an epilogue of its own (epilogue_rows: the residual / remainder tests decided once per
//    wave, buffer stores from one base per wave and plane; conv flag 0x8000 keeps the shared one).
//
// Tile geometry (as v6): 15x15 boards use the padded grid (outputs on a 15x17 grid, one board per
// 256-row tile, 225 of 256 rows live) or DENSE tiles; every other board uses DENSE tiles (256
// consecutive pixels of the batch; taps that leave the board are zeroed in the fragments).
// The result is bit-identical to conv3x3_v6 (same products, same accumulation order).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

#include "net.h"

// conv3x3_v7's output stores: streaming (nt) by default; AZ_V7_ST_PLAIN=1 builds plain stores (A/B of
// the row-boundary partial writes)
#if defined(AZ_V7_ST_PLAIN) && AZ_V7_ST_PLAIN
#define AZ_V7_ST ""
#else
#define AZ_V7_ST " nt"
#endif

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void lds_void_t;

template <int MODE>
struct H16 {                                           // MODE 2: fp16, MODE 1: bf16 (as Half16, conv_bf16.hip)
    __device__ static float to_f(uint16_t h) {
        if (MODE == 2) { _Float16 x; __builtin_memcpy(&x, &h, 2); return (float)x; }
        return __uint_as_float((uint32_t)h << 16);
    }
    __device__ static uint16_t from_f(float f) {
        if (MODE == 2) { _Float16 x = (_Float16)f; uint16_t h; __builtin_memcpy(&h, &x, 2); return h; }
        uint32_t u = __float_as_uint(f);
        u += 0x7fffu + ((u >> 16) & 1u);
        return (uint16_t)(u >> 16);
    }
    static constexpr int SH = 16 - (MODE == 2 ? 11 : 8);
    __device__ static void split(float x, uint16_t& h, int8_t& q) {
        h = from_f(x);
        const int d = (int)(__float_as_uint(x) - __float_as_uint(to_f(h)));
        const int r = (d + (1 << (SH - 1))) >> SH;
        q = (int8_t)min(127, max(-127, r));
    }
    __device__ static float join(uint16_t h, int8_t q) {
        return __uint_as_float(__float_as_uint(to_f(h)) + ((uint32_t)(int)q << SH));
    }
};

// The split-operand (x3) kernels' piece type: PT 1 = bf16 pieces (AZ_PREC_BF16X3), PT 2 = fp16 pieces
// (AZ_PREC_F16X3; weights per-output-channel power-of-2 scaled, undone in the epilogue by oscale)
template <int PT> struct X3T;
template <> struct X3T<1> {
    typedef bf16x8 frag;
    __device__ static f32x4v mma(const frag& b, const frag& a, const f32x4v& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(b, a, c, 0, 0, 0);
    }
};
template <> struct X3T<2> {
    typedef f16x8 frag;
    __device__ static f32x4v mma(const frag& b, const frag& a, const f32x4v& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(b, a, c, 0, 0, 0);
    }
};

__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)p; }

#ifdef AZ_V9_STAMPS
// Diagnostic builds only (make EXTRA=-DAZ_V9_STAMPS OUT=build_stamps): wave 0 of every block of the
// selected conv3x3_v9x3 launch (ConvBf16Args::stamp == g_v9_sel) records s_memrealtime (100 MHz) at
// its start, after the prologue barrier, after the main loop, after the epilogue's stores issue and
// after they complete, plus HW_ID / XCC_ID (tools/v9_stamps.py)
constexpr int V9_MAXB = 8192;
__device__ int g_v9_sel = -1;
__device__ unsigned long long g_v9_st[V9_MAXB][5];
__device__ unsigned g_v9_hw[V9_MAXB][2];
#define V9_STAMP(k)                                                                                 \
    do {                                                                                            \
        if (p.stamp == g_v9_sel && tid == 0 && blockIdx.x < V9_MAXB) {                              \
            g_v9_st[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();                              \
            if (k == 0) {                                                                           \
                g_v9_hw[blockIdx.x][0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);                 \
                g_v9_hw[blockIdx.x][1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);                \
            }                                                                                       \
        }                                                                                           \
    } while (0)
#else
#define V9_STAMP(k) do { } while (0)
#endif

#ifdef AZ_V7_STAMPS
// Diagnostic builds only (make EXTRA=-DAZ_V7_STAMPS OUT=build_stamps7): wave 0 of every block of the
// selected conv3x3_v7 launch (ConvBf16Args::stamp == g_v7_sel) records s_memrealtime (100 MHz) at its
// start, after the prologue barrier, at the main loop's end, when the first residual operands are in
// registers (conv1: right away), after the last store issues and after all stores complete, plus
// HW_ID / XCC_ID (tools/v7_stamps.py).  Row-streamed path only.
constexpr int V7_MAXB = 8192, V7_NST = 6;
__device__ int g_v7_sel = -1;
__device__ unsigned long long g_v7_st[V7_MAXB][V7_NST];
__device__ unsigned g_v7_hw[V7_MAXB][2];
#define V7_STAMP(k)                                                                                 \
    do {                                                                                            \
        if (p.stamp == g_v7_sel && tid == 0 && blockIdx.x < V7_MAXB) {                              \
            g_v7_st[blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();                              \
            if (k == 0) {                                                                           \
                g_v7_hw[blockIdx.x][0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);                 \
                g_v7_hw[blockIdx.x][1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);                \
            }                                                                                       \
        }                                                                                           \
    } while (0)
#else
#define V7_STAMP(k) do { } while (0)
#endif

template <int OFF, typename F>
__device__ __forceinline__ void ds_rd(F& d, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "i"(OFF) : "memory");
}
// s_waitcnt lgkmcnt(N) with the fragments it certifies as in-out operands, so every MFMA that
// reads them is ordered after the wait (the ds_reads are inline asm the compiler does not track)
template <int N, typename F>
__device__ __forceinline__ void lgkm(F (&x)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]) : "i"(N) : "memory");
}

template <int N, typename F>
__device__ __forceinline__ void lgkm1(F& x) {          // the same for one fragment
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(x) : "i"(N) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmc() {           // s_waitcnt vmcnt(N), N a compile-time constant
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

__device__ __forceinline__ void wait_vm(int n) {      // s_waitcnt vmcnt(n), n wave-uniform
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

// The row-streamed epilogue's output stores: a buffer store through a wave-uniform resource `rs`
// (four SGPRs) at the lane's byte offset `vo` + the scalar offset `so` + the immediate OFF (< 4096).
// asm volatile with a memory clobber, as the shared epilogue's global stores: the stores stay in
// program order, which is what keeps the rows' LDS reads and conversions from being hoisted in one go.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4_t store_rsrc(const void* base, uint32_t bytes) {   // base wave-uniform
    const uint64_t a = (uint64_t)(uintptr_t)base;
    return u32x4_t{(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a),
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)) & 0xffffu, bytes, 0x00020000u};
}
template <int OFF>
__device__ __forceinline__ void bst_b64(u32x2_t v, uint32_t vo, u32x4_t rs, int so) {
    static_assert(OFF >= 0 && OFF < 4096, "buffer immediate");
    asm volatile("buffer_store_dwordx2 %0, %1, %2, %3 offen offset:%4" AZ_V7_ST ::"v"(v), "v"(vo), "s"(rs), "s"(so), "i"(OFF) : "memory");
}
template <int OFF>
__device__ __forceinline__ void bst_b32(uint32_t v, uint32_t vo, u32x4_t rs, int so) {
    static_assert(OFF >= 0 && OFF < 4096, "buffer immediate");
    asm volatile("buffer_store_dword %0, %1, %2, %3 offen offset:%4" AZ_V7_ST ::"v"(v), "v"(vo), "s"(rs), "s"(so), "i"(OFF) : "memory");
}

template <int I, int N, typename Fn>
__device__ __forceinline__ void static_for(Fn&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Tile geometries (GEO_*, conv_plan.h; one board per tile unless DENSE):
//  GEO_PAD   outputs on an HB x (HB+2) grid: tap (dy, dx) of output row q is halo row q + dy*WG + dx
//            of the zero-padded (HB+2)^2 halo (two dead columns per grid row; 15x15: 225 of 256 rows live)
//  GEO_SLIM  outputs on an HB x (HB+1) grid over a halo of HB+2 rows of HB+1 columns whose column 0
//            is zero: the one zero column is the right neighbour of x = HB-1 (the next grid row's
//            column 0) and the left neighbour of x = 0, so no tap needs masking; one dead column per
//            grid row (15x15: 240 rows = 15 fragments of 16; the 16th fragment of the tile reads the
//            halo's all-zero rows >= 256 instead, so its MFMAs run on zero operands, which cost the
//            power-limited chip little -- a branch around them would route every accumulator
//            through phi copies and spill)
//  GEO_DENSE 256 consecutive pixels of the batch, taps that leave the board zeroed in the fragments
//  TM        DENSE only: output rows per tile (256; 128 / 64 for small batches, conv3x3_v7 only)
template <int HB, int GEO, int TM = 256>
struct Geom7 {
    static constexpr bool DENSE = GEO == GEO_DENSE, SLIM = GEO == GEO_SLIM;
    static constexpr int WG = DENSE ? HB : SLIM ? HB + 1 : HB + 2;   // grid / halo row width
    static constexpr int HW = HB * HB;
    static constexpr int GRID = DENSE ? TM : HB * WG;                // output grid rows of a tile
    static constexpr int NFRAG = (GRID + 15) / 16;                   // 16-row fragments with live rows
    static constexpr int TROWS = DENSE ? TM + 2 * HB + 2 : SLIM ? NFRAG * 16 + 2 * WG + 2 : (HB + 2) * (HB + 2);
    // DMA pieces of 64 rows per 8-channel group: 5 (320 rows) for 256-row tiles
    static constexpr int HROWS = (DENSE && TM < 256) ? (TROWS + 63) / 64 * 64 : 320;
    static constexpr int NRB = HROWS / 64;
    static_assert(TROWS <= HROWS, "halo does not fit");
    static_assert(DENSE ? (TM == 256 || TM == 192 || TM == 128 || TM == 64) : (TM == 256 && GRID <= 256 && NFRAG > 8),
                  "tile geometry");
};

}  // namespace

// MODE 2: fp16 operands, MODE 1: bf16.  Requires C % 64 == 0 (an even number of 32-channel
// chunks), N % 128 == 0, a ReLU (every g8 conv has one), no fp32 output.
// TM < 256 (DENSE, small batches): each wave owns TM / 2 rows = NI fragments (6, 4 or 2) x 64
// channels in one or two A register sets of NA fragments; the halo is NRB pieces per group.
// RG: weight-tile ring slots (4: tiles land 4 taps ahead, two blocks per CU; 3: 3 taps ahead, and
// with TM <= 128 (LDS 48 KB, <= 168 VGPRs) THREE blocks per CU -- small batches, more resident waves
// to hide the per-tap barrier and fragment latencies)
template <int MODE, int HB, int GEO, int TM = 256, int RG = 4>
__global__ __launch_bounds__(256, RG == 3 ? 3 : 2) void conv3x3_v7(ConvBf16Args p) {
    typedef H16<MODE> H;
    typedef Geom7<HB, GEO, TM> GM;
    constexpr bool DENSE = GM::DENSE, SLIM = GM::SLIM;
    typedef typename std::conditional<MODE == 2, f16x8, bf16x8>::type frag;
    constexpr int BNT = 128, WG = GM::WG, HW = GM::HW, HROWS = GM::HROWS, NRB = GM::NRB;
    constexpr int NI = TM / 32, NA = NI <= 4 ? NI : NI / 2, HALVES = NI / NA;   // fragments per wave / per A set
#ifdef AZ_V7_NOSKIP
    constexpr bool SKIP = false;
#else
    constexpr bool SKIP = SLIM && HALVES == 2;            // waves wm = 1 skip the SLIM tile's dead 16th fragment
#endif
    static_assert(NA * HALVES == NI && NA <= 4, "fragment split");
    static_assert(RG == 4 || (RG == 3 && TM <= 128), "ring");
    constexpr int WR = TM / 2;                            // rows per wave
    constexpr int A_BUF = 4 * HROWS * 16;                 // one chunk: [4 groups][320 rows][16 B] = 20 KB
    constexpr int B_TAP = 4 * BNT * 16;                   // one tap: [4 groups][128 ch][16 B] = 8 KB
    constexpr bool ROWS = SLIM && WG == 16 && TM == 256 && RG == 4;   // the row-streamed main loop's geometry
    constexpr int R_ROW = 4 * 1024;                       // ROWS: one fragment row of the block's residual tile (4 waves x 1 KB)
    // 72 KB (RG 4, TM 256); 48 KB (RG 3, TM 128); ROWS 80 KB: behind the halo double buffer, rows 0..9
    // of the residual tile's 16-bit plane (the per-tap loop's weight ring shares that area)
    constexpr int LDS = ROWS ? 2 * A_BUF + 10 * R_ROW : 2 * A_BUF + RG * B_TAP;
    static_assert(LDS >= 2 * A_BUF + RG * B_TAP && LDS <= 80 * 1024, "two blocks per CU");
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;             // 128 pixels x 64 channels per wave
    const int nsplit = p.N / BNT;
    const int xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int nb = slot % nsplit, tile = (slot / nsplit) * 8 + xcd;   // a tile's channel halves share an XCD
    const int n0 = nb * BNT;
    const int nboards = p.m_limit ? *p.m_limit : p.M / HW;
    if (DENSE ? tile * TM >= nboards * HW : tile >= nboards) return;
    V7_STAMP(0);
    const int C = p.C, GI = C / 8, GO = p.N / 8;
    const int NCH = C / 32, NS = 9 * NCH;

    const uint32_t a_bytes = (uint32_t)p.a_tail, b_bytes = (uint32_t)((size_t)9 * C * p.N * 2);
    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Ahi, (short)0, (int)(a_bytes + AZ_ACT_TAIL * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.Bblk, (short)0, (int)b_bytes, 0x00020000);
    const uint32_t PAD = a_bytes;                         // zeroed tail: padding rows

    // halo piece j of this wave: q = wave + 4j -> (8-channel group g, 64-row block rb); the lane's
    // source offset is recomputed at every issue (a handful of VALU; keeping five offsets live
    // across the main loop would spill)
    auto a_src = [&](int j, int ln) -> uint32_t {
        const int q = wave + 4 * j, rb = q % NRB, g = q / NRB;
        const int hr = rb * 64 + ln;
        int Y, X, b;
        bool in;
        if constexpr (DENSE) {                            // halo row -> pixel tile*TM - HB - 1 + hr
            const int gpx = tile * TM - (HB + 1) + hr;
            b = gpx >= 0 ? gpx / HW : -1;
            const int pix = gpx - b * HW;
            Y = pix / HB + 1; X = pix - (Y - 1) * HB + 1;
            in = hr < GM::TROWS && gpx >= 0;
        } else {
            Y = hr / WG; X = hr - Y * WG;
            b = tile;
            in = hr < GM::TROWS;
        }
        const bool ok = in && Y >= 1 && Y <= HB && X >= 1 && X <= HB && b < nboards;   // SLIM: X = 0 is the zero column
        return ok ? (uint32_t)((((size_t)b * GI + g) * HW + (Y - 1) * HB + (X - 1)) * 16) : PAD;
    };
    // weight pieces: q = wave + 4j (j = 0, 1) -> (group g = q / 2, 64-channel block rb = q % 2)
    int b_src[2], b_dst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wave + 4 * j, rb = q & 1, g = q >> 1;
        b_src[j] = (((g >> 1) * 18 + (g & 1)) * p.N + n0 + rb * 64) * 16;
        b_dst[j] = g * (BNT * 16) + rb * 1024;
    }
    const uint32_t lane16 = lane * 16;
    uint8_t* abuf = lds;
    uint8_t* bbuf = lds + 2 * A_BUF;
    // voffset = the lane's part (VGPR), soffset = the wave-uniform part (SGPR): keeps the per-tap
    // offsets out of vector registers
    auto issueA = [&](int j, int c, int buf) {            // piece j of chunk c's halo into A buffer `buf`
        const int q = wave + 4 * j, rb = q % NRB, g = q / NRB;
        int ln = lane;
        asm volatile("" : "+v"(ln));                      // recompute here, do not hoist
        const uint32_t vo = a_src(j, ln);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)(abuf + buf * A_BUF + g * (HROWS * 16) + rb * 1024),
                                                 16, (int)vo, __builtin_amdgcn_readfirstlane(c * (4 * HW * 16)), 0, 0);
    };
    auto issueB = [&](int s, int slot) {                  // the wave's two pieces of tap s's weights
        const int c = s / 9, t = s - 9 * c;
        const int so = __builtin_amdgcn_readfirstlane((36 * c + 2 * t) * p.N * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)(bbuf + slot * B_TAP + b_dst[j]), 16,
                                                     (int)lane16, so + b_src[j], 0, 0);
    };

    const int l16 = lane & 15, lg = lane >> 4;

    // epilogue, straight from the accumulators acc[NIE][NJ] of a wave tile of NIE fragment rows from
    // output grid row q0 x NJ 16-channel operands from channel chl - 4*lg: lane holds channels
    // chl + 16j + e of pixel l16 of every 16 x 16 tile; residual join, ReLU, 16-bit + int8 split,
    // streaming stores
    // fetch(i, j, e, h, q): the residual of fragment row i, operand j (element index e): 16-bit plane h,
    // int8 remainder q -- res_mem from global memory; the row-streamed loop has them on chip already
    auto res_mem = [&](int, int, size_t e, u32x2_t& h, uint32_t& q) {
        const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rhi, (short)0, 0x7fffffff, 0x00020000);
        const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rq, (short)0, 0x7fffffff, 0x00020000);
        h = __builtin_amdgcn_raw_buffer_load_b64(rh, (int)(e * 2), 0, AZ_RES_AUX);
        q = __builtin_amdgcn_raw_buffer_load_b32(rq, (int)e, 0, AZ_RES_AUX);
    };
    auto epilogue = [&](auto& acc, const int q0, const int chl, auto&& fetch) {
    typedef typename std::remove_reference<decltype(acc)>::type AccT;
    constexpr int NIE = std::extent<AccT, 0>::value, NJ = std::extent<AccT, 1>::value;
    float vmax = 0.0f;                                    // fp16: the largest output (the range guard)
    auto locate = [&](int i, int& b, int& pix) -> bool {  // fragment row i of the lane: board, pixel, live
        const int q = q0 + i * 16 + l16;                  // output grid row of the tile
        if constexpr (DENSE) {
            const int gq = tile * TM + q;
            b = gq / HW;
            pix = gq - b * HW;
            return b < nboards;
        } else {
            const int y = q / WG, x = q - y * WG;
            b = tile;
            pix = y * HB + x;
            return y < HB && x < HB;
        }
    };
    // The residual join's loads go out EB fragment rows at a time (one memory round trip per burst,
    // two per wave at NIE = 8, five at 15), not one round trip per row: each row's loads would
    // otherwise wait behind the previous row's stores (the asm stores are memory barriers to the
    // compiler), and a 2nd conv's epilogue was eight serial HBM round trips per wave (conv2 498 us
    // vs conv1 423 us per C3 launch under PMC, profiles/r06_c3_fp16_pmc_calib.json).  <= 48 VGPRs per
    // burst; the arithmetic and the stored values are unchanged.
    constexpr int EB = NIE <= 4 ? NIE : NIE % 4 == 0 ? 4 : NIE % 3 == 0 ? 3 : NIE % 2 == 0 ? 2 : 1;
    static_assert(NIE % EB == 0, "bursts");
#pragma unroll
    for (int i0 = 0; i0 < NIE; i0 += EB) {
    u32x2_t hv[EB][NJ];
    uint32_t qv[EB][NJ];
    if (p.Rhi) {
#pragma unroll
        for (int ii = 0; ii < EB; ++ii) {
            int b, pix;
            if (!locate(i0 + ii, b, pix)) continue;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int ch = chl + j * 16;
                const size_t e = (((size_t)b * GO + (ch >> 3)) * HW + pix) * 8 + (ch & 7);
                fetch(i0 + ii, j, e, hv[ii][j], qv[ii][j]);
            }
        }
    }
#ifdef AZ_V7_STAMPS
    if (i0 == 0) {                                        // the first burst's residual operands are in registers
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        V7_STAMP(3);
    }
#endif
#pragma unroll
    for (int ii = 0; ii < EB; ++ii) {
        const int i = i0 + ii;
        int b, pix;
        if (!locate(i, b, pix)) continue;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int ch = chl + j * 16;
            const size_t e = (((size_t)b * GO + (ch >> 3)) * HW + pix) * 8 + (ch & 7);
            float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (p.Rhi) {
                uint16_t hh[4];
                int8_t qq[4];
                __builtin_memcpy(hh, &hv[ii][j], 8);
                __builtin_memcpy(qq, &qv[ii][j], 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] += H::join(hh[k], qq[k]);
            }
            uint16_t oh[4];
            int8_t oq[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = __builtin_amdgcn_fmed3f(o[k], 0.0f, 3.0e38f);   // ReLU
                if constexpr (MODE == 2) vmax = __builtin_fmaxf(vmax, o[k]);
                if (p.Cq) H::split(o[k], oh[k], oq[k]);
                else oh[k] = H::from_f(o[k]);
            }
            u32x2_t hs;
            __builtin_memcpy(&hs, oh, 8);
            asm volatile("global_store_dwordx2 %0, %1, off" AZ_V7_ST ::"v"(p.Chi + e), "v"(hs) : "memory");
            if (p.Cq) {
                uint32_t qs;
                __builtin_memcpy(&qs, oq, 4);
                asm volatile("global_store_dword %0, %1, off" AZ_V7_ST ::"v"(p.Cq + e), "v"(qs) : "memory");
            }
        }
    }
    }
    if (MODE == 2 && !(vmax <= 65504.0f) && p.ovf) atomicOr(p.ovf, 1);   // fp16 overflow: the engine fails the forward
    };

    // The row-streamed main loop (SLIM 15x15, 256-row tile, 4-slot geometry; the default there, conv
    // flag 0x2000 keeps the per-tap loop below).  On the SLIM grid the halo row pitch WG is exactly one
    // fragment (16 rows), so the fragment that output fragment i reads at tap (dy, dx) IS the fragment
    // that output fragment i + dy reads at tap (0, dx): fragment row f = 0..16, shifted by dx, is read
    // from LDS once and multiplied into acc[f] (tap row 0), acc[f-1] (tap row 1) and acc[f-2] (tap row
    // 2) -- 51 fragment reads per chunk instead of 72 / 63.
    //  * wave tile: all 15 live fragments of the board x 32 channels n0 + 32*wave + 16j (120
    //    accumulator registers); no row halves, no dead 16th fragment, every wave does 270 MFMAs per chunk;
    //  * the wave's weights of a chunk (9 taps x 2 operands, 72 registers) come straight from the
    //    packed layout [C/16][9][2][N][8] by 16-B buffer loads (an operand is four 256-B runs, one per
    //    8-channel group): no weight tiles in LDS, no weight DMA, and with the ring gone ONE block
    //    barrier per chunk (the halo double buffer) instead of one per tap;
    //  * the next chunk's weights roll in behind the last use of each tap row: W(0,.) is dead after
    //    f = 14, W(1,.) after f = 15, W(2,.) after f = 16, and each row is reloaded right there;
    //  * every accumulator still receives its nine taps in the order t = 3*dy + dx (f ascending is dy
    //    ascending for a fixed output fragment), chunk after chunk, seeded by the bias: the result is
    //    bitwise that of the per-tap loop and of conv3x3_v6.
    //  * the last chunk is peeled: it has no next halo and no next weights to fetch and no barrier.
    //    A 2nd conv's residual tile arrives during the main loop instead of in the epilogue, where the
    //    co-resident blocks' joins would all ask HBM at once.  The wave's part of the 16-bit plane is
    //    15 fragment rows x 4 eight-channel groups; one row is one 1-KB LDS-DMA piece (lane = group x
    //    16 grid pixels, the dead 16th column re-reads pixel 14).  Rows 0..9 go behind the halo
    //    buffers, a few per chunk from the first chunk on (up to four, at dx == 1 of f = 0..3, so that
    //    they precede the chunk's last halo piece in the vmcnt order); rows 10..14 go into the halo
    //    buffer the last chunk leaves idle, in the slots where an unpeeled last chunk would reload its
    //    own halo.  The 30 int8-remainder loads of the wave go out in the last chunk too, into the
    //    registers of the dead tap rows.  Every piece is read back only by the wave that fetched it,
    //    after its own vmcnt(0) behind the loop: no barrier.  Conv flag 0x4000 keeps the unpeeled
    //    tile tail (the last chunk reloads itself, the join reads global memory in bursts of three rows).
    // vmcnt counts the halo's DMA pieces, the residual pieces and the weight loads together in issue
    // order; the budget before the chunk barrier is a compile-time constant (see there).
    if constexpr (ROWS) {
        if (!(p.flags & CONV_F_V7_PER_TAP)) {
            constexpr int NF = GM::NFRAG, NFR = NF + 2;   // 15 output fragments, 17 fragment rows of the halo
            static_assert(NF == 15 && NRB == 5 && (NFR * 16 + 2) <= GM::TROWS, "row-streamed geometry");
            f32x4v acc[NF][2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {                 // the bias seeds the accumulators
                const float4 bv = *reinterpret_cast<const float4*>(p.bias + n0 + wave * 32 + j * 16 + 4 * lg);
#pragma unroll
                for (int i = 0; i < NF; ++i) acc[i][j] = f32x4v{bv.x, bv.y, bv.z, bv.w};
            }
            // weight operand j of tap t of chunk c: rows n0 + 32*wave + 16j + l16 of the 16-channel
            // blocks 2c + (lg >> 1), half lg & 1; lane part in a VGPR, the rest in the scalar offset
            const int N16 = p.N * 16;
            const uint32_t w_lane = (uint32_t)((18 * (lg >> 1) + (lg & 1)) * N16 + l16 * 16);
            const int w_wave = (n0 + wave * 32) * 16;
            frag W[3][3][2];
            auto loadW = [&](int c, auto dyc) {           // tap row dy of chunk c
                constexpr int dy = decltype(dyc)::value;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int so = __builtin_amdgcn_readfirstlane((36 * c + 2 * (3 * dy + dx)) * N16 + w_wave);
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const auto v = __builtin_amdgcn_raw_buffer_load_b128(rsB, (int)(w_lane + j * 256), so, 0);
                        __builtin_memcpy(&W[dy][dx][j], &v, 16);
                    }
                }
            };
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            // fragment (f, dx): halo rows 16f + dx + l16 of group lg (the top row read is 273 < TROWS)
            const uint32_t a_lane = lds_addr(abuf) + lg * (HROWS * 16) + l16 * 16;
            frag F[3];                                    // step k = 3f + dx lives in F[k % 3]

            // prologue: halo of chunk 0, then the 18 weight loads of chunk 0
#pragma unroll
            for (int j = 0; j < NRB; ++j) issueA(j, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            loadW(0, I0{});
            loadW(0, I1{});
            loadW(0, I2{});
            __builtin_amdgcn_sched_barrier(0);
            wait_vmc<18>();                               // the halo landed; the weights may fly
            __builtin_amdgcn_s_barrier();
            V7_STAMP(1);
            __builtin_amdgcn_sched_barrier(0);
            ds_rd<0 * 16>(F[0], a_lane);
            ds_rd<1 * 16>(F[1], a_lane);
            ds_rd<2 * 16>(F[2], a_lane);

            // The residual tile: nothing of it on a conv without residual or under flag 0x4000.  Row r of
            // the wave's 15: rows 0..RR0-1 behind the halo buffers, the rest in halo buffer NCH & 1,
            // which the last chunk (reading buffer (NCH - 1) & 1) leaves idle; [row][wave][1 KB].
            constexpr int RR0 = 10;
            static_assert(2 * A_BUF + RR0 * R_ROW <= LDS && (NF - RR0) * R_ROW <= A_BUF && NF - RR0 <= NRB, "residual images");
            const bool tail_old = (p.flags & CONV_F_V7_OLD_TAIL) != 0;
            const bool resid = p.Rhi && !tail_old;
            const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rhi, (short)0, 0x7fffffff, 0x00020000);
            uint8_t* const r_lo = lds + 2 * A_BUF + wave * 1024;
            uint8_t* const r_hi = abuf + (NCH & 1) * A_BUF + wave * 1024;
            auto issueR = [&](int r) {                    // r wave-uniform
                int ln = lane;
                asm volatile("" : "+v"(ln));              // recompute here, do not hoist
                const uint32_t vo = (uint32_t)(((ln >> 4) * HW + min(ln & 15, HB - 1)) * 16);
                const int so = __builtin_amdgcn_readfirstlane((int)((((size_t)tile * GO + (n0 + wave * 32) / 8) * HW + r * HB) * 16));
                uint8_t* dst = r < RR0 ? r_lo + r * R_ROW : r_hi + (r - RR0) * R_ROW;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsR, (lds_void_t*)dst, 16, (int)vo, so, 0, AZ_RES_AUX);
            };
            // rows 0..RR0-1 spread over the chunks before the last: `per` of them per chunk (at most the
            // four slots a chunk has); what few chunks (C < 128) leave over goes out first in the last chunk
            int rnext = 0;
            const int per = resid ? min(4, (RR0 + NCH - 2) / (NCH - 1)) : 0;
            // the int8 remainder of fragment row i (the dead 16th column re-reads pixel 14)
            uint32_t QV[NF][2];
            auto loadQ = [&](int i) {
                const __amdgpu_buffer_rsrc_t rq = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rq, (short)0, 0x7fffffff, 0x00020000);
                const uint32_t qo = (uint32_t)((((n0 + wave * 32) / 8 + (lg >> 1)) * HW + min(l16, HB - 1)) * 8 + 4 * (lg & 1));
                const int so = __builtin_amdgcn_readfirstlane((int)(((size_t)tile * GO * HW + i * HB) * 8));
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    QV[i][j] = __builtin_amdgcn_raw_buffer_load_b32(rq, (int)(qo + j * (2 * HW * 8)), so, AZ_RES_AUX);
            };
            auto res_lds = [&](int i, int j, size_t, u32x2_t& h, uint32_t& q) {
                const uint8_t* src = (i < RR0 ? r_lo + i * R_ROW : r_hi + (i - RR0) * R_ROW) + (2 * j + (lg >> 1)) * 256 + l16 * 16 + (lg & 1) * 8;
                h = *reinterpret_cast<const u32x2_t*>(src);
                q = QV[i][j];
            };
            // The row-streamed path's own epilogue (the default; conv flag 0x8000 keeps the shared one
            // above, which tests p.Rhi / p.Cq per element and rebuilds a 64-bit address per store: about
            // 3 100 instructions per wave between the first and the last store against 1 780 here on a
            // 2nd conv, 263 on a first conv -- DESIGN.md section 5.3, "Round 10").  Same values, same
            // arithmetic, same stored bytes; what differs is the bookkeeping around them:
            //  * RES (a residual tile is on chip) and REM (the int8 remainder plane is written) are
            //    compile-time facts, one copy per combination net_forward launches: a first conv
            //    (no, no), a 2nd conv (yes, yes), a 2nd conv of a net without residual (no, yes);
            //  * one buffer resource per output plane whose base is the wave's own tile -- board `tile`,
            //    channel groups (n0 + 32 wave) / 8 .. + 3 -- and whose range is exactly that tile (4 x HW
            //    x 16 B; half in the int8 plane): a store's offset is the lane's part (group pair, pixel
            //    column, channel half), the operand's 2 HW x 16 B in a scalar and the fragment row's
            //    HB x 16 B as an immediate.  No 64-bit arithmetic per store, and no plane size limit;
            //  * the dead 16th grid column is one execution mask around the whole body (its accumulators
            //    stay out of the range guard, as in the shared epilogue);
            //  * rows go in bursts of three behind scheduling fences, so the live set stays the
            //    accumulators, the remainders and one burst's operands.
            auto epilogue_rows = [&](auto rc, auto qc) {
                constexpr bool RES = decltype(rc)::value, REM = decltype(qc)::value;
                constexpr int EB = 3;
                static_assert(NF % EB == 0 && (NF - 1) * HB * 16 < 4096, "bursts, store immediates");
                int* const ovf = p.ovf;
                const size_t ebase = ((size_t)tile * GO + (n0 + wave * 32) / 8) * HW * 8;
                const u32x4_t rsH = store_rsrc(p.Chi + ebase, 4 * HW * 16);
                const u32x4_t rsQ = REM ? store_rsrc(p.Cq + ebase, 4 * HW * 8) : u32x4_t{};
                const uint32_t voQ = (uint32_t)(((lg >> 1) * HW + l16) * 8 + (lg & 1) * 4), voH = 2 * voQ;
                const uint32_t lsrc = (uint32_t)((lg >> 1) * 256 + l16 * 16 + (lg & 1) * 8);
                float vmax = 0.0f;                        // fp16: the largest live output (the range guard)
                if (l16 < HB) {
                    static_for<0, NF / EB>([&](auto bc) {
                        constexpr int i0 = decltype(bc)::value * EB;
                        u32x2_t hv[EB][2];
                        if constexpr (RES) {
                            static_for<0, EB>([&](auto ic) {
                                constexpr int ii = decltype(ic)::value, i = i0 + ii;
                                const uint8_t* src = (i < RR0 ? r_lo + i * R_ROW : r_hi + (i - RR0) * R_ROW) + lsrc;
#pragma unroll
                                for (int j = 0; j < 2; ++j) hv[ii][j] = *reinterpret_cast<const u32x2_t*>(src + j * 512);
                            });
                        }
#ifdef AZ_V7_STAMPS
                        if constexpr (i0 == 0) {          // the first burst's residual operands are in registers
                            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                            V7_STAMP(3);
                        }
#endif
                        static_for<0, 2 * EB>([&](auto sc) {
                            constexpr int ii = decltype(sc)::value / 2, j = decltype(sc)::value % 2, i = i0 + ii;
                            float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                            if constexpr (RES) {
                                uint16_t hh[4];
                                int8_t qq[4];
                                __builtin_memcpy(hh, &hv[ii][j], 8);
                                __builtin_memcpy(qq, &QV[i][j], 4);
#pragma unroll
                                for (int k = 0; k < 4; ++k) o[k] += H::join(hh[k], qq[k]);
                            }
                            uint16_t oh[4];
                            int8_t oq[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                o[k] = __builtin_amdgcn_fmed3f(o[k], 0.0f, 3.0e38f);   // ReLU
                                if constexpr (MODE == 2) vmax = __builtin_fmaxf(vmax, o[k]);
                                if constexpr (REM) H::split(o[k], oh[k], oq[k]);
                                else oh[k] = H::from_f(o[k]);
                            }
                            u32x2_t hs;
                            __builtin_memcpy(&hs, oh, 8);
                            bst_b64<i * HB * 16>(hs, voH, rsH, j * (2 * HW * 16));
                            if constexpr (REM) {
                                uint32_t qs;
                                __builtin_memcpy(&qs, oq, 4);
                                bst_b32<i * HB * 8>(qs, voQ, rsQ, j * (2 * HW * 8));
                            }
                        });
                        __builtin_amdgcn_sched_barrier(0);
                    });
                    if (MODE == 2 && !(vmax <= 65504.0f) && ovf) atomicOr(ovf, 1);   // fp16 overflow: the engine fails the forward
                }
            };

            // one chunk; lastc: the peeled last chunk
            auto chunk = [&](const int c, auto lastc) {
                constexpr bool LASTC = decltype(lastc)::value;
                const int cn = c + 1 < NCH ? c + 1 : c;   // flag 0x4000: the last chunk reloads itself
                const uint32_t a_cur = a_lane + (c & 1) * A_BUF, a_nxt = a_lane + ((c + 1) & 1) * A_BUF;
                if constexpr (LASTC) {
                    if (resid)
                        for (; rnext < RR0; ++rnext) issueR(rnext);
                }
                static_for<0, 3 * NFR>([&](auto kc) {
                    constexpr int k = decltype(kc)::value, f = k / 3, dx = k % 3, r = k % 3;
                    constexpr int LAST = 3 * (NFR - 1);   // first step of the last fragment row
                    if constexpr (k == LAST) {
                        // every fragment read of this chunk has landed (none is issued after this point),
                        // and so have this wave's pieces of the next halo: the six W(0,.) loads issued at
                        // f = 15 are the only younger vector-memory operations -- the halo's last piece
                        // goes out at k = 12, the chunk's residual pieces before it (k = 1, 4, 7, 10), so
                        // vmcnt(6) certifies both whether or not this chunk fetched residual rows.  Past
                        // the barrier every wave is done with this chunk's halo buffer, which the next
                        // chunk's DMA overwrites, and the next chunk's halo is complete.  The last chunk
                        // has nothing to certify and no buffer to hand over: no barrier.
                        lgkm1<0>(F[0]);
                        lgkm1<0>(F[1]);
                        lgkm1<0>(F[2]);
                        if constexpr (!LASTC) {
                            wait_vmc<6>();
                            __builtin_amdgcn_s_barrier();
                        }
                    } else {
                        lgkm1<2>(F[r]);                   // fragments k + 1 and k + 2 stay in flight
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (!LASTC) {
                        // DMA: piece f of the next chunk's halo at f = 0..4, a residual row behind each of the
                        // first four; the next chunk's tap rows as they die
                        if constexpr (dx == 0 && f < NRB) issueA(f, cn, (c + 1) & 1);
                        if constexpr (dx == 1 && f < 4) {
                            if (f < per && rnext < RR0) {
                                issueR(rnext);
                                ++rnext;
                            }
                        }
                        if constexpr (k == 3 * NF) loadW(cn, I0{});
                        if constexpr (k == LAST) loadW(cn, I1{});
                    } else {
                        // residual rows 10..14 in the halo's slots; the remainder plane where the tap rows die
                        if constexpr (dx == 0 && f < NF - RR0) {
                            if (resid) issueR(RR0 + f);
                        }
                        if constexpr (k == 3 * NF) {
                            if (resid) {
#pragma unroll
                                for (int i = 0; i < 12; ++i) loadQ(i);
                            }
                        }
                        if constexpr (k == LAST) {
                            if (resid) {
#pragma unroll
                                for (int i = 12; i < NF; ++i) loadQ(i);
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    static_for<0, 3>([&](auto dyc) {
                        constexpr int dy = decltype(dyc)::value, i = f - dy;
                        if constexpr (i >= 0 && i < NF) {
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                if constexpr (MODE == 2)
                                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(W[dy][dx][j], F[r], acc[i][j], 0, 0, 0);
                                else
                                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(W[dy][dx][j], F[r], acc[i][j], 0, 0, 0);
                            }
                        }
                    });
                    __builtin_amdgcn_sched_barrier(0);
                    // fragment k + 3 into the register just consumed; past the chunk's end the next
                    // chunk's first three (its halo is certified by the barrier above)
                    if constexpr (k + 3 < 3 * NFR) ds_rd<(16 * ((k + 3) / 3) + (k + 3) % 3) * 16>(F[r], a_cur);
                    else if constexpr (!LASTC) ds_rd<(k + 3 - 3 * NFR) * 16>(F[r], a_nxt);
                    __builtin_amdgcn_sched_barrier(0);
                });
                if constexpr (!LASTC) {
                    loadW(cn, I2{});
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            const int nloop = tail_old ? NCH : NCH - 1;
            for (int c = 0; c < nloop; ++c) chunk(c, std::false_type{});
            if (!tail_old) chunk(NCH - 1, std::true_type{});
            V7_STAMP(2);
            // drain: under flag 0x4000 the three fragment reads past the end and the reloaded weights are
            // still in flight; they must land before the epilogue reuses their registers
            // (tools/lds_hazards.py).  The wave's residual pieces and remainder loads land here too.
            lgkm1<0>(F[0]);
            lgkm1<0>(F[1]);
            lgkm1<0>(F[2]);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            // wave-uniform: the lean epilogue by what the launch has (a residual without a remainder
            // plane is launched by nobody and takes the shared epilogue, as flags 0x4000 / 0x8000 do)
            const bool rem = p.Cq != nullptr;
            if (tail_old) epilogue(acc, 0, n0 + wave * 32 + 4 * lg, res_mem);
            else if ((p.flags & CONV_F_V7_OLD_EPILOGUE) || (resid && !rem)) epilogue(acc, 0, n0 + wave * 32 + 4 * lg, res_lds);
            else if (resid) epilogue_rows(std::true_type{}, std::true_type{});
            else if (rem) epilogue_rows(std::false_type{}, std::true_type{});
            else epilogue_rows(std::false_type{}, std::false_type{});
#ifdef AZ_V7_STAMPS
            V7_STAMP(4);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            V7_STAMP(5);
#endif
            return;
        }
    }

    f32x4v acc[NI][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {                         // the bias seeds the accumulators
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + n0 + wn * 64 + j * 16 + 4 * (lane >> 4));
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i][j] = f32x4v{bv.x, bv.y, bv.z, bv.w};
    }

    // fragment addresses: activations (MFMA column operand) at halo row wm*WR + 16i + l16 + tap
    // shift, group l >> 4; weights (row operand) at channel wn*64 + 16j + l16, group l >> 4
    const uint32_t a_lane = lds_addr(abuf) + lg * (HROWS * 16) + (wm * WR + l16) * 16;
    const uint32_t b_lane = lds_addr(bbuf) + lg * (BNT * 16) + (wn * 64 + l16) * 16;
    uint32_t mbits = 0;                                   // DENSE: board-edge bits of the lane's NI pixels
    if constexpr (DENSE) {
#pragma unroll
        for (int f = 0; f < NI; ++f) {
            const int gq = tile * TM + wm * WR + f * 16 + l16;
            const int pix = gq % HW, y = pix / HB, x = pix - y * HB;
            mbits |= ((x == 0 ? 1u : 0u) | (x == HB - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == HB - 1 ? 8u : 0u)) << (4 * f);
        }
    }

    // prologue: halo of chunk 0, weights of taps 0..RG-1
#pragma unroll
    for (int j = 0; j < NRB; ++j) issueA(j, 0, 0);
#pragma unroll
    for (int s = 0; s < RG; ++s) issueB(s, s);
    wait_vm(2 * (RG - 1));                                // A(0), B(0) landed; B(1..RG-1) may fly
    __builtin_amdgcn_s_barrier();

    auto maskA = [&](frag (&a)[4], int half, int dy, int dx) {
        if constexpr (DENSE) {
            const uint32_t test = (dy == 0 ? 4u : dy == 2 ? 8u : 0u) | (dx == 0 ? 1u : dx == 2 ? 2u : 0u);
            if (test) {
#pragma unroll
                for (int i = 0; i < NA; ++i)
                    if (mbits & (test << (4 * (half * NA + i)))) a[i] = frag{};
            }
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // The main loop, compiled once per row half of the tile (WMC = wm, a wave-uniform branch): on the
    // SLIM grid the second half's 16th fragment (grid rows 240..255) holds no live output, so with
    // SKIP waves wm = 1 neither read nor multiply it -- 1/16 of the tile's MFMAs and fragment reads
    // (as conv3x3_v9x3's SKIP variant).  -DAZ_V7_NOSKIP builds the round-5 kernel (A/B measurement),
    // where those MFMAs run on all-zero halo rows.
    auto main_loop = [&](auto wmc) {
        constexpr int WMC = decltype(wmc)::value;
        constexpr int NI1 = (SKIP && WMC == 1) ? NA - 1 : NA;   // fragments of the second A set this wave computes
        frag alo[4], ahi[4], bw[2][4];
        // fragments of tap t (compile time) of the chunk in A buffer `ab`, weights in slot `bs`
        // SLIM without SKIP: the 16th fragment (rows 240..255, no live outputs) of the second row half
        // reads 16 rows further on, where every halo row of every tap is zero (rows >= 256: halo row Y >= 16)
        const uint32_t z16 = (SLIM && wm == 1) ? 16 * 16 : 0;
        auto loadA = [&](frag (&a)[4], uint32_t ab, auto tc, auto hc) {
            constexpr int t = decltype(tc)::value, half = decltype(hc)::value;
            constexpr int sh = (t / 3) * WG + (t % 3);
            static_for<0, NA>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (half == 1 && i >= NI1) return;
                else if constexpr (SLIM && half == 1 && i == 3) ds_rd<((half * NA + i) * 16 + sh) * 16>(a[i], ab + z16);
                else ds_rd<((half * NA + i) * 16 + sh) * 16>(a[i], ab);
            });
        };
        auto loadB = [&](frag (&b)[4], uint32_t bs) {
            static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                ds_rd<j * 256>(b[j], bs);
            });
        };
        auto mma = [&](const frag (&a)[4], const frag (&b)[4], auto hc) {
            constexpr int half = decltype(hc)::value, NIH = half == 1 ? NI1 : NA;
#pragma unroll
            for (int i = 0; i < NIH; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if constexpr (MODE == 2)
                        acc[half * NA + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[j], a[i], acc[half * NA + i][j], 0, 0, 0);
                    else
                        acc[half * NA + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[half * NA + i][j], 0, 0, 0);
                }
            }
        };
        // tap 0 of chunk 0
        loadB(bw[0], b_lane);
        loadA(alo, a_lane, I0{}, I0{});
        if constexpr (HALVES == 2) loadA(ahi, a_lane, I0{}, I1{});

        // Two chunks per iteration: 18 taps, the weight registers alternate by tap parity.  Every tap
        // issues the same DMA pieces (a halo piece at taps 0..4, two weight pieces), past the end as
        // harmless reloads into free buffers, so the vmcnt budget is a compile-time constant: the
        // weights of tap s+1 were issued in tap s-RG+1 (the prologue for s < RG-1), followed by the
        // pieces of the RG-2 taps after it.  Fragments are read one tap ahead, past the end from free buffers.
        for (int c2 = 0; c2 < NCH; c2 += 2) {
            static_for<0, 18>([&](auto tc18) {
                constexpr int T = decltype(tc18)::value;      // tap of the chunk pair
                constexpr int t = T % 9, cur = T & 1, nxt = cur ^ 1;
                constexpr int allow = RG == 4 ? (t >= 2 && t - 2 < NRB ? 1 : 0) + (t >= 1 && t - 1 < NRB ? 1 : 0) + 4
                                              : (t >= 1 && t - 1 < NRB ? 1 : 0) + 2;
                constexpr int NAF = NA + (HALVES - 1) * NI1;  // activation fragment reads per tap
                const int c = c2 + T / 9;
                const int s = 9 * c + t;
                if constexpr (DENSE) asm volatile("" : "+v"(mbits));   // keep the edge masks inside the loop (no SGPR hoisting)
                // the NAF youngest LDS reads are this tap's activation fragments: the weights of tap s
                // (read one tap ago) are in registers -- required before the barrier frees their slot
                lgkm<NAF>(bw[cur]);
                wait_vm(allow);                               // weights of tap s+1 (and at t == 8 the next halo) landed
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                // DMA for later taps: a halo piece of chunk c+1 at taps 0..NRB-1 (the last chunk reloads
                // itself into the free buffer), then the weights of tap s+RG (clamped to the last tap)
                if constexpr (t < NRB) issueA(t, c + 1 < NCH ? c + 1 : c, (c + 1) & 1);
                issueB(s + RG < NS ? s + RG : NS - 1, (s + RG) % RG);
                // weights of tap s+1 (certified by the barrier above)
                loadB(bw[nxt], b_lane + ((s + 1) % RG) * B_TAP);
                __builtin_amdgcn_sched_barrier(0);
                lgkm<(HALVES - 1) * NI1 + 4>(alo);            // activations of tap s, low half
                maskA(alo, 0, t / 3, t % 3);
                mma(alo, bw[cur], I0{});
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t an = a_lane + ((t == 8 ? c + 1 : c) & 1) * A_BUF;
                constexpr int tn = (t + 1) % 9;
                loadA(alo, an, std::integral_constant<int, tn>{}, I0{});
                if constexpr (HALVES == 2) {
                    lgkm<4 + NA>(ahi);                        // activations of tap s, high half
                    maskA(ahi, 1, t / 3, t % 3);
                    __builtin_amdgcn_sched_barrier(0);
                    mma(ahi, bw[cur], I1{});
                    __builtin_amdgcn_sched_barrier(0);
                    loadA(ahi, an, std::integral_constant<int, tn>{}, I1{});
                }
                __builtin_amdgcn_sched_barrier(0);
            });
        }
        // drain: the last tap's fragment reads (past the end) may still be in flight.  The compiler does
        // not see them, so without the fragments as operands of the wait it reuses their registers in
        // the epilogue, and a late LDS return overwrites a live value (seen as wrong outputs under LDS
        // contention: three blocks per CU, tools/lds_hazards.py)
        lgkm<0>(alo);
        if constexpr (HALVES == 2) lgkm<0>(ahi);
        lgkm<0>(bw[0]);
        lgkm<0>(bw[1]);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    };
    if constexpr (SKIP) {
        if (wm == 0) main_loop(I0{});
        else main_loop(I1{});
    } else {
        main_loop(I0{});
    }

    epilogue(acc, wm * WR, n0 + wn * 64 + 4 * lg, res_mem);
}

// conv3x3_v7x3: the fp32-faithful trunk conv (AZ_PREC_BF16X3) on the v7 tile.
//
// Every fp32 operand x is carried as two bf16 planes, hi = bf16(x) and lo = bf16(x - hi), each
// in the g8 layout (activations) or the chunk-blocked layout (weights), and a product is
// hi*hi + lo*hi + hi*lo: three v_mfma_f32_16x16x32_bf16 with fp32 accumulation (lo*lo, ~2^-18
// of the product, is dropped) -- the arithmetic of conv3x3_v4<0>, on v7's geometry:
//
//  * tile 256 output rows x 128 channels per 256-thread block, wave tile 128 x 64 (as v7);
//  * LDS 144 KB: the halo of a 32-channel chunk, hi and lo planes, double-buffered (2 x 40 KB),
//    and a 4-slot ring of per-tap weight tiles, hi and lo (4 x 16 KB) -- one block per CU.
//    A tap is 96 MFMAs per wave (3x v7's), so one wave per SIMD keeps the matrix pipe fed, and
//    every fragment of tap s+1 (24 ds_read_b128: weights hi/lo, both row halves hi/lo) is read
//    into a second register set during tap s's MFMAs, in three batches of 8 (each batch waits
//    for the previous one, which is long done by then: never more than 8 LDS reads in flight);
//  * MFMAs in six units of 16 (Bh*Ah, Bl*Ah, Bh*Al per row half): consecutive MFMAs never
//    share an accumulator, so no unit waits on the previous one's result;
//  * epilogue from registers: residual hi + lo joined in fp32, ReLU, re-split into hi / lo,
//    streaming stores.
// Input: p.Ahi / p.Alo (g8 hi / lo, both with zeroed tails at p.a_tail), p.Bblk / p.Bblk_lo,
// residual p.Rhi / p.Rlo (optional), output p.Chi / p.Clo.
template <int HB, int GEO, int PT>
__global__ __launch_bounds__(256, 1) void conv3x3_v7x3(ConvBf16Args p) {
    typedef Geom7<HB, GEO> GM;
    typedef H16<PT> H;
    constexpr bool DENSE = GM::DENSE, SLIM = GM::SLIM;
    typedef typename X3T<PT>::frag frag;
    constexpr int BNT = 128, WG = GM::WG, HW = GM::HW, HROWS = GM::HROWS;
    constexpr int A_PL = 4 * HROWS * 16;                  // one plane of a chunk's halo: 20 KB
    constexpr int A_BUF = 2 * A_PL;                       // hi + lo: 40 KB
    constexpr int B_PL = 4 * BNT * 16;                    // one plane of a tap's weights: 8 KB
    constexpr int B_TAP = 2 * B_PL;                       // hi + lo: 16 KB
    constexpr int LDS = 2 * A_BUF + 4 * B_TAP;            // 144 KB
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int nsplit = p.N / BNT;
    const int xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const int nb = slot % nsplit, tile = (slot / nsplit) * 8 + xcd;   // a tile's channel halves share an XCD
    const int n0 = nb * BNT;
    const int nboards = p.m_limit ? *p.m_limit : p.M / HW;
    if (DENSE ? tile * 256 >= nboards * HW : tile >= nboards) return;
    const int C = p.C, GI = C / 8, GO = p.N / 8;
    const int NCH = C / 32, NS = 9 * NCH;

    const uint32_t a_bytes = (uint32_t)p.a_tail, b_bytes = (uint32_t)((size_t)9 * C * p.N * 2);
    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Ahi, (short)0, (int)(a_bytes + AZ_ACT_TAIL * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsAl =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Alo, (short)0, (int)(a_bytes + AZ_ACT_TAIL * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.Bblk, (short)0, (int)b_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsBl =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Bblk_lo, (short)0, (int)b_bytes, 0x00020000);
    const uint32_t PAD = a_bytes;                         // zeroed tails: padding rows

    auto a_src = [&](int j, int ln) -> uint32_t {         // as conv3x3_v7: halo piece j of this wave
        const int q = wave + 4 * j, rb = q % 5, g = q / 5;
        const int hr = rb * 64 + ln;
        int Y, X, b;
        bool in;
        if constexpr (DENSE) {
            const int gpx = tile * 256 - (HB + 1) + hr;
            b = gpx >= 0 ? gpx / HW : -1;
            const int pix = gpx - b * HW;
            Y = pix / HB + 1; X = pix - (Y - 1) * HB + 1;
            in = hr < GM::TROWS && gpx >= 0;
        } else {
            Y = hr / WG; X = hr - Y * WG;
            b = tile;
            in = hr < GM::TROWS;
        }
        const bool ok = in && Y >= 1 && Y <= HB && X >= 1 && X <= HB && b < nboards;
        return ok ? (uint32_t)((((size_t)b * GI + g) * HW + (Y - 1) * HB + (X - 1)) * 16) : PAD;
    };
    int b_src[2], b_dst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wave + 4 * j, rb = q & 1, g = q >> 1;
        b_src[j] = (((g >> 1) * 18 + (g & 1)) * p.N + n0 + rb * 64) * 16;
        b_dst[j] = g * (BNT * 16) + rb * 1024;
    }
    const uint32_t lane16 = lane * 16;
    uint8_t* abuf = lds;
    uint8_t* bbuf = lds + 2 * A_BUF;
    auto issueA = [&](int j, int c, int buf) {            // piece j of chunk c's halo, hi and lo planes
        const int q = wave + 4 * j, rb = q % 5, g = q / 5;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t vo = a_src(j, ln);
        const int so = __builtin_amdgcn_readfirstlane(c * (4 * HW * 16));
        uint8_t* dst = abuf + buf * A_BUF + g * (HROWS * 16) + rb * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)dst, 16, (int)vo, so, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsAl, (lds_void_t*)(dst + A_PL), 16, (int)vo, so, 0, 0);
    };
    auto issueB = [&](int s, int slot) {                  // the wave's four pieces of tap s's weights
        const int c = s / 9, t = s - 9 * c;
        const int so = __builtin_amdgcn_readfirstlane((36 * c + 2 * t) * p.N * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            uint8_t* dst = bbuf + slot * B_TAP + b_dst[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)dst, 16, (int)lane16, so + b_src[j], 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBl, (lds_void_t*)(dst + B_PL), 16, (int)lane16, so + b_src[j], 0, 0);
        }
    };

    f32x4v acc[8][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + n0 + wn * 64 + j * 16 + 4 * (lane >> 4));
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i][j] = f32x4v{bv.x, bv.y, bv.z, bv.w};
    }

    const int l16 = lane & 15, lg = lane >> 4;
    const uint32_t a_lane = lds_addr(abuf) + lg * (HROWS * 16) + (wm * 128 + l16) * 16;
    const uint32_t b_lane = lds_addr(bbuf) + lg * (BNT * 16) + (wn * 64 + l16) * 16;
    uint32_t mbits = 0;
    if constexpr (DENSE) {
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int gq = tile * 256 + wm * 128 + f * 16 + l16;
            const int pix = gq % HW, y = pix / HB, x = pix - y * HB;
            mbits |= ((x == 0 ? 1u : 0u) | (x == HB - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == HB - 1 ? 8u : 0u)) << (4 * f);
        }
    }

    // prologue: halo of chunk 0 (hi + lo), weights of taps 0..3
#pragma unroll
    for (int j = 0; j < 5; ++j) issueA(j, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) issueB(s, s);
    wait_vm(12);                                          // A(0), B(0) landed; B(1..3) may fly
    __builtin_amdgcn_s_barrier();

    // fragment registers, double-buffered by tap parity: a[buf][row half][plane][i], bw[buf][plane][j]
    frag a[2][2][2][4], bw[2][2][4];
    auto maskA = [&](frag (&x)[4], int half, int dy, int dx) {
        if constexpr (DENSE) {
            const uint32_t test = (dy == 0 ? 4u : dy == 2 ? 8u : 0u) | (dx == 0 ? 1u : dx == 2 ? 2u : 0u);
            if (test) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (mbits & (test << (4 * (half * 4 + i)))) x[i] = frag{};
            }
        }
    };
    const uint32_t z16 = (SLIM && wm == 1) ? 16 * 16 : 0;  // SLIM: 16th fragment reads all-zero halo rows
    auto loadA = [&](frag (&x)[4], uint32_t ab, auto tc, auto hc, auto pc) {
        constexpr int t = decltype(tc)::value, half = decltype(hc)::value, pl = decltype(pc)::value;
        constexpr int sh = (t / 3) * WG + (t % 3);
        static_for<0, 4>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if constexpr (SLIM && half == 1 && i == 3) ds_rd<pl * A_PL + ((half * 4 + i) * 16 + sh) * 16>(x[i], ab + z16);
            else ds_rd<pl * A_PL + ((half * 4 + i) * 16 + sh) * 16>(x[i], ab);
        });
    };
    auto loadB = [&](frag (&x)[4], uint32_t bs, auto pc) {
        constexpr int pl = decltype(pc)::value;
        static_for<0, 4>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            ds_rd<pl * B_PL + j * 256>(x[j], bs);
        });
    };
    auto mma = [&](const frag (&x)[4], const frag (&b)[4], int half) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[half * 4 + i][j] = X3T<PT>::mma(b[j], x[i], acc[half * 4 + i][j]);
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // fragments of tap 0 of chunk 0, in batches of 8 LDS reads
    loadB(bw[0][0], b_lane, I0{});
    loadB(bw[0][1], b_lane, I1{});
    lgkm<0>(bw[0][0]);
    loadA(a[0][0][0], a_lane, I0{}, I0{}, I0{});
    loadA(a[0][0][1], a_lane, I0{}, I0{}, I1{});
    lgkm<0>(a[0][0][0]);
    loadA(a[0][1][0], a_lane, I0{}, I1{}, I0{});
    loadA(a[0][1][1], a_lane, I0{}, I1{}, I1{});

    // Two chunks per iteration (18 taps, register sets alternate by tap parity).  DMA as conv3x3_v7
    // with twice the pieces: a halo piece pair at taps 0..4, four weight pieces per tap; the weights
    // of tap s+1 were issued in tap s-3, followed by the pieces of taps s-2 and s-1.
    for (int c2 = 0; c2 < NCH; c2 += 2) {
        static_for<0, 18>([&](auto tc18) {
            constexpr int T = decltype(tc18)::value;
            constexpr int t = T % 9, cur = T & 1, nxt = cur ^ 1;
            constexpr int allow = 2 * (t >= 2 && t - 2 < 5 ? 1 : 0) + 2 * (t >= 1 && t - 1 < 5 ? 1 : 0) + 8;
            constexpr int tn = (t + 1) % 9;
            using TN = std::integral_constant<int, tn>;
            const int c = c2 + T / 9;
            const int s = 9 * c + t;
            if constexpr (DENSE) asm volatile("" : "+v"(mbits));
            // every fragment of tap s is in registers (the last batch was read before the previous
            // tap's last MFMA units): required before the barrier frees tap s's weight slot
            lgkm<0>(a[cur][1][0]);
            lgkm<0>(a[cur][1][1]);
            wait_vm(allow);                               // weights of tap s+1 (and at t == 8 the next halo) landed
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (t < 5) issueA(t, c + 1 < NCH ? c + 1 : c, (c + 1) & 1);
            issueB(s + 4 < NS ? s + 4 : NS - 1, (s + 4) & 3);
            // batch 1: the weights of tap s+1 (certified by the barrier above)
            const uint32_t bn = b_lane + ((s + 1) & 3) * B_TAP;
            loadB(bw[nxt][0], bn, I0{});
            loadB(bw[nxt][1], bn, I1{});
            __builtin_amdgcn_sched_barrier(0);
            maskA(a[cur][0][0], 0, t / 3, t % 3);
            maskA(a[cur][0][1], 0, t / 3, t % 3);
            mma(a[cur][0][0], bw[cur][0], 0);             // hi x hi, row half 0
            __builtin_amdgcn_sched_barrier(0);
            lgkm<0>(bw[nxt][0]);
            lgkm<0>(bw[nxt][1]);
            // batch 2: row half 0 of tap s+1
            const uint32_t an = a_lane + ((t == 8 ? c + 1 : c) & 1) * A_BUF;
            loadA(a[nxt][0][0], an, TN{}, I0{}, I0{});
            loadA(a[nxt][0][1], an, TN{}, I0{}, I1{});
            __builtin_amdgcn_sched_barrier(0);
            mma(a[cur][0][0], bw[cur][1], 0);             // hi(act) x lo(weights)
            __builtin_amdgcn_sched_barrier(0);
            mma(a[cur][0][1], bw[cur][0], 0);             // lo(act) x hi(weights)
            __builtin_amdgcn_sched_barrier(0);
            lgkm<0>(a[nxt][0][0]);
            lgkm<0>(a[nxt][0][1]);
            // batch 3: row half 1 of tap s+1
            loadA(a[nxt][1][0], an, TN{}, I1{}, I0{});
            loadA(a[nxt][1][1], an, TN{}, I1{}, I1{});
            __builtin_amdgcn_sched_barrier(0);
            maskA(a[cur][1][0], 1, t / 3, t % 3);
            maskA(a[cur][1][1], 1, t / 3, t % 3);
            mma(a[cur][1][0], bw[cur][0], 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a[cur][1][0], bw[cur][1], 1);
            __builtin_amdgcn_sched_barrier(0);
            mma(a[cur][1][1], bw[cur][0], 1);
            __builtin_amdgcn_sched_barrier(0);
        });
    }
    // drain with every fragment register as an operand (see conv3x3_v7)
#pragma unroll
    for (int k = 0; k < 8; ++k) lgkm<0>(a[k >> 2][(k >> 1) & 1][k & 1]);
#pragma unroll
    for (int k = 0; k < 4; ++k) lgkm<0>(bw[k >> 1][k & 1]);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    // epilogue from the accumulators: residual hi + lo joined in fp32, ReLU, split, streaming stores
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rhi, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rlo, (short)0, 0x7fffffff, 0x00020000);
    const int chl = n0 + wn * 64 + 4 * lg;
    float4 osc[4];                                        // PT 2: the weights' per-channel scale, undone
    if constexpr (PT == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) osc[j] = *reinterpret_cast<const float4*>(p.oscale + chl + j * 16);
    }
    float vmax = 0.0f;                                    // PT 2: fp16 range guard
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int q = wm * 128 + i * 16 + l16;
        int b, pix;
        bool live;
        if constexpr (DENSE) {
            const int gq = tile * 256 + q;
            b = gq / HW;
            pix = gq - b * HW;
            live = b < nboards;
        } else {
            const int y = q / WG, x = q - y * WG;
            b = tile;
            pix = y * HB + x;
            live = y < HB && x < HB;
        }
        if (!live) continue;
        u32x2_t hv[4], lv[4];
        if (p.Rhi) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ch = chl + j * 16;
                const size_t e = (((size_t)b * GO + (ch >> 3)) * HW + pix) * 8 + (ch & 7);
                hv[j] = __builtin_amdgcn_raw_buffer_load_b64(rh, (int)(e * 2), 0, AZ_RES_AUX);
                lv[j] = __builtin_amdgcn_raw_buffer_load_b64(rl, (int)(e * 2), 0, AZ_RES_AUX);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ch = chl + j * 16;
            const size_t e = (((size_t)b * GO + (ch >> 3)) * HW + pix) * 8 + (ch & 7);
            float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if constexpr (PT == 2) {
                o[0] *= osc[j].x; o[1] *= osc[j].y; o[2] *= osc[j].z; o[3] *= osc[j].w;
            }
            if (p.Rhi) {
                uint16_t hh[4], ll[4];
                __builtin_memcpy(hh, &hv[j], 8);
                __builtin_memcpy(ll, &lv[j], 8);
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] += H::to_f(hh[k]) + H::to_f(ll[k]);
            }
            uint16_t oh[4], ol[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[k] = __builtin_amdgcn_fmed3f(o[k], 0.0f, 3.0e38f);   // ReLU
                if constexpr (PT == 2) vmax = fmaxf(vmax, o[k]);
                oh[k] = H::from_f(o[k]);
                ol[k] = H::from_f(o[k] - H::to_f(oh[k]));
            }
            u32x2_t hs, ls;
            __builtin_memcpy(&hs, oh, 8);
            __builtin_memcpy(&ls, ol, 8);
            asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p.Chi + e), "v"(hs) : "memory");
            asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p.Clo + e), "v"(ls) : "memory");
        }
    }
    if (PT == 2 && !(vmax <= 65504.0f) && p.ovf) atomicOr(p.ovf, 1);    // fp16 pieces: the engine fails the forward
}

// conv3x3_v9x3: the fp32-faithful trunk conv on a full-width tile (the default for AZ_PREC_BF16X3
// at N % 256 == 0; conv3x3_v7x3 above is the A/B reference).
//
// Same operands and arithmetic as conv3x3_v7x3 -- every accumulator receives, per tap, Bh*Ah,
// then Bl*Ah, then Bh*Al, so the two kernels are bitwise equal -- on a different shape of work:
//
//  * ONE 512-thread block per CU (8 waves, two per SIMD: waves w and w + 4 share one) owns a
//    256-row tile x ALL 256 output channels (wave tile 128 rows x 64 channels, as v7x3).  The halo
//    is fetched once per tile, not once per channel half (v7x3 reads it twice: 1.36x algorithmic
//    HBM), and a SIMD's two waves hide each other's LDS-DMA issue (~60 cycles a piece), fragment
//    reads and barrier skew -- with v7x3's one wave per SIMD the matrix pipe idles through them;
//  * LDS 144 KB: the 32-channel halo chunk, hi + lo, double-buffered (2 x 40 KB) and a 2-slot
//    ring of per-tap weight tiles, hi + lo for 256 channels (2 x 32 KB).  Tap s's barrier certifies
//    tap s+1's weights (issued one tap earlier) and frees tap s's slot for tap s+2;
//  * a tap is four MFMA units per wave -- U0 Ah(rows 0-63 of the wave) x {Bh, Bl}, U1 Al x Bh,
//    U2 Ah(rows 64-127) x {Bh, Bl}, U3 Al x Bh -- over two 4-fragment activation register sets:
//    the next unit's fragments are read during the current one, and the next tap's weights are
//    read fragment by fragment as U2 / U3 release them (64 fragment VGPRs + 128 accumulators:
//    two waves per SIMD fit the register file);
//  * epilogue from registers as v7x3.
template <int HB, int GEO, int VAR, int PT>
__global__ __launch_bounds__(512, 1) void conv3x3_v9x3(ConvBf16Args p) {
    constexpr bool MID = VAR & 1;                         // the tap barrier after unit U0 (else at the tap start)
    constexpr bool SKIP = (VAR & 2) && GEO == GEO_SLIM;   // waves 4-7 skip the SLIM tile's dead 16th fragment
    typedef Geom7<HB, GEO> GM;
    typedef H16<PT> H;
    constexpr bool DENSE = GM::DENSE, SLIM = GM::SLIM;
    typedef typename X3T<PT>::frag frag;
    constexpr int BNT = 256, WG = GM::WG, HW = GM::HW, HROWS = GM::HROWS;
    constexpr int A_PL = 4 * HROWS * 16;                  // one plane of a chunk's halo: 20 KB
    constexpr int A_BUF = 2 * A_PL;                       // hi + lo: 40 KB
    constexpr int B_PL = 4 * BNT * 16;                    // one plane of a tap's weights: 16 KB
    constexpr int B_TAP = 2 * B_PL;                       // hi + lo: 32 KB
    constexpr int LDS = 2 * A_BUF + 2 * B_TAP;            // 144 KB
    __shared__ __attribute__((aligned(16))) uint8_t lds[LDS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;             // 128 pixels x 64 channels per wave
    const int nsplit = p.N / BNT;
    const int nb = blockIdx.x % nsplit, tile = blockIdx.x / nsplit;
    const int n0 = nb * BNT;
    const int nboards = p.m_limit ? *p.m_limit : p.M / HW;
    if (DENSE ? tile * 256 >= nboards * HW : tile >= nboards) return;
    // First-round stagger: the blocks of a launch run in lockstep rounds (one per CU, identical
    // work), so every CU reaches its epilogue at once and the epilogues' stores (and the second
    // conv's residual reads) saturate HBM together (tools/v9_stamps.py: 22 us of a 148 us block).
    // Offsetting the first round's starts over p.stagger ns keeps the CUs out of phase for the
    // whole launch, and each epilogue overlaps other CUs' main loops.
    if (p.stagger > 0 && blockIdx.x < 256) {
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        const uint64_t wait = (uint64_t)(((blockIdx.x * 37u) & 63u) * (uint32_t)p.stagger) / 640u;   // 10 ns ticks
        while (__builtin_amdgcn_s_memrealtime() - t0 < wait) __builtin_amdgcn_s_sleep(4);
    }
    V9_STAMP(0);
    const int C = p.C, GI = C / 8, GO = p.N / 8;
    const int NCH = C / 32, NS = 9 * NCH;

    const uint32_t a_bytes = (uint32_t)p.a_tail, b_bytes = (uint32_t)((size_t)9 * C * p.N * 2);
    const __amdgpu_buffer_rsrc_t rsA =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Ahi, (short)0, (int)(a_bytes + AZ_ACT_TAIL * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsAl =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Alo, (short)0, (int)(a_bytes + AZ_ACT_TAIL * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc((void*)p.Bblk, (short)0, (int)b_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsBl =
        __builtin_amdgcn_make_buffer_rsrc((void*)p.Bblk_lo, (short)0, (int)b_bytes, 0x00020000);
    const uint32_t PAD = a_bytes;                         // zeroed tails: padding rows

    // halo piece pair q (hi + lo) = (8-channel group g = q / 5, 64-row block rb = q % 5): 20 pairs
    // per chunk, pair q = wave + 8j issued at tap j of the previous chunk (j = 0..2, q < 20)
    auto a_src = [&](int q, int ln) -> uint32_t {
        const int rb = q % 5, g = q / 5;
        const int hr = rb * 64 + ln;
        int Y, X, b;
        bool in;
        if constexpr (DENSE) {
            const int gpx = tile * 256 - (HB + 1) + hr;
            b = gpx >= 0 ? gpx / HW : -1;
            const int pix = gpx - b * HW;
            Y = pix / HB + 1; X = pix - (Y - 1) * HB + 1;
            in = hr < GM::TROWS && gpx >= 0;
        } else {
            Y = hr / WG; X = hr - Y * WG;
            b = tile;
            in = hr < GM::TROWS;
        }
        const bool ok = in && Y >= 1 && Y <= HB && X >= 1 && X <= HB && b < nboards;
        return ok ? (uint32_t)((((size_t)b * GI + g) * HW + (Y - 1) * HB + (X - 1)) * 16) : PAD;
    };
    // weight pieces of a tap, per plane 16 (group g = q >> 2, 64-channel block rb = q & 3): q = wave + 8j
    int b_src[2], b_dst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = wave + 8 * j, rb = q & 3, g = q >> 2;
        b_src[j] = (((g >> 1) * 18 + (g & 1)) * p.N + n0 + rb * 64) * 16;
        b_dst[j] = g * (BNT * 16) + rb * 1024;
    }
    const uint32_t lane16 = lane * 16;
    uint8_t* abuf = lds;
    uint8_t* bbuf = lds + 2 * A_BUF;
    auto issueA = [&](int j, int c, int buf) {            // pair j of this wave for chunk c's halo
        const int q = wave + 8 * j;
        if (q >= 20) return;                              // wave-uniform
        const int rb = q % 5, g = q / 5;
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const uint32_t vo = a_src(q, ln);
        const int so = __builtin_amdgcn_readfirstlane(c * (4 * HW * 16));
        uint8_t* dst = abuf + buf * A_BUF + g * (HROWS * 16) + rb * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t*)dst, 16, (int)vo, so, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsAl, (lds_void_t*)(dst + A_PL), 16, (int)vo, so, 0, 0);
    };
    auto issueB = [&](int s, int slot) {                  // the wave's four pieces of tap s's weights
        const int c = s / 9, t = s - 9 * c;
        const int so = __builtin_amdgcn_readfirstlane((36 * c + 2 * t) * p.N * 16);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            uint8_t* dst = bbuf + slot * B_TAP + b_dst[j];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void_t*)dst, 16, (int)lane16, so + b_src[j], 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsBl, (lds_void_t*)(dst + B_PL), 16, (int)lane16, so + b_src[j], 0, 0);
        }
    };

    f32x4v acc[8][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + n0 + wn * 64 + j * 16 + 4 * (lane >> 4));
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i][j] = f32x4v{bv.x, bv.y, bv.z, bv.w};
    }

    const int l16 = lane & 15, lg = lane >> 4;
    const uint32_t a_lane = lds_addr(abuf) + lg * (HROWS * 16) + (wm * 128 + l16) * 16;
    const uint32_t b_lane = lds_addr(bbuf) + lg * (BNT * 16) + (wn * 64 + l16) * 16;
    uint32_t mbits = 0;
    if constexpr (DENSE) {
#pragma unroll
        for (int f = 0; f < 8; ++f) {
            const int gq = tile * 256 + wm * 128 + f * 16 + l16;
            const int pix = gq % HW, y = pix / HB, x = pix - y * HB;
            mbits |= ((x == 0 ? 1u : 0u) | (x == HB - 1 ? 2u : 0u) | (y == 0 ? 4u : 0u) | (y == HB - 1 ? 8u : 0u)) << (4 * f);
        }
    }

    // prologue: halo of chunk 0 (hi + lo), weights of taps 0 and 1
#pragma unroll
    for (int j = 0; j < 3; ++j) issueA(j, 0, 0);
    issueB(0, 0);
    issueB(1, 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    V9_STAMP(1);

    frag aX[4], aY[4], bh[4], bl[4];
    auto maskA = [&](frag (&x)[4], int half, int dy, int dx) {
        if constexpr (DENSE) {
            const uint32_t test = (dy == 0 ? 4u : dy == 2 ? 8u : 0u) | (dx == 0 ? 1u : dx == 2 ? 2u : 0u);
            if (test) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (mbits & (test << (4 * (half * 4 + i)))) x[i] = frag{};
            }
        }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // The main loop, compiled once per row half of the tile (WMC = wm): with SKIP the second half
    // (waves 4-7) neither reads nor multiplies its 16th fragment, whose rows hold no live outputs
    // on the SLIM grid -- 1/16 of a SIMD's MFMAs saved without a branch inside the loop.
    auto main_loop = [&](auto wmc) {
        constexpr int WMC = decltype(wmc)::value;
        constexpr int NI1 = (SKIP && WMC == 1) ? 3 : 4;  // fragments of row half 1 this wave computes
        const uint32_t z16 = (SLIM && wm == 1) ? 16 * 16 : 0;    // SLIM: 16th fragment reads all-zero halo rows
        auto loadA = [&](frag (&x)[4], uint32_t ab, auto tc, auto hc, auto pc) {
            constexpr int t = decltype(tc)::value, half = decltype(hc)::value, pl = decltype(pc)::value;
            constexpr int sh = (t / 3) * WG + (t % 3);
            static_for<0, 4>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                if constexpr (half == 1 && i >= NI1) return;
                else if constexpr (SLIM && half == 1 && i == 3) ds_rd<pl * A_PL + ((half * 4 + i) * 16 + sh) * 16>(x[i], ab + z16);
                else ds_rd<pl * A_PL + ((half * 4 + i) * 16 + sh) * 16>(x[i], ab);
            });
        };
        auto loadB = [&](frag (&x)[4], uint32_t bs, auto pc) {
            constexpr int pl = decltype(pc)::value;
            static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                ds_rd<pl * B_PL + j * 256>(x[j], bs);
            });
        };
        auto mma = [&](const frag (&x)[4], const frag (&b)[4], auto hc) {
            constexpr int half = decltype(hc)::value, NI = half == 1 ? NI1 : 4;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[half * 4 + i][j] = X3T<PT>::mma(b[j], x[i], acc[half * 4 + i][j]);
            }
        };
        // row half 1 with the weights b, j-major: after fragment j's MFMAs, b[j] is reloaded with
        // plane pl of the next tap's weights (at bn)
        auto mma_reload = [&](const frag (&x)[4], frag (&b)[4], uint32_t bn, auto pc) {
            constexpr int pl = decltype(pc)::value;
            static_for<0, 4>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
#pragma unroll
                for (int i = 0; i < NI1; ++i)
                    acc[4 + i][j] = X3T<PT>::mma(b[j], x[i], acc[4 + i][j]);
                __builtin_amdgcn_sched_barrier(0);
                ds_rd<pl * B_PL + j * 256>(b[j], bn);
                __builtin_amdgcn_sched_barrier(0);
            });
        };
        // the tap's DMA: a halo piece pair of chunk c+1 at t < 3 (the last chunk reloads itself into
        // the free buffer) and the weights of tap s+2 (clamped) into tap s's slot
        auto dma = [&](int t, int c, int s) {
            if (t < 3) issueA(t, c + 1 < NCH ? c + 1 : c, (c + 1) & 1);
            issueB(s + 2 < NS ? s + 2 : NS - 1, s & 1);
        };
        loadB(bh, b_lane, I0{});
        loadB(bl, b_lane, I1{});
        loadA(aX, a_lane, I0{}, I0{}, I0{});

        for (int c2 = 0; c2 < NCH; c2 += 2) {
            static_for<0, 18>([&](auto tc18) {
                constexpr int T = decltype(tc18)::value;
                constexpr int t = T % 9, tn = (t + 1) % 9;
                using TC = std::integral_constant<int, t>;
                using TN = std::integral_constant<int, tn>;
                const int c = c2 + T / 9;
                const int s = 9 * c + t;
                if constexpr (DENSE) asm volatile("" : "+v"(mbits));
                // tap s's weights and U0's fragments are in registers
                lgkm<0>(aX);
                lgkm<0>(bh);
                lgkm<0>(bl);
                if constexpr (!MID) {
                    // barrier at the tap start: tap s's weight reads are done (its slot may take tap
                    // s+2), tap s+1's weights (and at t == 8 the next halo) landed in every wave
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    dma(t, c, s);
                }
                const uint32_t ac = a_lane + (c & 1) * A_BUF;
                loadA(aY, ac, TC{}, I0{}, I1{});          // U1: lo, row half 0
                __builtin_amdgcn_sched_barrier(0);
                maskA(aX, 0, t / 3, t % 3);
                mma(aX, bh, I0{});                        // U0: hi x hi, hi(act) x lo(weights)
                __builtin_amdgcn_sched_barrier(0);
                mma(aX, bl, I0{});
                __builtin_amdgcn_sched_barrier(0);
                lgkm<0>(aY);
                if constexpr (MID) {
                    // barrier after U0: every wave's reads of tap s's weights (issued at the end of
                    // tap s-1) have completed behind U0's MFMAs, so tap s's slot may take tap s+2;
                    // tap s+1's weights (and at t == 8 the next halo) landed in every wave
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    dma(t, c, s);
                }
                loadA(aX, ac, TC{}, I1{}, I0{});          // U2: hi, row half 1
                __builtin_amdgcn_sched_barrier(0);
                maskA(aY, 0, t / 3, t % 3);
                mma(aY, bh, I0{});                        // U1: lo(act) x hi(weights)
                __builtin_amdgcn_sched_barrier(0);
                lgkm<0>(aX);
                loadA(aY, ac, TC{}, I1{}, I1{});          // U3: lo, row half 1
                __builtin_amdgcn_sched_barrier(0);
                maskA(aX, 1, t / 3, t % 3);
                mma(aX, bh, I1{});                        // U2
                __builtin_amdgcn_sched_barrier(0);
                const uint32_t bn = b_lane + ((s + 1) & 1) * B_TAP;
                mma_reload(aX, bl, bn, I1{});             // U2, releasing bl to tap s+1
                if constexpr (NI1 == 4) lgkm<4>(aY);      // U3's fragments (the 4 weight reads may fly)
                else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(aY[0]), "+v"(aY[1]), "+v"(aY[2]) :: "memory");
                const uint32_t an = a_lane + ((t == 8 ? c + 1 : c) & 1) * A_BUF;
                loadA(aX, an, TN{}, I0{}, I0{});          // next tap's U0
                __builtin_amdgcn_sched_barrier(0);
                maskA(aY, 1, t / 3, t % 3);
                mma_reload(aY, bh, bn, I0{});             // U3, releasing bh to tap s+1
            });
        }
        // drain with every fragment register as an operand (see conv3x3_v7): the next tap's reads
        // past the end are in flight, and the two row-half branches' registers merge after this
        lgkm<0>(aX);
        lgkm<0>(aY);
        lgkm<0>(bh);
        lgkm<0>(bl);
    };
    if (SKIP && wm == 1) main_loop(I1{});
    else main_loop(I0{});
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    V9_STAMP(2);

    // epilogue from the accumulators: residual hi + lo joined in fp32, ReLU, split, streaming stores.
    // The residual of row fragments 0-3 is loaded in one burst, then 4-7 once 0-3 are stored (their
    // accumulators and residual registers free): two memory round trips per wave, not eight.
    const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rhi, (short)0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc((void*)p.Rlo, (short)0, 0x7fffffff, 0x00020000);
    const int chl = n0 + wn * 64 + 4 * lg;
    float4 osc[4];                                        // PT 2: the weights' per-channel scale, undone
    if constexpr (PT == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) osc[j] = *reinterpret_cast<const float4*>(p.oscale + chl + j * 16);
    }
    float vmax = 0.0f;                                    // PT 2: fp16 range guard
    auto row_of = [&](int i, int& b, int& pix) -> bool {  // output row of fragment i of this lane
        const int q = wm * 128 + i * 16 + l16;
        if constexpr (DENSE) {
            const int gq = tile * 256 + q;
            b = gq / HW;
            pix = gq - b * HW;
            return b < nboards;
        } else {
            const int y = q / WG, x = q - y * WG;
            b = tile;
            pix = y * HB + x;
            return y < HB && x < HB;
        }
    };
    u32x2_t hv[4][4], lv[4][4];
    auto load_res = [&](auto i0c) {
        constexpr int i0 = decltype(i0c)::value;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            int b, pix;
            if (!row_of(i0 + ii, b, pix)) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ch = chl + j * 16;
                const size_t e = (((size_t)b * GO + (ch >> 3)) * HW + pix) * 8 + (ch & 7);
                hv[ii][j] = __builtin_amdgcn_raw_buffer_load_b64(rh, (int)(e * 2), 0, AZ_RES_AUX);
                lv[ii][j] = __builtin_amdgcn_raw_buffer_load_b64(rl, (int)(e * 2), 0, AZ_RES_AUX);
            }
        }
    };
    auto finish = [&](auto i0c) {
        constexpr int i0 = decltype(i0c)::value;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int i = i0 + ii;
            int b, pix;
            if (!row_of(i, b, pix)) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ch = chl + j * 16;
                const size_t e = (((size_t)b * GO + (ch >> 3)) * HW + pix) * 8 + (ch & 7);
                float o[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
                if constexpr (PT == 2) {
                    o[0] *= osc[j].x; o[1] *= osc[j].y; o[2] *= osc[j].z; o[3] *= osc[j].w;
                }
                if (p.Rhi) {
                    uint16_t hh[4], ll[4];
                    __builtin_memcpy(hh, &hv[ii][j], 8);
                    __builtin_memcpy(ll, &lv[ii][j], 8);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] += H::to_f(hh[k]) + H::to_f(ll[k]);
                }
                uint16_t oh[4], ol[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    o[k] = __builtin_amdgcn_fmed3f(o[k], 0.0f, 3.0e38f);   // ReLU
                    if constexpr (PT == 2) vmax = fmaxf(vmax, o[k]);
                    oh[k] = H::from_f(o[k]);
                    ol[k] = H::from_f(o[k] - H::to_f(oh[k]));
                }
                u32x2_t hs, ls;
                __builtin_memcpy(&hs, oh, 8);
                __builtin_memcpy(&ls, ol, 8);
                asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p.Chi + e), "v"(hs) : "memory");
                asm volatile("global_store_dwordx2 %0, %1, off nt" ::"v"(p.Clo + e), "v"(ls) : "memory");
            }
        }
    };
    using I4 = std::integral_constant<int, 4>;
    if (p.Rhi) load_res(I0{});
    finish(I0{});
    if (p.Rhi) load_res(I4{});
    finish(I4{});
#ifdef AZ_V9_STAMPS
    V9_STAMP(3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    V9_STAMP(4);
#endif
    if (PT == 2 && !(vmax <= 65504.0f) && p.ovf) atomicOr(p.ovf, 1);    // fp16 pieces: the engine fails the forward
}

// Host side ----------------------------------------------------------------------------------
// diagnostic: select the stamped conv3x3_v9x3 launch / read its stamps (AZ_V9_STAMPS builds; else -1)
extern "C" int az_diag_v9_stamps(int sel, unsigned long long* st, unsigned* hw, int n) {
#ifdef AZ_V9_STAMPS
    if (sel >= -1) {
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_v9_sel), &sel, sizeof(int)) != hipSuccess) return -2;
        static unsigned long long zero[V9_MAXB][5];
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_v9_st), zero, sizeof(zero)) != hipSuccess) return -2;
    }
    if (st && n > 0) {
        n = n < V9_MAXB ? n : V9_MAXB;
        if (hipDeviceSynchronize() != hipSuccess) return -2;
        if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_v9_st), (size_t)n * 5 * 8) != hipSuccess) return -2;
        if (hw && hipMemcpyFromSymbol(hw, HIP_SYMBOL(g_v9_hw), (size_t)n * 2 * 4) != hipSuccess) return -2;
    }
    return 0;
#else
    (void)sel; (void)st; (void)hw; (void)n;
    return -1;
#endif
}

// diagnostic: select the stamped conv3x3_v7 launch / read its stamps (AZ_V7_STAMPS builds; else -1)
extern "C" int az_diag_v7_stamps(int sel, unsigned long long* st, unsigned* hw, int n) {
#ifdef AZ_V7_STAMPS
    if (sel >= -1) {
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_v7_sel), &sel, sizeof(int)) != hipSuccess) return -2;
        static unsigned long long zero[V7_MAXB][V7_NST];
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_v7_st), zero, sizeof(zero)) != hipSuccess) return -2;
    }
    if (st && n > 0) {
        n = n < V7_MAXB ? n : V7_MAXB;
        if (hipDeviceSynchronize() != hipSuccess) return -2;
        if (hipMemcpyFromSymbol(st, HIP_SYMBOL(g_v7_st), (size_t)n * V7_NST * 8) != hipSuccess) return -2;
        if (hw && hipMemcpyFromSymbol(hw, HIP_SYMBOL(g_v7_hw), (size_t)n * 2 * 4) != hipSuccess) return -2;
    }
    return 0;
#else
    (void)sel; (void)st; (void)hw; (void)n;
    return -1;
#endif
}

// Executing a plan (conv_plan.h): each helper maps the plan's runtime fields to the one instantiation
// they name and launches it on the plan's grid; a combination without an instantiation is an error.
template <int HB, int GEO, int TM = 256, int RG = 4>
static int v7_launch_g(const ConvPlan& p, const ConvBf16Args& a, hipStream_t st) {
    if (p.mode == 2) hipLaunchKernelGGL((conv3x3_v7<2, HB, GEO, TM, RG>), dim3(p.grid), dim3(p.block), 0, st, a);
    else if (p.mode == 1) hipLaunchKernelGGL((conv3x3_v7<1, HB, GEO, TM, RG>), dim3(p.grid), dim3(p.block), 0, st, a);
    else return -1;
    return 0;
}
// conv3x3_v7 of one board: DENSE tiles of 256 / 192 rows on the 4-slot ring, of 128 / 64 rows on
// either ring; 15x15 has the PAD and SLIM tiles besides
template <int HB>
static int v7_launch(const ConvPlan& p, const ConvBf16Args& a, hipStream_t st) {
    if (p.geo == GEO_DENSE) {
        switch (p.tm * 10 + p.ring) {
            case 643: return v7_launch_g<HB, GEO_DENSE, 64, 3>(p, a, st);
            case 644: return v7_launch_g<HB, GEO_DENSE, 64>(p, a, st);
            case 1283: return v7_launch_g<HB, GEO_DENSE, 128, 3>(p, a, st);
            case 1284: return v7_launch_g<HB, GEO_DENSE, 128>(p, a, st);
            case 1924: return v7_launch_g<HB, GEO_DENSE, 192>(p, a, st);
            case 2564: return v7_launch_g<HB, GEO_DENSE, 256>(p, a, st);
            default: return -1;
        }
    }
    if constexpr (HB == 15) {
        if (p.tm == 256 && p.ring == 4 && p.geo == GEO_PAD) return v7_launch_g<15, GEO_PAD>(p, a, st);
        if (p.tm == 256 && p.ring == 4 && p.geo == GEO_SLIM) return v7_launch_g<15, GEO_SLIM>(p, a, st);
    }
    return -1;
}

template <int HB, int GEO>
static int v7x3_launch_g(const ConvPlan& p, const ConvBf16Args& a, hipStream_t st) {
    if (p.pt == 2) hipLaunchKernelGGL((conv3x3_v7x3<HB, GEO, 2>), dim3(p.grid), dim3(p.block), 0, st, a);
    else hipLaunchKernelGGL((conv3x3_v7x3<HB, GEO, 1>), dim3(p.grid), dim3(p.block), 0, st, a);
    return 0;
}

// first-round stagger (ns; az_diag_set_v9_stagger): 32 us measured best of 0 / 8 / 16 / 32 / 64 us,
// -0.8 % per C3 launch, -0.7 % C4 (profiles/r04_v9x3_stagger.txt); on the launches the plan names
static int g_v9_stagger = 32000;
extern "C" int az_diag_set_v9_stagger(int ns) { g_v9_stagger = ns; return 0; }
template <int HB, int GEO>
static int v9x3_launch_g(const ConvPlan& p, const ConvBf16Args& a, hipStream_t st) {
    const dim3 grid(p.grid), block(p.block);
    ConvBf16Args b = a;
    b.stagger = p.stagger ? g_v9_stagger : 0;
    if (p.pt == 2) {
        if (p.var != 3) return -1;
        hipLaunchKernelGGL((conv3x3_v9x3<HB, GEO, 3, 2>), grid, block, 0, st, b);
        return 0;
    }
    switch (p.var) {
        case 0: hipLaunchKernelGGL((conv3x3_v9x3<HB, GEO, 0, 1>), grid, block, 0, st, b); return 0;
        case 1: hipLaunchKernelGGL((conv3x3_v9x3<HB, GEO, 1, 1>), grid, block, 0, st, b); return 0;
        case 2: hipLaunchKernelGGL((conv3x3_v9x3<HB, GEO, 2, 1>), grid, block, 0, st, b); return 0;
        case 3: hipLaunchKernelGGL((conv3x3_v9x3<HB, GEO, 3, 1>), grid, block, 0, st, b); return 0;
        default: return -1;
    }
}

// az_conv_launch's half for the kernels of this file (CONV_V7 / CONV_V7X3 / CONV_V9X3)
int az_conv_launch_v7(const ConvPlan& p, const ConvBf16Args& a, hipStream_t st) {
    return az_conv_board_dispatch(p.board, [&](auto hb) -> int {
        constexpr int HB = decltype(hb)::value;
        constexpr int GEO_X3 = HB == 15 ? GEO_SLIM : GEO_DENSE;   // the x3 kernels' one tile per board
        switch (p.kernel) {
            case CONV_V7: return v7_launch<HB>(p, a, st);
            case CONV_V7X3: return p.geo == GEO_X3 && p.tm == 256 ? v7x3_launch_g<HB, GEO_X3>(p, a, st) : -1;
            case CONV_V9X3: return p.geo == GEO_X3 && p.tm == 256 ? v9x3_launch_g<HB, GEO_X3>(p, a, st) : -1;
            default: return -1;
        }
    });
}
