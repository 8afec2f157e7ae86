// weight_pack_dev.h -- the device side of the weight packing (weight_pack.hip): launchers of the
// kernels that turn a parameter blob in device memory into the kernels' weight layouts, stream-ordered
// and without host work per element.  The element arithmetic and the layouts are weight_pack.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace wpdev {

// conv + BN (eval) of one layer: w [co][ci][taps] (+ cb, g, be, mu, var [co]) -> W [co][taps][cpad]
// (channels ci .. cpad-1 zero) and b [co].  g == nullptr: no BN -- W is the permuted w (wpack::fc_perm
// with ci = hc, taps = pp, cpad = hc) and b is not written.
struct Fold {
    const float *w, *cb, *g, *be, *mu, *var;
    int co, ci, taps, cpad;
    float *W, *b;
};
hipError_t fold(hipStream_t st, const Fold& f);

// Every piece set made from the rows of one folded layer W [N][taps * C] (bias b [N]); each output is
// optional (null: not written).
struct Rows {
    const float *W, *b;
    int N, taps, C;
    uint16_t *hi, *lo, *h16, *fh, *fl;                   // row-major, as W: bf16 hi / lo, fp16, scaled fp16 hi / lo
    uint16_t *bk_bf, *bk_h, *bk_lo, *bk_fh, *bk_fl;      // the same five chunk-blocked (taps == 9, C % 16 == 0)
    float *bx, *sx;                                      // [N]: b * 2^s, 2^-s
    // k_smallnet sets (taps == 9, N == F, C % 8 == 0): layer sm_l of [layer][tap][n][c] over F channels,
    // channels C .. F-1 zero; sm_w plain, the other five fragment-major; sm_b / sm_bx / sm_sx [layer][F]
    uint16_t *sm_w, *sm_wf, *sm_xh, *sm_xl, *sm_fh, *sm_fl;
    float *sm_b, *sm_bx, *sm_sx;
    int sm_l, F;
};
hipError_t rows(hipStream_t st, const Rows& r);

hipError_t copy_f32(hipStream_t st, const float* src, float* dst, size_t n);
hipError_t fill_u16(hipStream_t st, uint16_t* dst, size_t n, uint16_t v);
hipError_t fill_f32(hipStream_t st, float* dst, size_t n, float v);

}  // namespace wpdev
