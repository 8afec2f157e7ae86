// weight_pack.h -- the arithmetic that turns a parameter blob into the kernels' weight layouts:
// batch-norm folding, the 16-bit conversions and hi / lo splits, the per-row power-of-two scaling of
// the fp16 pieces (AZ_PREC_F16X3) and the layout permutations.  The element functions (WP_HD) are one
// source for the host loops below (az_net_load_weights) and for the device kernels of weight_pack.hip
// (az_net_load_weights_device), whose buffers are compared byte for byte.  Plain C++ without hipcc
// (WP_HD is then empty; net_load.hip keeps the allocations and uploads), so
// tests/test_weight_pack_cpu.py checks every output bit for bit without a device.  Compile with
// -ffp-contract=off -fno-fast-math: the results are compared bitwise.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define WP_HD __host__ __device__
#else
#define WP_HD
#endif

namespace wpack {

struct ParamCursor {
    const float* p; size_t off = 0;
    const float* take(size_t n) { const float* r = p + off; off += n; return r; }
};

// ---- element arithmetic, host and device
WP_HD inline uint32_t f2u(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
WP_HD inline float u2f(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

WP_HD inline uint16_t f2bf(float f) {   // round to nearest even
    uint32_t u = f2u(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
WP_HD inline float bf2f(uint16_t h) { return u2f((uint32_t)h << 16); }

// conv + BN (eval): the scale of an output channel and its folded bias (cb: the conv's own bias or 0)
WP_HD inline float fold_scale(float g, float var) { return g / sqrtf(var + 1e-5f); }
WP_HD inline float fold_bias(float cb, float mu, float scale, float be) { return (cb - mu) * scale + be; }

// w = hi + lo in bf16 pieces
WP_HD inline void split_bf16_1(float w, uint16_t* hi, uint16_t* lo) { *hi = f2bf(w); *lo = f2bf(w - bf2f(*hi)); }

// fp16 bits of w, round to nearest even (NaN payloads are not part of the bitwise contract)
WP_HD inline uint16_t f2h(float w) { _Float16 h = (_Float16)w; uint16_t u; __builtin_memcpy(&u, &h, 2); return u; }
WP_HD inline float h2f(uint16_t u) { _Float16 h; __builtin_memcpy(&h, &u, 2); return (float)h; }

// The running maximum of |w| over a row as std::max keeps it: a NaN never replaces m.
WP_HD inline float absmax_step(float m, float w) { const float a = fabsf(w); return m < a ? a : m; }

// ilogb of m > 0 (inf: INT_MAX) and 2^e for any e (0 below 2^-149, inf above 2^127), in integer
// exponent arithmetic: no libm call whose host and device versions could differ
WP_HD inline int ilogb_pos(float m) {
    const uint32_t u = f2u(m) & 0x7fffffffu;
    const int e = (int)(u >> 23);
    if (e == 255) return INT_MAX;
    if (e) return e - 127;
    return (31 - __builtin_clz(u)) - 149;   // subnormal: u != 0
}
WP_HD inline float pow2f(int e) {
    if (e > 127) return u2f(0x7f800000u);
    if (e >= -126) return u2f((uint32_t)(e + 127) << 23);
    if (e >= -149) return u2f(1u << (e + 149));
    return 0.0f;
}
// the shift s of a row with max |w| = m: max * 2^s in [2^13, 2^14), capped at 60; 0 for an all-zero row
WP_HD inline int pow2_shift(float m) {
    if (!(m > 0.0f)) return 0;
    const int s = 13 - ilogb_pos(m);
    return s < 60 ? s : 60;
}
// w * up (up = 2^s: exact) in fp16 hi / lo pieces
WP_HD inline void pow2_split_1(float w, float up, uint16_t* fh, uint16_t* fl) {
    float ws = w * up;
#ifdef __HIP_DEVICE_COMPILE__
    // keep the product a value of its own: the gfx9 backend otherwise converts (_Float16)(w * up) with a
    // mixed-precision fma whose +0 addend turns a product of -0 into +0 (the host keeps the sign)
    asm volatile("" : "+v"(ws));
#endif
    *fh = f2h(ws);
    *fl = f2h(ws - h2f(*fh));
}

// ---- layouts: where element (output row o / n, tap t, channel c) of a layer goes
// chunk-blocked [C/16][9][2][N][8]
WP_HD inline size_t chunk_blocked_idx(int N, int o, int t, int c) {
    return ((((size_t)(c / 16) * 9 + t) * 2 + (c / 8) % 2) * N + o) * 8 + c % 8;
}
// k_smallnet's [layer * 9 + tap][n][c] over F channels, and the same element fragment-major
WP_HD inline size_t smallnet_idx(int F, size_t lt, int n, int c) { return (lt * F + n) * F + c; }
WP_HD inline size_t frag_major_idx(int F, size_t lt, int n, int c) {
    const int kk = c / 32, J = n / 16, ln = (n & 15) + 16 * ((c % 32) / 8);
    return (((lt * (F / 32) + kk) * (F / 16) + J) * 64 + ln) * 8 + c % 8;
}

// ---- host loops
// conv + BN (eval) -> folded [co][tap*cpad + c] weights and bias
inline void fold_conv(ParamCursor& pc, int co, int ci, int k, int cpad, bool has_bias, std::vector<float>& W, std::vector<float>& b) {
    const float* w = pc.take((size_t)co * ci * k * k);
    const float* cb = has_bias ? pc.take(co) : nullptr;
    const float* g = pc.take(co);
    const float* be = pc.take(co);
    const float* mu = pc.take(co);
    const float* var = pc.take(co);
    const int taps = k * k;
    W.assign((size_t)co * taps * cpad, 0.0f);
    b.assign(co, 0.0f);
    for (int o = 0; o < co; ++o) {
        const float scale = fold_scale(g[o], var[o]);
        b[o] = fold_bias(cb ? cb[o] : 0.0f, mu[o], scale, be[o]);
        for (int c = 0; c < ci; ++c)
            for (int t = 0; t < taps; ++t) W[((size_t)o * taps + t) * cpad + c] = w[((size_t)o * ci + c) * taps + t] * scale;
    }
}

// FC weights [out][hc][pp] (torch flattens NCHW: index c*pp + px) -> [out][pp][hc] (our pooled
// head map is [px][c])
inline void fc_perm(const float* w, int out, int hc, int pp, std::vector<float>& Wt) {
    Wt.assign((size_t)out * hc * pp, 0.0f);
    for (int o = 0; o < out; ++o)
        for (int c = 0; c < hc; ++c)
            for (int px = 0; px < pp; ++px) Wt[((size_t)o * pp + px) * hc + c] = w[((size_t)o * hc + c) * pp + px];
}

// w = hi + lo in bf16 pieces
inline void split_bf16(const float* w, size_t n, uint16_t* hi, uint16_t* lo) {
    for (size_t i = 0; i < n; ++i) split_bf16_1(w[i], &hi[i], &lo[i]);
}

inline void to_f16(const float* w, size_t n, uint16_t* h16) {
    for (size_t i = 0; i < n; ++i) h16[i] = f2h(w[i]);
}

// The fp16 pieces of AZ_PREC_F16X3: row r of W [rows][K] scaled by 2^s (max |W[r]| * 2^s in
// [2^13, 2^14)) and split into fp16 hi / lo, same layout; sx[r] = 2^-s, bx[r] = b[r] * 2^s (the
// accumulators' start; b and bx may be null).  s is capped at 60 so that a near-zero row (max |w|
// below 2^-47) cannot overflow 2^s or bias * 2^s (its tiny weights keep only fp16's subnormal
// precision); an all-zero row has s = 0.
inline void pow2_split_rows(const float* W, size_t rows, size_t K, const float* b, uint16_t* fh, uint16_t* fl, float* bx,
                            float* sx) {
    for (size_t r = 0; r < rows; ++r) {
        float m = 0.0f;
        for (size_t k = 0; k < K; ++k) m = absmax_step(m, W[r * K + k]);
        const int s = pow2_shift(m);
        const float up = pow2f(s);
        if (bx) bx[r] = b[r] * up;
        sx[r] = pow2f(-s);
        for (size_t k = 0; k < K; ++k) pow2_split_1(W[r * K + k], up, &fh[r * K + k], &fl[r * K + k]);
    }
}

// [N][9][C] -> [C/16][9][2][N][8]: one 64-row piece of a chunk/tap/half is 1 KiB contiguous (C % 16 == 0)
inline std::vector<uint16_t> chunk_blocked(const std::vector<uint16_t>& src, int N, int C) {
    std::vector<uint16_t> out(src.size());
    for (int o = 0; o < N; ++o)
        for (int t = 0; t < 9; ++t)
            for (int c = 0; c < C; ++c)
                out[chunk_blocked_idx(N, o, t, c)] = src[((size_t)o * 9 + t) * C + c];
    return out;
}

// k_smallnet: one 3x3 layer [F][9][cl] appended to dst as [tap][n][c] over F channels (c >= cl zero)
template <class T>
inline void smallnet_append(std::vector<T>& dst, const std::vector<T>& src, int F, int cl) {
    const size_t o = dst.size();
    dst.resize(o + (size_t)9 * F * F, T(0));
    for (int t = 0; t < 9; ++t)
        for (int nn = 0; nn < F; ++nn)
            for (int c = 0; c < cl; ++c) dst[o + smallnet_idx(F, t, nn, c)] = src[((size_t)nn * 9 + t) * cl + c];
}

// k_smallnet's [layer][tap][n][c] weights fragment-major: [layer][tap][32-channel chunk kk]
// [16-channel block J][lane][8] -- one MFMA A operand (rows 16 J + lane % 16, channels
// 32 kk + 8 (lane / 16) ..) is 1 KB contiguous
inline std::vector<uint16_t> frag_major(const std::vector<uint16_t>& src, int F) {
    const size_t ne = src.size();
    std::vector<uint16_t> out(ne);
    const size_t nl = ne / ((size_t)9 * F * F);
    for (size_t lt = 0; lt < nl * 9; ++lt)
        for (int nn = 0; nn < F; ++nn)
            for (int c = 0; c < F; ++c) out[frag_major_idx(F, lt, nn, c)] = src[smallnet_idx(F, lt, nn, c)];
    return out;
}

// Both FC layers as one matrix [NC][K] for k_fc_heads_x3: policy rows [A][K] padded to a multiple of
// 64, then the value rows [H][K] (the partial-column layout of k_fc_finish), in bf16 hi / lo pieces
// and in scaled fp16 hi / lo pieces with rs [NC] = 2^-s.  Padded rows are zero with scale 1.
struct FcRows {
    int NC = 0;
    std::vector<uint16_t> hi, lo, fh, fl;
    std::vector<float> rs;
};
inline FcRows fc_rows(const float* Wp, int A, const float* Wv, int H, int K) {
    const int NTP = (A + 63) / 64, NTV = (H + 63) / 64;
    FcRows f;
    f.NC = (NTP + NTV) * 64;
    const size_t n = (size_t)f.NC * K;
    f.hi.assign(n, 0); f.lo.assign(n, 0); f.fh.assign(n, 0); f.fl.assign(n, 0);
    f.rs.assign(f.NC, 1.0f);
    auto put = [&](const float* Wm, int rows, int r0) {
        const size_t o = (size_t)r0 * K;
        split_bf16(Wm, (size_t)rows * K, f.hi.data() + o, f.lo.data() + o);
        pow2_split_rows(Wm, rows, K, nullptr, f.fh.data() + o, f.fl.data() + o, nullptr, f.rs.data() + r0);
    };
    put(Wp, A, 0);
    put(Wv, H, NTP * 64);
    return f;
}

}  // namespace wpack
