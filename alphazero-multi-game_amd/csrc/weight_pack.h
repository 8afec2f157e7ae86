// weight_pack.h -- the host arithmetic that turns a parameter blob into the kernels' weight
// layouts: batch-norm folding, the 16-bit conversions and hi / lo splits, the per-row power-of-two
// scaling of the fp16 pieces (AZ_PREC_F16X3) and the layout permutations.  Plain C++ with no HIP
// dependency (net_host.hip keeps the allocations and uploads), so tests/test_weight_pack_cpu.py
// checks every output bit for bit without a device.  Compile with -ffp-contract=off -fno-fast-math:
// the results are compared bitwise.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace wpack {

struct ParamCursor {
    const float* p; size_t off = 0;
    const float* take(size_t n) { const float* r = p + off; off += n; return r; }
};

inline uint16_t f2bf(float f) {   // round to nearest even
    uint32_t u; std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; std::memcpy(&f, &u, 4); return f; }

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
        const float scale = g[o] / std::sqrt(var[o] + 1e-5f);
        b[o] = ((cb ? cb[o] : 0.0f) - mu[o]) * scale + be[o];
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
    for (size_t i = 0; i < n; ++i) { hi[i] = f2bf(w[i]); lo[i] = f2bf(w[i] - bf2f(hi[i])); }
}

inline void to_f16(const float* w, size_t n, uint16_t* h16) {
    for (size_t i = 0; i < n; ++i) { _Float16 h = (_Float16)w[i]; std::memcpy(&h16[i], &h, 2); }
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
        for (size_t k = 0; k < K; ++k) m = std::max(m, std::fabs(W[r * K + k]));
        const int s = m > 0.0f ? std::min(60, 13 - std::ilogb(m)) : 0;
        const float up = std::ldexp(1.0f, s);
        if (bx) bx[r] = b[r] * up;
        sx[r] = std::ldexp(1.0f, -s);
        for (size_t k = 0; k < K; ++k) {
            const float ws = W[r * K + k] * up;                     // exact: a power of two
            const _Float16 ph = (_Float16)ws;
            const _Float16 pl = (_Float16)(ws - (float)ph);
            std::memcpy(&fh[r * K + k], &ph, 2);
            std::memcpy(&fl[r * K + k], &pl, 2);
        }
    }
}

// [N][9][C] -> [C/16][9][2][N][8]: one 64-row piece of a chunk/tap/half is 1 KiB contiguous (C % 16 == 0)
inline std::vector<uint16_t> chunk_blocked(const std::vector<uint16_t>& src, int N, int C) {
    std::vector<uint16_t> out(src.size());
    for (int o = 0; o < N; ++o)
        for (int t = 0; t < 9; ++t)
            for (int c = 0; c < C; ++c)
                out[((((size_t)(c / 16) * 9 + t) * 2 + (c / 8) % 2) * N + o) * 8 + c % 8] = src[((size_t)o * 9 + t) * C + c];
    return out;
}

// k_smallnet: one 3x3 layer [F][9][cl] appended to dst as [tap][n][c] over F channels (c >= cl zero)
template <class T>
inline void smallnet_append(std::vector<T>& dst, const std::vector<T>& src, int F, int cl) {
    const size_t o = dst.size();
    dst.resize(o + (size_t)9 * F * F, T(0));
    for (int t = 0; t < 9; ++t)
        for (int nn = 0; nn < F; ++nn)
            for (int c = 0; c < cl; ++c) dst[o + ((size_t)t * F + nn) * F + c] = src[((size_t)nn * 9 + t) * cl + c];
}

// k_smallnet's [layer][tap][n][c] weights fragment-major: [layer][tap][32-channel chunk kk]
// [16-channel block J][lane][8] -- one MFMA A operand (rows 16 J + lane % 16, channels
// 32 kk + 8 (lane / 16) ..) is 1 KB contiguous
inline std::vector<uint16_t> frag_major(const std::vector<uint16_t>& src, int F) {
    const size_t ne = src.size();
    std::vector<uint16_t> out(ne);
    const size_t nl = ne / ((size_t)9 * F * F);
    for (size_t l = 0; l < nl; ++l)
        for (int t = 0; t < 9; ++t)
            for (int kk = 0; kk < F / 32; ++kk)
                for (int J = 0; J < F / 16; ++J)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int e = 0; e < 8; ++e) {
                            const int nn = 16 * J + (ln & 15), c = 32 * kk + 8 * (ln >> 4) + e;
                            out[((((l * 9 + t) * (F / 32) + kk) * (F / 16) + J) * 64 + ln) * 8 + e] =
                                src[((l * 9 + t) * F + nn) * F + c];
                        }
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
