// csrc/weight_pack.h behind a C interface for tests/test_weight_pack_cpu.py (ctypes).  With
// -DWEIGHT_PACK_MAIN the same small cases run as a stand-alone program (for a sanitizer build).
#include "../../alphazero-multi-game_amd/csrc/weight_pack.h"

using namespace wpack;

extern "C" {

void wp_f2bf(const float* in, int n, uint16_t* out) { for (int i = 0; i < n; ++i) out[i] = f2bf(in[i]); }
void wp_bf2f(const uint16_t* in, int n, float* out) { for (int i = 0; i < n; ++i) out[i] = bf2f(in[i]); }
void wp_split_bf16(const float* w, int n, uint16_t* hi, uint16_t* lo) { split_bf16(w, n, hi, lo); }
void wp_to_f16(const float* w, int n, uint16_t* h) { to_f16(w, n, h); }

// W [co][k*k][cpad], b [co]; returns the blob floats consumed
int wp_fold_conv(const float* blob, int co, int ci, int k, int cpad, int has_bias, float* W, float* b) {
    ParamCursor pc{blob};
    std::vector<float> Wv, bv;
    fold_conv(pc, co, ci, k, cpad, has_bias != 0, Wv, bv);
    std::copy(Wv.begin(), Wv.end(), W);
    std::copy(bv.begin(), bv.end(), b);
    return (int)pc.off;
}

void wp_fc_perm(const float* w, int out, int hc, int pp, float* Wt) {
    std::vector<float> v;
    fc_perm(w, out, hc, pp, v);
    std::copy(v.begin(), v.end(), Wt);
}

void wp_pow2_split_rows(const float* W, int rows, int K, const float* b, uint16_t* fh, uint16_t* fl, float* bx, float* sx) {
    pow2_split_rows(W, rows, K, b, fh, fl, bx, sx);
}

void wp_chunk_blocked(const uint16_t* src, int N, int C, uint16_t* dst) {
    const std::vector<uint16_t> out = chunk_blocked(std::vector<uint16_t>(src, src + (size_t)N * 9 * C), N, C);
    std::copy(out.begin(), out.end(), dst);
}

// layers [L][F][9][cl[l]] back to back -> [L][9][F][F] (dst) and its fragment-major copy (frag)
void wp_smallnet(const uint16_t* src, int L, int F, const int* cl, uint16_t* dst, uint16_t* frag) {
    std::vector<uint16_t> acc;
    for (int l = 0; l < L; ++l) {
        const size_t n = (size_t)F * 9 * cl[l];
        smallnet_append(acc, std::vector<uint16_t>(src, src + n), F, cl[l]);
        src += n;
    }
    std::copy(acc.begin(), acc.end(), dst);
    const std::vector<uint16_t> f = frag_major(acc, F);
    std::copy(f.begin(), f.end(), frag);
}

// returns NC; every output [NC][K] (rs [NC])
int wp_fc_rows(const float* Wp, int A, const float* Wv, int H, int K, uint16_t* hi, uint16_t* lo, uint16_t* fh, uint16_t* fl,
               float* rs) {
    const FcRows f = fc_rows(Wp, A, Wv, H, K);
    std::copy(f.hi.begin(), f.hi.end(), hi); std::copy(f.lo.begin(), f.lo.end(), lo);
    std::copy(f.fh.begin(), f.fh.end(), fh); std::copy(f.fl.begin(), f.fl.end(), fl);
    std::copy(f.rs.begin(), f.rs.end(), rs);
    return f.NC;
}

}  // extern "C"

#ifdef WEIGHT_PACK_MAIN
#include <cstdio>
// the shapes of tests/test_weight_pack_cpu.py on arbitrary values: every read and write of the
// header under the sanitizers
int main() {
    auto vals = [](size_t n, float scale) {
        std::vector<float> v(n);
        for (size_t i = 0; i < n; ++i) v[i] = scale * ((float)((i * 2654435761u) % 2001u) - 1000.0f) / 1000.0f;
        return v;
    };
    for (int k : {3, 1})
        for (int bias : {0, 1}) {
            const int co = 3, ci = 2, cpad = 16;
            std::vector<float> blob = vals((size_t)co * ci * k * k + 5 * co, 1.0f);
            for (float& x : blob) x = std::fabs(x) + 0.5f;     // positive variances
            std::vector<float> W((size_t)co * k * k * cpad), b(co);
            wp_fold_conv(blob.data(), co, ci, k, cpad, bias, W.data(), b.data());
        }
    {
        const int N = 3, C = 32;
        std::vector<uint16_t> src((size_t)N * 9 * C), dst(src.size());
        for (size_t i = 0; i < src.size(); ++i) src[i] = (uint16_t)i;
        wp_chunk_blocked(src.data(), N, C, dst.data());
    }
    {
        const int rows = 4, K = 7;
        std::vector<float> W = vals((size_t)rows * K, 0.3f), b = vals(rows, 2.0f), bx(rows), sx(rows);
        for (int k = 0; k < K; ++k) { W[K + k] = 0.0f; W[2 * K + k] = std::ldexp(W[2 * K + k], -50); }
        W[3 * K] = 0.25f;
        std::vector<uint16_t> fh(W.size()), fl(W.size()), hi(W.size()), lo(W.size());
        wp_pow2_split_rows(W.data(), rows, K, b.data(), fh.data(), fl.data(), bx.data(), sx.data());
        wp_split_bf16(W.data(), (int)W.size(), hi.data(), lo.data());
        wp_to_f16(W.data(), (int)W.size(), hi.data());
    }
    {
        const int L = 2, F = 64, cl[2] = {16, 64};
        std::vector<uint16_t> src((size_t)F * 9 * (16 + 64)), dst((size_t)L * 9 * F * F), frag(dst.size());
        for (size_t i = 0; i < src.size(); ++i) src[i] = (uint16_t)(i * 7);
        wp_smallnet(src.data(), L, F, cl, dst.data(), frag.data());
    }
    {
        const int A = 70, H = 5, K = 8, hc = 2, pp = 4, NC = 192;
        std::vector<float> w = vals((size_t)A * K, 0.1f), wv = vals((size_t)H * K, 3.0f), Wp((size_t)A * K), rs(NC);
        wp_fc_perm(w.data(), A, hc, pp, Wp.data());
        std::vector<uint16_t> hi((size_t)NC * K), lo(hi.size()), fh(hi.size()), fl(hi.size());
        if (wp_fc_rows(Wp.data(), A, wv.data(), H, K, hi.data(), lo.data(), fh.data(), fl.data(), rs.data()) != NC) return 1;
    }
    std::puts("weight_pack ok");
    return 0;
}
#endif
