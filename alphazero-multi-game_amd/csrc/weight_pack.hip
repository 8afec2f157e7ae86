// weight_pack.hip -- the weight packing on the device (az_net_load_weights_device): a parameter blob
// in device memory -> every weight buffer of an az_net, byte for byte what the host loops of
// weight_pack.h produce.  Two kernels do the work, each one block per output channel row:
//   k_fold  BN folding and the [co][ci][tap] -> [co][tap][cpad] transpose through LDS (both sides
//           coalesced); without BN the plain permutation of the FC weights
//   k_rows  reads a folded row twice (max |w|, then the pieces) and writes every 16-bit piece set of
//           it in every layout: row-major, chunk-blocked and k_smallnet's plain / fragment-major
// The element arithmetic and the index functions are weight_pack.h's (WP_HD), so host and device
// share one source; built with -ffp-contract=off -fno-fast-math like the host loops.
#include "weight_pack_dev.h"

#include "weight_pack.h"

namespace wpdev {
namespace {

using namespace wpack;

constexpr int THREADS = 256;
constexpr int TILE = 4096;   // floats of LDS per block in k_fold

__global__ __launch_bounds__(THREADS) void k_fold(Fold f) {
    __shared__ float tile[TILE];
    const int o = blockIdx.x, taps = f.taps, ci = f.ci;
    const int tp = taps | 1;        // odd row pitch: the transposed read is free of bank conflicts
    const int CH = TILE / tp;       // channels per pass
    float scale = 1.0f;
    if (f.g) {
        scale = fold_scale(f.g[o], f.var[o]);
        if (threadIdx.x == 0) f.b[o] = fold_bias(f.cb ? f.cb[o] : 0.0f, f.mu[o], scale, f.be[o]);
    }
    const float* src = f.w + (size_t)o * ci * taps;
    float* dst = f.W + (size_t)o * taps * f.cpad;
    for (int c0 = 0; c0 < ci; c0 += CH) {
        const int n = min(CH, ci - c0);
        for (int i = threadIdx.x; i < n * taps; i += THREADS) tile[(i / taps) * tp + i % taps] = src[(size_t)c0 * taps + i];
        __syncthreads();
        for (int i = threadIdx.x; i < n * taps; i += THREADS) {
            const int t = i / n, c = i % n;
            const float w = tile[c * tp + t];
            dst[(size_t)t * f.cpad + c0 + c] = f.g ? w * scale : w;
        }
        __syncthreads();
    }
    const int pad = f.cpad - ci;    // the zero channels the host gets from assign(.., 0)
    for (int i = threadIdx.x; i < pad * taps; i += THREADS) dst[(size_t)(i / pad) * f.cpad + ci + i % pad] = 0.0f;
}

template <int V> struct alignas(2 * V) U16x { uint16_t v[V]; };
template <int V> struct alignas(4 * V) F32x { float v[V]; };
template <int V> __device__ inline void put(uint16_t* p, size_t i, const U16x<V>& x) {
    if (p) *reinterpret_cast<U16x<V>*>(p + i) = x;
}

// V consecutive channels per thread (8: 16-byte stores; 1 where C is no multiple of 8)
template <int V>
__global__ __launch_bounds__(THREADS) void k_rows(Rows a) {
    __shared__ float red[THREADS / 64];
    const int r = blockIdx.x, K = a.taps * a.C;
    const float* Wr = a.W + (size_t)r * K;
    float m = 0.0f;
    for (int k = threadIdx.x * V; k < K; k += THREADS * V) {
        const F32x<V> w = *reinterpret_cast<const F32x<V>*>(Wr + k);
        for (int e = 0; e < V; ++e) m = absmax_step(m, w.v[e]);
    }
    for (int o = 32; o; o >>= 1) { const float t = __shfl_xor(m, o); m = m < t ? t : m; }   // no NaN among the partial maxima
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int i = 1; i < THREADS / 64; ++i) m = m < red[i] ? red[i] : m;
    const int s = pow2_shift(m);
    const float up = pow2f(s);
    if (threadIdx.x == 0) {
        const float sx = pow2f(-s);
        if (a.bx) a.bx[r] = a.b[r] * up;
        if (a.sx) a.sx[r] = sx;
        if (a.sm_b) {
            const size_t i = (size_t)a.sm_l * a.F + r;
            a.sm_b[i] = a.b[r];
            a.sm_bx[i] = a.b[r] * up;
            a.sm_sx[i] = sx;
        }
    }
    const bool layouts = a.bk_bf || a.sm_w;
    for (int k = threadIdx.x * V; k < K; k += THREADS * V) {
        const F32x<V> w = *reinterpret_cast<const F32x<V>*>(Wr + k);
        U16x<V> hi, lo, h16, fh, fl;
        for (int e = 0; e < V; ++e) {
            split_bf16_1(w.v[e], &hi.v[e], &lo.v[e]);
            h16.v[e] = f2h(w.v[e]);
            pow2_split_1(w.v[e], up, &fh.v[e], &fl.v[e]);
        }
        const size_t i = (size_t)r * K + k;
        put(a.hi, i, hi); put(a.lo, i, lo); put(a.h16, i, h16); put(a.fh, i, fh); put(a.fl, i, fl);
        if (!layouts) continue;
        const int t = k / a.C, c = k % a.C;
        if (a.bk_bf) {
            const size_t j = chunk_blocked_idx(a.N, r, t, c);
            put(a.bk_bf, j, hi); put(a.bk_h, j, h16); put(a.bk_lo, j, lo); put(a.bk_fh, j, fh); put(a.bk_fl, j, fl);
        }
        if (a.sm_w) {
            const size_t lt = (size_t)a.sm_l * 9 + t;
            put(a.sm_w, smallnet_idx(a.F, lt, r, c), h16);
            const size_t j = frag_major_idx(a.F, lt, r, c);
            put(a.sm_wf, j, h16); put(a.sm_xh, j, hi); put(a.sm_xl, j, lo); put(a.sm_fh, j, fh); put(a.sm_fl, j, fl);
        }
    }
    if (a.sm_w && a.C < a.F) {      // the input conv's channels C .. F-1 of the 64-channel layout
        const int pad = a.F - a.C;
        U16x<V> z;
        for (int e = 0; e < V; ++e) z.v[e] = 0;
        for (int i = threadIdx.x * V; i < 9 * pad; i += THREADS * V) {
            const int t = i / pad, c = a.C + i % pad;
            const size_t lt = (size_t)a.sm_l * 9 + t;
            put(a.sm_w, smallnet_idx(a.F, lt, r, c), z);
            const size_t j = frag_major_idx(a.F, lt, r, c);
            put(a.sm_wf, j, z); put(a.sm_xh, j, z); put(a.sm_xl, j, z); put(a.sm_fh, j, z); put(a.sm_fl, j, z);
        }
    }
}

template <class T>
__global__ __launch_bounds__(THREADS) void k_fill(T* dst, size_t n, T v) {
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * THREADS) dst[i] = v;
}
__global__ __launch_bounds__(THREADS) void k_copy(const float* src, float* dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * THREADS) dst[i] = src[i];
}
inline unsigned blocks_for(size_t n) { return (unsigned)std::min<size_t>((n + THREADS - 1) / THREADS, 2048); }

}  // namespace

hipError_t fold(hipStream_t st, const Fold& f) {
    if (f.co <= 0 || f.ci <= 0 || f.taps <= 0 || f.taps >= TILE || f.cpad < f.ci) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_fold, dim3(f.co), dim3(THREADS), 0, st, f);
    return hipGetLastError();
}

hipError_t rows(hipStream_t st, const Rows& r) {
    if (r.N <= 0 || r.taps <= 0 || r.C <= 0) return hipErrorInvalidValue;
    if (r.bk_bf && (r.taps != 9 || r.C % 16)) return hipErrorInvalidValue;
    if (r.sm_w && (r.taps != 9 || r.N != r.F || r.F % 32 || r.C > r.F || r.C % 8)) return hipErrorInvalidValue;
    if (r.C % 8 == 0) hipLaunchKernelGGL(k_rows<8>, dim3(r.N), dim3(THREADS), 0, st, r);
    else hipLaunchKernelGGL(k_rows<1>, dim3(r.N), dim3(THREADS), 0, st, r);
    return hipGetLastError();
}

hipError_t copy_f32(hipStream_t st, const float* src, float* dst, size_t n) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_copy, dim3(blocks_for(n)), dim3(THREADS), 0, st, src, dst, n);
    return hipGetLastError();
}
hipError_t fill_u16(hipStream_t st, uint16_t* dst, size_t n, uint16_t v) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fill<uint16_t>, dim3(blocks_for(n)), dim3(THREADS), 0, st, dst, n, v);
    return hipGetLastError();
}
hipError_t fill_f32(hipStream_t st, float* dst, size_t n, float v) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_fill<float>, dim3(blocks_for(n)), dim3(THREADS), 0, st, dst, n, v);
    return hipGetLastError();
}

}  // namespace wpdev
