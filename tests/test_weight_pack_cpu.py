"""The weight-packing arithmetic on the CPU (csrc/weight_pack.h compiled for the host).

The loaders (csrc/net_load.hip) turn a parameter blob into the kernels' weight formats with the
plain C++ of weight_pack.h: batch-norm folding, bf16 / fp16 conversion and hi / lo splits, the per-row
power-of-two scaling of the fp16 pieces (AZ_PREC_F16X3: s = min(60, 13 - ilogb(max |w|))) and the
layout permutations.  Here the header is compiled with ROCm's clang++ (it has _Float16; no offload,
no FMA contraction, no fast-math) and every output is compared bitwise with a numpy restatement:
bf16 is round-to-nearest-even on the uint32 view, fp16 goes through np.float16, scales come from
np.frexp / np.ldexp, permutations are reshapes and transposes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLANG = "/opt/rocm/llvm/bin/clang++"
f32, u16, u32 = np.float32, np.uint16, np.uint32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("weightpack") / "libweightpack.so")
    subprocess.run([CLANG, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                    os.path.join(HERE, "native", "weight_pack_host.cpp"), "-o", out], check=True)
    L = ctypes.CDLL(out)
    L.wp_fold_conv.restype = ctypes.c_int
    L.wp_fc_rows.restype = ctypes.c_int
    return L


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _bits(a):
    return np.ascontiguousarray(a).view(u32 if a.dtype == f32 else u16)


# ---- numpy restatement
def np_f2bf(x):
    u = np.ascontiguousarray(x, f32).view(u32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    rne = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffffffff) >> 16
    return np.where(nan, (u >> 16) | 0x40, rne).astype(u16)


def np_bf2f(h):
    return (h.astype(u32) << 16).view(f32)


def np_split_bf16(w):
    hi = np_f2bf(w)
    return hi, np_f2bf(w - np_bf2f(hi))


def np_f16(w):
    with np.errstate(over="ignore"):
        return w.astype(np.float16)


def np_pow2_split_rows(W, b):
    fh, fl = np.zeros(W.shape, u16), np.zeros(W.shape, u16)
    bx, sx = np.zeros(len(W), f32), np.zeros(len(W), f32)
    for r, row in enumerate(W):
        m = np.abs(row).max()
        s = min(60, 13 - (int(np.frexp(m)[1]) - 1)) if m > 0 else 0     # ilogb(m) = frexp exponent - 1
        up = np.ldexp(f32(1), s).astype(f32)
        sx[r] = np.ldexp(f32(1), -s)
        if b is not None:
            bx[r] = b[r] * up
        ws = row * up
        ph = np_f16(ws)
        fh[r] = ph.view(u16)
        fl[r] = np_f16(ws - ph.astype(f32)).view(u16)
    return fh, fl, bx, sx


def c_pow2_split_rows(lib, W, b):
    rows, K = W.shape
    fh, fl = np.zeros(W.shape, u16), np.zeros(W.shape, u16)
    bx, sx = np.zeros(rows, f32), np.zeros(rows, f32)
    lib.wp_pow2_split_rows(_p(W), rows, K, _p(b) if b is not None else None, _p(fh), _p(fl),
                           _p(bx) if b is not None else None, _p(sx))
    return fh, fl, bx, sx


# ---- 16-bit conversions
def test_bf16_round_and_split(lib):
    rng = np.random.default_rng(1)
    x = np.concatenate([
        (rng.standard_normal(4096) * np.exp2(rng.integers(-60, 60, 4096))).astype(f32),
        rng.integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(u32).view(f32),          # every class incl. NaN / inf
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, 1.00390625, 1.01171875, 3.3895314e38], f32),   # ties, overflow
    ])
    got = np.zeros(len(x), u16)
    lib.wp_f2bf(_p(x), len(x), _p(got))
    assert np.array_equal(got, np_f2bf(x))
    back = np.zeros(len(x), f32)
    lib.wp_bf2f(_p(got), len(x), _p(back))
    assert np.array_equal(_bits(back), _bits(np_bf2f(got)))
    fin = x[np.isfinite(x) & (np.abs(x) < 1e38)]
    hi, lo = np.zeros(len(fin), u16), np.zeros(len(fin), u16)
    lib.wp_split_bf16(_p(fin), len(fin), _p(hi), _p(lo))
    rhi, rlo = np_split_bf16(fin)
    assert np.array_equal(hi, rhi) and np.array_equal(lo, rlo)


def test_fp16_conversion(lib):
    rng = np.random.default_rng(2)
    x = np.concatenate([(rng.standard_normal(4096) * np.exp2(rng.integers(-30, 18, 4096))).astype(f32),
                        np.array([0.0, -0.0, 65504.0, 65520.0, 1e-8, 6e-8, 0.1 * 8192], f32)])
    got = np.zeros(len(x), u16)
    lib.wp_to_f16(_p(x), len(x), _p(got))
    assert np.array_equal(got, np_f16(x).view(u16))


# ---- batch-norm folding
@pytest.mark.parametrize("k,bias", [(3, False), (3, True), (1, False), (1, True)])
def test_fold_conv(lib, k, bias):
    co, ci, cpad, taps = 3, 2, 16, k * k
    rng = np.random.default_rng(10 * k + bias)
    w = rng.standard_normal((co, ci, taps)).astype(f32)
    cb = rng.standard_normal(co).astype(f32)
    g, be, mu = (rng.standard_normal(co).astype(f32) for _ in range(3))
    var = (rng.random(co) + 0.1).astype(f32)
    blob = np.concatenate([w.ravel()] + ([cb] if bias else []) + [g, be, mu, var]).astype(f32)
    W, b = np.full((co, taps, cpad), np.nan, f32), np.full(co, np.nan, f32)
    used = lib.wp_fold_conv(_p(blob), co, ci, k, cpad, int(bias), _p(W), _p(b))
    assert used == len(blob)
    scale = g / np.sqrt(var + f32(1e-5))
    rb = ((cb if bias else np.zeros(co, f32)) - mu) * scale + be
    rW = np.zeros((co, taps, cpad), f32)
    rW[:, :, :ci] = w.transpose(0, 2, 1) * scale[:, None, None]
    assert scale.dtype == f32 and rb.dtype == f32
    assert np.array_equal(_bits(b), _bits(rb))
    assert np.array_equal(_bits(W), _bits(rW))


# ---- the fp16 pieces' row scaling
def test_pow2_split_rows(lib):
    rng = np.random.default_rng(3)
    K = 18
    W = (rng.standard_normal((5, K)) * 0.07).astype(f32)           # row 0: an ordinary row
    W[1] = 0.0                                                     # all zero: s = 0
    W[2] = (rng.random(K) * np.exp2(-51.0)).astype(f32)            # max exactly 2^-50: s capped at 60
    W[2, 4] = np.exp2(-50.0)
    W[3] = np.clip(W[3], -0.2, 0.2)                                # max exactly a power of two (0.25)
    W[3, 7] = -0.25
    W[4, 0] = 3.0e4                                                # a large row: negative s
    b = rng.standard_normal(5).astype(f32)
    ref = np_pow2_split_rows(W, b)
    # the rule itself: s = 0 / 60 / 15 for rows 1 / 2 / 3, max |row| * 2^s in [2^13, 2^14) where uncapped
    assert ref[3][1] == 1.0 and ref[3][2] == np.exp2(-60.0) and ref[3][3] == np.exp2(-15.0)
    for r in (0, 3, 4):
        assert 2 ** 13 <= np.abs(W[r]).max() / ref[3][r] < 2 ** 14
    got = c_pow2_split_rows(lib, W, b)
    for g, r in zip(got, ref):
        assert np.array_equal(_bits(g), _bits(r))
    # the probe value: 0.1f * 8192 splits into 0x6266 / 0x3266
    one = np.array([[0.1 * 8192, 8192.0]], f32)
    fh, fl, _, sx = c_pow2_split_rows(lib, one, None)
    assert sx[0] == 1.0 and (fh[0, 0], fl[0, 0]) == (0x6266, 0x3266)


# ---- layouts
def test_chunk_blocked_layout(lib):
    N, C = 3, 32                                                   # two 16-channel chunks, both 8-halves
    src = np.arange(N * 9 * C, dtype=u16).reshape(N, 9, C)
    got = np.zeros(src.size, u16)
    lib.wp_chunk_blocked(_p(src), N, C, _p(got))
    ref = src.reshape(N, 9, C // 16, 2, 8).transpose(2, 1, 3, 0, 4)    # [C/16][9][2][N][8]
    assert np.array_equal(got, ref.ravel())


def test_smallnet_gather_and_frag_major(lib):
    F, cls = 64, [16, 64]                                          # the input conv (16 planes), one trunk layer
    L = len(cls)
    rng = np.random.default_rng(4)
    layers = [rng.integers(1, 2 ** 16, (F, 9, cl)).astype(u16) for cl in cls]
    src = np.concatenate([a.ravel() for a in layers])
    cl = np.array(cls, np.int32)
    dst, frag = np.full((L, 9, F, F), 0xffff, u16), np.zeros(L * 9 * F * F, u16)
    lib.wp_smallnet(_p(src), L, F, _p(cl), _p(dst), _p(frag))
    ref = np.zeros((L, 9, F, F), u16)                              # [layer][tap][n][c], c >= cl zero
    for l, a in enumerate(layers):
        ref[l, :, :, :cls[l]] = a.transpose(1, 0, 2)
    assert np.array_equal(dst, ref)
    # [l][t][kk][J][lane = 16 q + r][e] = [l][t][n = 16 J + r][c = 32 kk + 8 q + e]
    rf = ref.reshape(L, 9, F // 16, 16, F // 32, 4, 8).transpose(0, 1, 4, 2, 5, 3, 6)
    assert np.array_equal(frag, rf.ravel())


def test_fc_perm(lib):
    out, hc, pp = 5, 3, 4
    w = np.random.default_rng(5).standard_normal((out, hc, pp)).astype(f32)
    got = np.zeros((out, pp, hc), f32)
    lib.wp_fc_perm(_p(w), out, hc, pp, _p(got))
    assert np.array_equal(_bits(got), _bits(w.transpose(0, 2, 1)))


def test_fc_rows(lib):
    A, H, K = 70, 5, 8                                             # policy rows pad to 128, value rows to 64
    NC = 192
    rng = np.random.default_rng(6)
    Wp = (rng.standard_normal((A, K)) * 0.05).astype(f32)
    Wv = (rng.standard_normal((H, K)) * 2.0).astype(f32)
    Wp[3] = 0.0
    hi, lo, fh, fl = (np.full((NC, K), 0xffff, u16) for _ in range(4))
    rs = np.zeros(NC, f32)
    assert lib.wp_fc_rows(_p(Wp), A, _p(Wv), H, K, _p(hi), _p(lo), _p(fh), _p(fl), _p(rs)) == NC
    rhi, rlo, rfh, rfl = (np.zeros((NC, K), u16) for _ in range(4))
    rrs = np.ones(NC, f32)
    for Wm, r0 in ((Wp, 0), (Wv, 128)):
        n = len(Wm)
        rhi[r0:r0 + n], rlo[r0:r0 + n] = np_split_bf16(Wm)
        rfh[r0:r0 + n], rfl[r0:r0 + n], _, rrs[r0:r0 + n] = np_pow2_split_rows(Wm, None)
    for g, r in ((hi, rhi), (lo, rlo), (fh, rfh), (fl, rfl), (rs, rrs)):
        assert np.array_equal(_bits(g), _bits(r))
    pad = np.r_[A:128, 128 + H:NC]
    assert not hi[pad].any() and not lo[pad].any() and not fh[pad].any() and not fl[pad].any()
    assert (rs[pad] == 1.0).all()
