"""Head and tail shapes beyond heads 32 / pool 8 / hidden 256 (csrc/net_plan.h's tails trunk / fused /
hconv / convs and head kernels generic / f32 / x3-bf16 / x3-fp16), each on the GPU against the fp32
oracle (oracle/net_oracle.py):

  * parity: |logit - ref| <= 1e-4 and |value - ref| <= 1e-4 (BASELINE.json north_star, as
    test_gpu_net.py; plain bf16 gets that file's sanity bound), with the `tail=` and `heads=` fields of
    net.plan() asserted, so every case provably reaches the kernels it is meant for;
  * bitwise: a board's outputs in a permuted batch and in a tail slice; on every tail=fused case the
    forward under conv flag 0x400000 (k_pool_g8 + gemm_f32 instead of k_pool_heads_g8);
  * predictBatch past the 1024 actions k_softmax_rows once staged in LDS (1500, 4672 and 8192 actions).

The hconv tail is not compared bitwise with the convs tail: the plan takes hconv whenever
head_channels * pool^2 % 32 == 0 off the fused tail and no conv flag turns that off.

A case either runs or is a creation-time refusal asserted with its message; the only refusals are
precisions the shape does not accept (net_plan.h refusal(), restated in accepts() below)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
PREC = {"f32": 0, "bf16x3": 1, "bf16": 2, "fp16": 3, "f16x3": 4}
G8_BOARDS = (8, 9, 13, 15, 19)
FLAGS = 0x204                    # the library's default conv flags
KEEP_POOL = 0x400000             # CONV_F_KEEP_POOL: k_pool_g8 + the head GEMM instead of k_pool_heads_g8

# id: ((board, planes, channels, actions, head_channels, pool, hidden, residual, conv_bias, capacity, B),
#      blocks, precisions, tail, heads -- one name, or {precision: name})
CASES = {}


def _case(name, shape, precs, tail, heads="f32", blocks=1):
    CASES[name] = (shape, blocks, precs.split(), tail, heads)


# k_smallnet_g / k_smallnet_x3 with a runtime pool size: pool_cells<HB, 0, NT>'s general loop (bins wider
# than 3: P = 1, 2, 3) and its "bins <= 3 x 3" branch (P = 5, 6, 7); the FC heads at K = 32 P^2
for _P in (1, 2, 3, 5, 6, 7):
    _case(f"small-P{_P}", (15, 11, 64, 225, 32, _P, 256, 1, 0, 8, 5), "fp16 f16x3 bf16x3", "trunk", blocks=2)
_case("small-bias", (15, 11, 64, 225, 32, 4, 256, 1, 1, 8, 5), "fp16 f16x3", "trunk")
# k_pool_heads_g8 with P^2 < 64: the zeroed pl rows, the m < PP store guard
for _P in (1, 3, 4, 7):
    _case(f"fused9-P{_P}", (9, 11, 128, 81, 32, _P, 256, 1, 0, 8, 5), "fp16 bf16 bf16x3 f16x3", "fused")
_case("fused19-P5", (19, 8, 128, 362, 32, 5, 256, 1, 0, 4, 3), "fp16 bf16 bf16x3 f16x3", "fused")
_case("fused15-P2-bias", (15, 11, 128, 225, 32, 2, 256, 0, 1, 4, 3), "fp16 bf16 bf16x3 f16x3", "fused")
# k_pool_g8 past 64 cells (the second pass of its o += 64 loop), and pooling up (P > board)
_case("pool9x9", (9, 11, 128, 81, 32, 9, 512, 1, 0, 4, 3), "fp16 bf16x3 f32", "hconv")
_case("pool-up", (8, 11, 128, 1500, 32, 10, 4, 1, 0, 4, 2), "fp16 bf16x3 f32", "hconv")
# the hconv tail with 2 head_channels = 32 / 8 / 128 outputs; k_fc_heads with cell stride != head_channels;
# k_fc_finish with hidden % 64 != 0, hidden > 256, 8192 actions
_case("hconv-N32", (8, 111, 128, 4672, 16, 8, 64, 1, 0, 4, 3), "fp16 f16x3 f32", "hconv")
_case("hconv-N8", (13, 8, 128, 170, 4, 8, 260, 1, 0, 4, 3), "fp16 f16x3 f32", "hconv")
_case("hconv-N128", (19, 8, 128, 8192, 64, 2, 1028, 0, 0, 4, 2), "fp16 f16x3 f32", "hconv")
# the convs tail and NET_HEADS_GENERIC: split-K gemm_f32 partials, k_splitk_reduce, k_value_head (hidden > 256)
_case("convs-K36", (9, 11, 128, 81, 4, 3, 260, 1, 1, 4, 3), "fp16 bf16x3 f32", "convs", "generic")
_case("convs-K300", (15, 11, 32, 225, 12, 5, 1028, 1, 0, 4, 3), "bf16x3 f32", "convs", "generic")
_case("convs-K8", (6, 11, 16, 36, 8, 1, 8, 1, 0, 4, 3), "f32", "convs", "generic")
# k_fc_finish with fewer than 64 actions, a single action, four hidden units
for _A, _Hd in ((1, 256), (63, 256), (81, 4), (1, 4)):
    _case(f"policy-A{_A}-H{_Hd}", (9, 11, 128, _A, 32, 8, _Hd, 1, 0, 4, 3), "fp16", "fused")
# k_fc_heads_x3 (capacity >= 512) with an odd number of K steps (K = 288: 9, K = 800: 25, K = 32: 1,
# K = 576 in two slices: 9 each) and cells strided by 2 head_channels
_X3 = {"fp16": "x3-bf16", "f16x3": "x3-fp16"}
for _hc, _P in ((32, 3), (32, 5), (8, 2), (16, 6)):
    _case(f"x3heads-hc{_hc}-P{_P}", (15, 11, 128, 225, _hc, _P, 256, 1, 0, 512, 5), "fp16 f16x3",
          "fused" if _hc == 32 else "hconv", _X3)
# the plan says x3-*, head_channels % 8 != 0: az_launch_fc_heads runs the f32 kernel and drops the fp16 row scale
_case("x3heads-f32-fallback", (15, 11, 128, 225, 4, 8, 256, 1, 0, 512, 5), "fp16 f16x3", "hconv", _X3)
_case("small-cap512-P3", (15, 11, 64, 225, 32, 3, 256, 1, 0, 512, 5), "fp16 f16x3", "trunk", _X3)

RUNS = [(c, p) for c, v in CASES.items() for p in v[2]]
FUSED_RUNS = [(c, p) for c, p in RUNS if CASES[c][3] == "fused"]
PREDICT_RUNS = [(c, p) for c, p in RUNS if c in ("pool-up", "hconv-N32", "hconv-N128", "small-P5")]


def accepts(case, prec):
    """net_plan.h refusal(): the precisions a plain net of this shape is created at."""
    (bs, ci, ch, A, hc, P, Hd, res, bias, cap, B), blocks = CASES[case][:2]
    g8 = bs in G8_BOARDS and ch % 128 == 0
    small = bs == 15 and ch == 64 and ci <= 16 and 1 <= P <= 8 and hc == 32 and blocks <= 15
    if prec == "f32":
        return True
    if prec == "f16x3" and not (g8 or small or blocks == 0):
        return False
    if ch % 32:
        return False
    return prec != "fp16" or (bs == 15 and ch % 64 == 0) or g8


def refusal_message(case, prec):
    ch = CASES[case][0][2]
    if prec == "f16x3":
        return "AZ_PREC_F16X3 needs an 8/9/13/15/19 board with channels % 128 == 0"
    return "bf16/fp16 trunk needs channels % 32 == 0" if ch % 32 else "AZ_PREC_FP16 trunk needs 15x15 boards"


REFUSED = [(c, p) for c in CASES for p in PREC if not accepts(c, p)]


def _id(cp):
    return f"{cp[0]}-{cp[1]}"


def _desc(case, prec):
    import az_amd
    (bs, ci, ch, A, hc, P, Hd, res, bias, cap, B), blocks = CASES[case][:2]
    return az_amd.NetDesc(bs, ci, ch, blocks, A, hc, P, Hd, res, bias, PREC[prec], cap)


def _flags(f):
    from az_amd import _lib
    _lib.lib().az_diag_set_conv_flags(int(f))


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


_REF = {}


def reference(case):
    """(blob, planes, oracle logits, oracle values) of a case: computed once, shared by every precision
    and test of the case, read-only."""
    import net_oracle
    if case not in _REF:
        bs, ci, B = CASES[case][0][0], CASES[case][0][1], CASES[case][0][10]
        desc = _desc(case, "f32")
        blob = net_oracle.init_blob(desc, seed=31)
        rng = np.random.default_rng(1000 + list(CASES).index(case))
        x = (rng.random((B, ci, bs, bs)) < (0.05 if ci > 16 else 0.2)).astype(np.float32)
        rl, rv = net_oracle.forward(desc, blob, x)
        for a in (blob, x, rl, rv):
            a.flags.writeable = False
        _REF[case] = (blob, x, rl, rv)
    return _REF[case]


class Run:
    pass


@pytest.fixture(scope="module")
def run(request, engine):
    """One (case, precision): the net with the case's weights and its forward of the case's boards."""
    import az_amd
    case, prec = request.param
    assert accepts(case, prec), "a listed precision the shape does not accept"
    r = Run()
    r.case, r.prec = case, prec
    r.blob, r.x, r.rl, r.rv = reference(case)
    r.net = az_amd.HipNeuralNetwork(engine, _desc(case, prec))
    try:
        r.net.load_weights(r.blob)
        r.lo, r.v = r.net.forward(r.x)
        yield r
    finally:
        r.net.close()


@pytest.mark.parametrize("run", RUNS, ids=_id, indirect=True)
def test_gpu_head_shape_matches_fp32_reference(run):
    shape, blocks, precs, tail, heads = CASES[run.case]
    plan = run.net.plan().split()
    assert f"tail={tail}" in plan, plan
    assert f"heads={heads[run.prec] if isinstance(heads, dict) else heads}" in plan, plan
    if tail == "trunk":
        assert run.net.trunk_kernel().startswith("k_smallnet_g<" if run.prec == "fp16" else "k_smallnet_x3<")
    el, ev = float(np.abs(run.lo - run.rl).max()), float(np.abs(run.v - run.rv).max())
    print(f"{run.case} {shape} {run.prec}: {' '.join(plan)}: max|dlogit|={el:.3e} (|logit|max {np.abs(run.rl).max():.3f}) "
          f"max|dvalue|={ev:.3e}")
    assert np.isfinite(run.lo).all() and np.isfinite(run.v).all()
    if run.prec == "bf16":
        assert el < 5e-2 * max(1.0, np.abs(run.rl).max()) and ev < 5e-2
    else:
        assert el <= TOL and ev <= TOL


@pytest.mark.parametrize("run", RUNS, ids=_id, indirect=True)
def test_gpu_head_shape_batch_position_independent(run):
    """A board's outputs are bitwise the same in a permuted batch and in a tail slice."""
    B = len(run.x)
    perm = np.random.default_rng(B).permutation(B)
    if (perm == np.arange(B)).all():
        perm = np.roll(perm, 1)
    lo2, v2 = run.net.forward(run.x[perm])
    assert np.array_equal(lo2, run.lo[perm]) and np.array_equal(v2, run.v[perm])
    t = B - 2 if B > 2 else B - 1
    lo3, v3 = run.net.forward(run.x[t:])
    assert np.array_equal(lo3, run.lo[t:]) and np.array_equal(v3, run.v[t:])


@pytest.mark.parametrize("run", FUSED_RUNS, ids=_id, indirect=True)
def test_gpu_head_shape_fused_tail_bitwise(run):
    """k_pool_heads_g8 against k_pool_g8 + gemm_f32<64> (conv flag 0x400000), as test_gpu_pool_heads.py."""
    try:
        _flags(FLAGS | KEEP_POOL)
        assert "tail=hconv" in run.net.plan().split()
        ls, vs = run.net.forward(run.x)
    finally:
        _flags(FLAGS)
    assert "tail=fused" in run.net.plan().split()
    assert np.abs(run.lo).max() > 0
    assert np.array_equal(run.lo, ls) and np.array_equal(run.v, vs)


@pytest.mark.parametrize("run", PREDICT_RUNS, ids=_id, indirect=True)
def test_gpu_head_shape_predict_batch(run):
    """predictBatch's softmax on rows of up to 8192 actions: normalised, every probability that of the
    GPU's own logits, and within 1e-5 of the oracle's."""
    import net_oracle
    pp, pv = run.net.predictBatch(run.x)
    A = run.lo.shape[1]
    bound = (A + 16) * 2.0 ** -24    # a serial fp32 sum of A terms plus a few ulps of expf: any summation order meets it
    sums = pp.astype(np.float64).sum(axis=1)
    z = run.lo.astype(np.float64)
    want = np.exp(z - z.max(axis=1, keepdims=True))
    want /= want.sum(axis=1, keepdims=True)
    rel = float((np.abs(pp - want) / want).max())
    eo = float(np.abs(pp - net_oracle.softmax_policy(run.rl)).max())
    print(f"{run.case} {run.prec} A={A}: max|sum - 1|={np.abs(sums - 1).max():.3e} max rel={rel:.3e} (bound {bound:.3e}) "
          f"max|p - oracle|={eo:.3e}")
    assert np.array_equal(pv, run.v)
    assert np.abs(sums - 1.0).max() <= bound
    assert rel <= bound
    assert eo <= 1e-5


@pytest.mark.parametrize("cp", REFUSED, ids=_id)
def test_gpu_head_shape_refused_precision(engine, cp):
    import az_amd
    case, prec = cp
    with pytest.raises(az_amd.AzError, match=re.escape(refusal_message(case, prec))):
        az_amd.HipNeuralNetwork(engine, _desc(case, prec))
