"""The lifecycle contract of an az_net (include/az_engine.h az_net_set_precision / az_net_load_weights /
az_net_init_random, the receiving side of az_net_broadcast_weights):

    A net's forward outputs, trunk_kernel() and get_weights() depend only on its description, its
    current precision and the last blob loaded.  How it got there does not matter.  A
    set_precision(p) that returns success means forwards at p work; one that fails leaves the net
    exactly as it was.

az_net_set_precision only switches the dispatch, so every weight set a precision reads must be on
the device from the last load, whatever precision the net had then (csrc/net_load.hip), and the
buffer list a broadcast copies must hold every one of them whatever the first load's precision.

Every history ends at (final precision p, blob B) and is compared BITWISE with `fresh = create(p);
load(B)`, whose outputs are first held to the fp32 oracle (so a mistake both sides share cannot
pass).  The shape classes are the smallest nets that reach each load / dispatch branch:

  small    15x15, 64 channels, 2 blocks   k_smallnet_g / k_smallnet_x3 (the sm_* weight sets)
  g8-15    15x15, 128 channels, 1 block   conv3x3_v6 / v7x3 SLIM, the 16-plane g8 input conv
  g8-9     9x9, 128 channels, 1 block     DENSE tiles, the zero-padded 32-channel input layer (in32)
  nhwc     15x15, 32 channels, 1 block    the NHWC bf16-split path; FP16 and F16X3 are refused
  f32only  8x8, 16 channels, conv bias    every precision but F32 is refused
"""
import ctypes
import itertools

import numpy as np
import pytest

from replay_util import compare_roots, replay_eval_log, root_record

TOL = 1e-4                      # tests/test_gpu_net.py: F32, the X3 precisions and FP16 at init scale
F32, BF16X3, BF16, FP16, F16X3 = 0, 1, 2, 3, 4
PNAME = {F32: "f32", BF16X3: "bf16x3", BF16: "bf16", FP16: "fp16", F16X3: "f16x3"}
PRECS = [F32, BF16X3, BF16, FP16, F16X3]

SHAPES = {  # id: (board, planes, channels, blocks, B, conv_bias); heads 32 / 8 / 256, residual 1
    "small":   (15, 11, 64, 2, 5, 0),
    "g8-15":   (15, 11, 128, 1, 3, 0),
    "g8-9":    (9, 11, 128, 1, 3, 0),
    "nhwc":    (15, 11, 32, 1, 3, 0),
    "f32only": (8, 11, 16, 1, 3, 1),
}
# the precisions az_net_create accepts per shape class (net_host.hip check_precision): bf16 pieces need
# channels % 32 == 0, fp16 operands 15x15 with channels % 64 == 0 or a g8 board with channels % 128 == 0,
# fp16 pieces a g8 board with channels % 128 == 0 or the 15x15 64-channel fused net
ACCEPTED = {
    "small":   [F32, BF16X3, BF16, FP16, F16X3],
    "g8-15":   [F32, BF16X3, BF16, FP16, F16X3],
    "g8-9":    [F32, BF16X3, BF16, FP16, F16X3],
    "nhwc":    [F32, BF16X3, BF16],
    "f32only": [F32],
}
SEED_A, SEED_B, SEED_C = 22, 21, 23
FINAL = [(s, p) for s in SHAPES for p in PRECS if p in ACCEPTED[s]]
SWITCHED = [(s, p) for s, p in FINAL if len(ACCEPTED[s]) > 1]     # final states another precision can lead to
REFUSED = [(s, p) for s in SHAPES for p in PRECS if p not in ACCEPTED[s]]


def _id(sp):
    return f"{sp[0]}-{PNAME[sp[1]]}"


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def _desc(shape, prec, max_batch=None):
    import az_amd
    bs, ci, ch, blocks, B, bias = SHAPES[shape]
    return az_amd.NetDesc(bs, ci, ch, blocks, bs * bs, 32, 8, 256, 1, bias, prec, max_batch or B)


def _create(engine, shape, prec, max_batch=None):
    import az_amd
    return az_amd.HipNeuralNetwork(engine, _desc(shape, prec, max_batch))


def _x(shape):
    bs, ci, _, _, B, _ = SHAPES[shape]
    rng = np.random.default_rng(300 + bs + SHAPES[shape][2])
    return (rng.random((B, ci, bs, bs)) < 0.25).astype(np.float32)


_blobs, _fresh = {}, {}


def _blob(shape, seed):
    import net_oracle
    if (shape, seed) not in _blobs:
        b = net_oracle.init_blob(_desc(shape, F32), seed)
        b.setflags(write=False)
        _blobs[(shape, seed)] = b
    return _blobs[(shape, seed)]


def _fresh_state(engine, shape, prec, seed):
    """(logits, values, trunk kernel) of create(prec); load(init_blob(seed)) on the shape's inputs,
    computed once per module and held to the fp32 oracle at tests/test_gpu_net.py's bounds."""
    import net_oracle
    key = (shape, prec, seed)
    if key not in _fresh:
        blob, x = _blob(shape, seed), _x(shape)
        net = _create(engine, shape, prec)
        try:
            net.load_weights(blob)
            lo, v = net.forward(x)
            kernel = net.trunk_kernel()
        finally:
            net.close()
        rl, rv = net_oracle.forward(_desc(shape, prec), np.array(blob), x)
        el, ev = float(np.abs(lo - rl).max()), float(np.abs(v - rv).max())
        print(f"fresh {shape} {PNAME[prec]} seed {seed}: trunk {kernel}, max|dlogit|={el:.3e} "
              f"(|logit|max {np.abs(rl).max():.3f}) max|dvalue|={ev:.3e}")
        if prec == BF16:      # the throughput variant: test_gpu_net.py's sanity bound
            assert el < 5e-2 * max(1.0, float(np.abs(rl).max())) and ev < 5e-2, (el, ev)
        else:
            assert el <= TOL and ev <= TOL, (el, ev)
        lo.setflags(write=False)
        v.setflags(write=False)
        _fresh[key] = (lo, v, kernel)
    return _fresh[key]


def _check(net, fresh, blob, x, where):
    """The contract's observables of `net` against the fresh net's, bit for bit."""
    lo, v, kernel = fresh
    l1, v1 = net.forward(x)
    assert np.array_equal(l1, lo) and np.array_equal(v1, v), ("forward", *where)
    assert net.trunk_kernel() == kernel, ("trunk_kernel", *where, net.trunk_kernel(), kernel)
    assert np.array_equal(net.get_weights(), blob), ("get_weights", *where)
    l2, v2 = net.forward(x[1:3])
    assert np.array_equal(l2, lo[1:3]) and np.array_equal(v2, v[1:3]), ("sub-batch", *where)


def _copy_weights(dst, src):
    """What az_net_broadcast_weights does to a non-root rank's net (tests/test_gpu_dist.py)."""
    from az_amd import _lib
    f = _lib.lib().az_diag_net_copy_weights
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    _lib.check(f(dst.h, src.h))


@pytest.mark.gpu
@pytest.mark.parametrize("sp", FINAL + REFUSED, ids=_id)
def test_gpu_net_create_accepts_what_the_shape_class_says(engine, sp):
    """The precisions each shape class is created at (the histories below start from them)."""
    import az_amd
    shape, p = sp
    if p in ACCEPTED[shape]:
        _create(engine, shape, p).close()
    else:
        with pytest.raises(az_amd.AzError):
            _create(engine, shape, p)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", SWITCHED, ids=_id)
def test_gpu_net_history_switch_after_load(engine, sp):
    """a: create(q); load(B); set_precision(p)."""
    shape, p = sp
    x, B = _x(shape), _blob(shape, SEED_B)
    fresh = _fresh_state(engine, shape, p, SEED_B)
    for q in ACCEPTED[shape]:
        if q == p:
            continue
        net = _create(engine, shape, q)
        try:
            net.load_weights(B)
            net.set_precision(p)
            _check(net, fresh, B, x, ("a", PNAME[q]))
        finally:
            net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", SWITCHED, ids=_id)
def test_gpu_net_history_reload_at_other_precision(engine, sp):
    """b: create(p); load(A); set_precision(q); load(B); set_precision(p) -- no weight set of A may
    survive the second load.  (A and B do differ: the outputs of create(p); load(A) are others.)"""
    shape, p = sp
    x, A, B = _x(shape), _blob(shape, SEED_A), _blob(shape, SEED_B)
    fresh = _fresh_state(engine, shape, p, SEED_B)
    stale = _fresh_state(engine, shape, p, SEED_A)
    assert not np.array_equal(stale[0], fresh[0]) and not np.array_equal(stale[1], fresh[1])
    for q in ACCEPTED[shape]:
        if q == p:
            continue
        net = _create(engine, shape, p)
        try:
            net.load_weights(A)
            la, va = net.forward(x)
            assert np.array_equal(la, stale[0]) and np.array_equal(va, stale[1]), ("b: first load", PNAME[q])
            net.set_precision(q)
            net.load_weights(B)
            net.set_precision(p)
            _check(net, fresh, B, x, ("b", PNAME[q]))
            lb, vb = net.forward(x)
            assert not np.array_equal(lb, stale[0]) and not np.array_equal(vb, stale[1]), ("b: stale", PNAME[q])
        finally:
            net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", SWITCHED, ids=_id)
def test_gpu_net_history_switch_then_load(engine, sp):
    """c: create(q); load(A); set_precision(p); load(B)."""
    shape, p = sp
    x, A, B = _x(shape), _blob(shape, SEED_A), _blob(shape, SEED_B)
    fresh = _fresh_state(engine, shape, p, SEED_B)
    for q in ACCEPTED[shape]:
        if q == p:
            continue
        net = _create(engine, shape, q)
        try:
            net.load_weights(A)
            net.set_precision(p)
            net.load_weights(B)
            _check(net, fresh, B, x, ("c", PNAME[q]))
        finally:
            net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", SWITCHED, ids=_id)
def test_gpu_net_history_init_random_after_switch(engine, sp):
    """d: create(q); set_precision(p); init_random(s) against create(p); load(init_blob(s))."""
    shape, p = sp
    x, B = _x(shape), _blob(shape, SEED_B)
    fresh = _fresh_state(engine, shape, p, SEED_B)
    for q in ACCEPTED[shape]:
        if q == p:
            continue
        net = _create(engine, shape, q)
        try:
            net.set_precision(p)
            net.init_random(SEED_B)
            _check(net, fresh, B, x, ("d", PNAME[q]))
        finally:
            net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", SWITCHED, ids=_id)
def test_gpu_net_history_broadcast_receiver(engine, sp):
    """e: src = create(q1); load(B) and a never-loaded dst = create(q2), every ordered pair q1 != q2 the
    shape accepts (F32 / FP16 in both orders on `small` among them): az_diag_net_copy_weights(dst,
    src) as a broadcast does on a non-root rank, then dst.set_precision(p).  A second round with
    blob C loaded into src catches a buffer missing from a list recorded at the first load."""
    shape, p = sp
    x, B, C = _x(shape), _blob(shape, SEED_B), _blob(shape, SEED_C)
    fresh_b = _fresh_state(engine, shape, p, SEED_B)
    fresh_c = _fresh_state(engine, shape, p, SEED_C)
    assert not np.array_equal(fresh_b[0], fresh_c[0])
    pairs = list(itertools.permutations(ACCEPTED[shape], 2))
    assert shape != "small" or {(F32, FP16), (FP16, F32)} <= set(pairs)
    for q1, q2 in pairs:
        src, dst = _create(engine, shape, q1), _create(engine, shape, q2)
        try:
            src.load_weights(B)
            _copy_weights(dst, src)
            dst.set_precision(p)
            _check(dst, fresh_b, B, x, ("e", PNAME[q1], PNAME[q2]))
            src.load_weights(C)
            _copy_weights(dst, src)
            _check(dst, fresh_c, C, x, ("e: second round", PNAME[q1], PNAME[q2]))
        finally:
            src.close()
            dst.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", REFUSED, ids=_id)
def test_gpu_net_refused_precision_leaves_the_net_as_it_was(engine, sp):
    """f: where the shape has no kernel for p, set_precision(p) raises, the next forward is bitwise
    the forward before the attempt and trunk_kernel() is unchanged."""
    import az_amd
    shape, p = sp
    x, B = _x(shape), _blob(shape, SEED_B)
    for q in ACCEPTED[shape]:
        fresh = _fresh_state(engine, shape, q, SEED_B)
        net = _create(engine, shape, q)
        try:
            net.load_weights(B)
            l0, v0 = net.forward(x)
            with pytest.raises(az_amd.AzError):
                net.set_precision(p)
            assert net.desc.precision == q
            l1, v1 = net.forward(x)
            assert np.array_equal(l1, l0) and np.array_equal(v1, v0), ("f", PNAME[q])
            _check(net, fresh, B, x, ("f", PNAME[q]))
        finally:
            net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [F16X3, FP16], ids=lambda p: PNAME[p])
@pytest.mark.parametrize("shape", ["small", "g8-15"])
def test_gpu_net_range_fallback_in_place(engine, shape, prec):
    """g: what HipNeuralNetwork::fallbackToFp32Range does, on the handle that reported the overflow.  A
    trunk whose activations leave the fp16 range (trunk_scaled_blob at 3e5) fails the 16-bit forward
    with AZ_ERR_RANGE; set_precision(BF16X3) on the same net then gives a fresh BF16X3 net's outputs
    bit for bit (within 1e-4 of the fp32 network), and switching back raises the range error again:
    the engine's sticky flag is neither lost nor left set."""
    import az_amd
    import net_oracle
    from az_amd import _lib
    from test_gpu_trained_scale import trunk_scaled_blob
    bs, ci = SHAPES[shape][0], SHAPES[shape][1]
    Bn = 8
    x = (np.random.default_rng(77).random((Bn, ci, bs, bs)) < 0.25).astype(np.float32)
    blob, amax = trunk_scaled_blob(_desc(shape, prec, Bn), 99, x, act_max=3.0e5)
    assert amax > 65504
    ref = _create(engine, shape, BF16X3, Bn)
    net = _create(engine, shape, prec, Bn)
    try:
        ref.load_weights(blob)
        rl3, rv3 = ref.forward(x)
        kernel3 = ref.trunk_kernel()
        rl, rv = net_oracle.forward(_desc(shape, BF16X3, Bn), blob, x)
        el, ev = float(np.abs(rl3 - rl).max()), float(np.abs(rv3 - rv).max())
        print(f"range fallback {shape} {PNAME[prec]}: max activation {amax:.3e}, bf16x3 max|dlogit|={el:.3e} "
              f"max|dvalue|={ev:.3e}")
        assert el <= TOL and ev <= TOL
        net.load_weights(blob)
        for _ in range(2):
            with pytest.raises(az_amd.AzError, match="fp16 activation overflow") as ei:
                net.forward(x)
            assert ei.value.code == _lib.AZ_ERR_RANGE
            net.set_precision(BF16X3)
            l3, v3 = net.forward(x)
            assert np.array_equal(l3, rl3) and np.array_equal(v3, rv3)
            assert net.trunk_kernel() == kernel3
            l3, v3 = net.forward(x)                      # no flag left set by the reported overflow
            assert np.array_equal(l3, rl3) and np.array_equal(v3, rv3)
            net.set_precision(prec)
        with pytest.raises(az_amd.AzError, match="fp16 activation overflow"):
            net.forward(x)
    finally:
        net.close()
        ref.close()


G, SIMS = 4, 16


def _search(engine, net, **kw):
    import az_amd
    return az_amd.ParallelMCTS(engine, n_games=G, board_size=15, num_simulations=SIMS, evaluator=az_amd.AZ_EVAL_NET,
                               net=net, noise_seed=42, noise_seed_stride=1, **kw)


def _play(m, moves, on_move=None):
    """`moves` plies of every slot; returns the root records per ply and slot."""
    out = []
    for ply in range(moves):
        m.search()
        act, val, probs, cact, nch = m.select(True, 1.0)
        assert all(int(act[g]) >= 0 and nch[g] > 0 for g in range(G)), (ply, act.tolist())
        out.append([root_record(m, g, act, val, probs, nch) for g in range(G)])
        term, _ = m.updateWithMove(act)
        assert not term.any()
        if ply % 2 == 0:
            m.addDirichletNoise(0.03, 0.25)
        if on_move is not None:
            on_move(ply)
    return out


@pytest.mark.gpu
def test_gpu_search_on_switched_net_matches_fresh(engine):
    """(i) a search handle on a net with history a (created F32, loaded, switched to F16X3) gives the
    root children, probabilities and value bits of one on a net created at F16X3."""
    B = _blob("small", SEED_B)
    recs = []
    for q in (F16X3, F32):
        net = _create(engine, "small", q, G)
        m = None
        try:
            net.load_weights(B)
            net.set_precision(F16X3)
            assert net.trunk_kernel() == "k_smallnet_x3<15, 8, true, 2>"
            m = _search(engine, net)
            m.newGames()
            m.addDirichletNoise(0.03, 0.25)
            recs.append(_play(m, 2))
        finally:
            if m is not None:
                m.close()
            net.close()
    assert recs[0] == recs[1]
    assert any(len(r["N"]) > 1 for r in recs[0][1])


@pytest.mark.gpu
def test_gpu_search_precision_switch_between_moves(engine):
    """(ii) set_precision on the net of a live search, between two moves (bench.py's parity mode): the
    evaluations logged before the switch are bitwise a dense forward of a fresh FP16 net on the
    logged planes, those after it of a fresh F16X3 net, and the game replays bit for bit."""
    import az_oracle as O
    B = _blob("small", SEED_B)
    logged, cap = 1, (SIMS + 2) * 3
    net = _create(engine, "small", FP16, G)
    m = None
    n_before = []
    try:
        net.load_weights(B)
        m = _search(engine, net)
        m.enableEvalLog(logged, cap)
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)

        def switch(ply):
            if ply == 0:
                n_before.append(len(m.readEvalLog(cap)[1]))
                net.set_precision(F16X3)
        dev = [ply[logged] for ply in _play(m, 2, switch)]
        pol, valv, planes = m.readEvalLog(cap)
    finally:
        if m is not None:
            m.close()
        net.close()
    n0 = n_before[0]
    assert 0 < n0 < len(pol) < cap, (n0, len(pol))
    ref = replay_eval_log(pol, valv, planes, [(logged, 2)], bs=15, sims=SIMS, game=O.GAME_GOMOKU)[0]
    compare_roots(dev, ref["moves"])
    for prec, sl in ((FP16, slice(0, n0)), (F16X3, slice(n0, len(pol)))):
        fresh = _create(engine, "small", prec, G)
        try:
            fresh.load_weights(B)
            xs = planes[sl]
            dv = np.concatenate([fresh.forward(xs[i:i + G])[1] for i in range(0, len(xs), G)])
        finally:
            fresh.close()
        same = dv.view(np.uint32) == valv[sl].view(np.uint32)
        assert same.all(), (PNAME[prec], np.flatnonzero(~same).tolist())
    # the two precisions do give different bits on these positions: the split above is not vacuous
    other = _create(engine, "small", FP16, G)
    try:
        other.load_weights(B)
        xs = planes[n0:]
        dv = np.concatenate([other.forward(xs[i:i + G])[1] for i in range(0, len(xs), G)])
    finally:
        other.close()
    assert (dv.view(np.uint32) != valv[n0:].view(np.uint32)).any()


@pytest.mark.gpu
def test_gpu_host_network_set_precision_after_init_random():
    """The C++ surface (what the self_play binary does with --net-blocks / --net-channels): a
    HipNeuralNetwork built at AZ_PREC_F32 on the `small` shape, initRandom, setPrecision(AZ_PREC_F16X3),
    predictBatch -- bitwise the outputs of one constructed at AZ_PREC_F16X3."""
    import _alphazero_cpp as az
    bs, _, ch, blocks, Bn, _ = SHAPES["small"]
    states = []
    rng = np.random.default_rng(4)
    for i in range(Bn):
        s = az.GomokuState(bs)
        for _ in range(i * 5):
            s.makeMove(int(rng.choice(s.getLegalMoves())))
        states.append(s)
    outs = []
    for created in (F16X3, F32):
        net = az.HipNeuralNetwork(boardSize=bs, channels=ch, blocks=blocks, precision=created, maxBatch=Bn)
        net.initRandom(7)
        net.setPrecision(F16X3)
        pol, val = net.predictBatch(states)
        outs.append((np.asarray(pol, np.float32), np.asarray(val, np.float32)))
        del net
    assert np.isfinite(outs[0][0]).all() and outs[0][0].max() > 0
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
