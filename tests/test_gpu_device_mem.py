"""Who owns device memory (csrc/dev_pool.h): every handle -- az_net, az_search, az_dataset, az_dist --
allocates from pools it holds, so destroying it, or failing half-way through building it, frees
everything.  az_diag_device_mem reads the live totals of every pool in the process and
az_diag_fail_alloc makes the nth allocation from now fail on the host (AZ_ERR_OOM, no device call),
which reaches every allocation-failure path without exhausting the device.

Checked here, through raw ctypes calls (no Python finaliser can move the counters):
  1. create / load / use / destroy of every handle returns the counters to where they were;
  2. a failure at EVERY allocation of every create leaves nothing behind, and a create after the
     sweep gives a handle that computes what one that never saw a failure computes;
  3. a first weight load that fails at any allocation, then succeeds, leaves a weight list that a
     broadcast-style copy (az_diag_net_copy_weights) can rely on, bit for bit;
  4. az_search_set_slot_nets and az_search_enable_eval_log are all-or-nothing at every allocation;
  5. az_search_root_children frees its temporaries on every failure.

Shapes are the smallest that reach each allocation branch (1 block, max_batch 4).  The fused
64-filter kernel's weight sets exist only at 15x15 (net_plan.h az_smallnet_supported), so they are
covered by a 15x15 x 64 net beside the 9x9 x 64 one, which carries the 16-bit trunk copies alone."""
import ctypes
import gc

import numpy as np
import pytest

F32, BF16X3, BF16, FP16, F16X3 = 0, 1, 2, 3, 4
EVAL_NET, EVAL_RANDOM, EVAL_CALLBACK = 0, 2, 4
OOM = -3
BIG = 1 << 20
c_int, c_int64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
ref = ctypes.byref

# id: (board, channels, precision at creation, rand-wire); 11 planes, heads 32 / 8 / 256
NETS = {
    "small-15x15-64":    (15, 64, FP16, False),   # the k_smallnet sets (sm_*), 16-bit planes
    "c64-9x9":           (9, 64, F32, False),     # 16-bit trunk copies, no small-net sets (the nets of the searches)
    "g8-9x9-128":        (9, 128, FP16, False),   # g8 with the zero-padded input layer (in32)
    "g8-15x15-128":      (15, 128, FP16, False),  # g8 with its own input conv
    "f32-9x9-48":        (9, 48, F32, False),     # f32 only: no 16-bit planes, no 16-bit copies
    "randwire-15x15-64": (15, 64, F32, True),     # node buffers, router tables, split-K workspace
}
# id: (game, board, G, evaluator)
SEARCHES = {
    "gomoku-random":   (0, 9, 4, EVAL_RANDOM),
    "gomoku-net":      (0, 9, 4, EVAL_NET),
    "go-random":       (1, 9, 2, EVAL_RANDOM),
    "gomoku-callback": (0, 9, 2, EVAL_CALLBACK),
}
SIMS = 8


@pytest.fixture(scope="module")
def L():
    from az_amd import _lib
    lib = _lib.lib()
    lib.az_diag_net_copy_weights.argtypes = [vp, vp]
    lib.az_diag_net_copy_weights.restype = c_int
    return lib


@pytest.fixture(scope="module")
def eng(L):
    h = vp()
    assert L.az_engine_create(0, ref(h)) == 0, L.az_last_error()
    yield h
    L.az_engine_destroy(h)


@pytest.fixture(autouse=True)
def _disarm(L):
    try:
        yield
    finally:
        L.az_diag_fail_alloc(-1)


def ok(L, rc):
    assert rc == 0, (rc, L.az_last_error().decode())


def mem(L):
    b, n = c_int64(), c_int64()
    ok(L, L.az_diag_device_mem(ref(b), ref(n)))
    return b.value, n.value


def baseline(L):
    gc.collect()
    return mem(L)


def allocs_of(L, call):
    """(return code, pool allocations the call made): read off a countdown too long to fire."""
    assert L.az_diag_fail_alloc(BIG) == -1
    rc = call()
    return rc, BIG - L.az_diag_fail_alloc(-1)


def sweep(L, call, K, base, after_failure=None):
    """Arm every k in [0, K): the call fails with AZ_ERR_OOM, leaves the counters at `base` and the
    countdown disarmed."""
    assert K > 0
    for k in range(K):
        assert L.az_diag_fail_alloc(k) == -1
        rc = call()
        assert rc == OOM, (k, rc, L.az_last_error().decode())
        assert L.az_diag_fail_alloc(-1) == -1, (k, "still armed")
        assert mem(L) == base, (k, mem(L), base)
        if after_failure is not None:
            after_failure(k)


# ---------------------------------------------------------------- nets
def net_desc(name, prec=None):
    from az_amd import _lib
    bs, ch, p, rw = NETS[name]
    return _lib.NetDesc(bs, 11, ch, 1, bs * bs, 32, 8, 256, 0 if rw else 1, 0, p if prec is None else prec, 4)


def net_create(L, eng, name, out, prec=None):
    d = net_desc(name, prec)
    return (L.az_net_create_randwire if NETS[name][3] else L.az_net_create)(eng, ref(d), ref(out))


def net_x(name):
    bs = NETS[name][0]
    return np.ascontiguousarray((np.random.default_rng(500 + bs).random((4, 11, bs, bs)) < 0.25).astype(np.float32))


def net_forward(L, h, name):
    bs = NETS[name][0]
    x = net_x(name)
    lo, v = np.zeros((4, bs * bs), np.float32), np.zeros(4, np.float32)
    fp = ctypes.POINTER(ctypes.c_float)
    ok(L, L.az_net_forward(h, x.ctypes.data_as(fp), 4, lo.ctypes.data_as(fp), v.ctypes.data_as(fp)))
    return lo.view(np.uint32).copy(), v.view(np.uint32).copy()


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NETS))
def test_gpu_net_lifecycle_and_create_sweep(L, eng, name):
    base = baseline(L)
    h = vp()
    rc, K = allocs_of(L, lambda: net_create(L, eng, name, h))
    ok(L, rc)
    created = mem(L)
    assert K > 0 and created[1] - base[1] == K and created[0] > base[0]
    rc, KL = allocs_of(L, lambda: L.az_net_init_random(h, 5))
    ok(L, rc)
    assert KL > 0 and mem(L)[1] == created[1] + KL
    loaded = mem(L)
    want = net_forward(L, h, name)
    ok(L, L.az_net_init_random(h, 6))                     # a reload allocates nothing
    assert mem(L) == loaded
    ok(L, L.az_net_profile(h, 1))
    assert mem(L)[1] == loaded[1] + 1
    net_forward(L, h, name)
    ok(L, L.az_net_profile(h, 1))                         # the clock buffer is allocated once
    assert mem(L)[1] == loaded[1] + 1
    L.az_net_destroy(h)
    assert mem(L) == base
    print(f"net {name}: create K = {K}, first load K = {KL}, {created[0] - base[0]} + {loaded[0] - created[0]} bytes")

    out = vp()
    sweep(L, lambda: net_create(L, eng, name, out), K, base)
    assert out.value is None
    ok(L, net_create(L, eng, name, out))
    ok(L, L.az_net_init_random(out, 5))
    assert mem(L) == loaded
    assert same(net_forward(L, out, name), want)
    L.az_net_destroy(out)
    assert mem(L) == base


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small-15x15-64", "g8-9x9-128"])
def test_gpu_first_load_failure_sweep(L, eng, name):
    """A first load that fails at allocation k, then a load that succeeds: the net's weight list is
    complete and in the loader's order -- a fresh net filled from it buffer by buffer computes the
    source's outputs, which are those of a net whose first load never failed."""
    base = baseline(L)
    refnet = vp()
    ok(L, net_create(L, eng, name, refnet))
    rc, K = allocs_of(L, lambda: L.az_net_init_random(refnet, 5))
    ok(L, rc)
    want = {}
    for prec in (FP16, F16X3):
        ok(L, L.az_net_set_precision(refnet, prec))
        want[prec] = net_forward(L, refnet, name)
    assert not same(want[FP16], want[F16X3])
    L.az_net_destroy(refnet)
    assert mem(L) == base and K > 0
    print(f"first load {name}: K = {K}")
    for k in range(K):
        src, dst = vp(), vp()
        ok(L, net_create(L, eng, name, src))
        ok(L, net_create(L, eng, name, dst))
        try:
            assert L.az_diag_fail_alloc(k) == -1
            assert L.az_net_init_random(src, 5) == OOM, k
            assert L.az_diag_fail_alloc(-1) == -1
            ok(L, L.az_net_init_random(src, 5))
            ok(L, L.az_diag_net_copy_weights(dst, src))
            for prec in (FP16, F16X3):
                ok(L, L.az_net_set_precision(src, prec))
                ok(L, L.az_net_set_precision(dst, prec))
                got = net_forward(L, src, name)
                assert same(got, want[prec]), (k, prec, "source")
                assert same(net_forward(L, dst, name), got), (k, prec, "copy")
        finally:
            L.az_net_destroy(src)
            L.az_net_destroy(dst)
        assert mem(L) == base, k


# ---------------------------------------------------------------- searches
def search_cfg(name):
    from az_amd import _lib
    game, bs, G, kind = SEARCHES[name]
    return _lib.SearchCfg(G, bs, SIMS, 1.5, 0.0, 3, kind, 7, 12345, 42, 1, 0, 0.03, 0.25, 4, 0, 0, game)


def make_net(L, eng, seed, name="c64-9x9"):
    h = vp()
    ok(L, net_create(L, eng, name, h))
    ok(L, L.az_net_init_random(h, seed))
    return h


def uniform_evaluator(name):
    from az_amd import _lib
    game, bs, G, kind = SEARCHES[name]
    NA = bs * bs + game

    def fn(_user, n, games, plen, moves, max_path, planes, n_planes, pol, val):
        for i in range(n * NA):
            pol[i] = 1.0 / NA
        for i in range(n):
            val[i] = 0.0
        return 0
    return _lib.EVAL_FN(fn)


def search_create(L, eng, name, net, out, cb=None):
    cfg = search_cfg(name)
    rc = L.az_search_create(eng, net, ref(cfg), ref(out))
    if rc == 0 and cb is not None:
        ok(L, L.az_search_set_evaluator(out, cb, None))
    return rc


def root_visits(L, s, name):
    game, bs, G, _ = SEARCHES[name]
    NA = bs * bs + game
    out = []
    for g in range(G):
        act, N = (c_int * NA)(), (c_int * NA)()
        n = c_int()
        ok(L, L.az_search_root_children(s, g, act, N, None, None, None, ref(n)))
        out.append((list(act[:n.value]), list(N[:n.value])))
    return out


def start(L, s, name):
    G = SEARCHES[name][2]
    games = (c_int * G)(*range(G))
    ok(L, L.az_search_new_games(s, games, G))
    ok(L, L.az_search_add_noise(s, 0.03, 0.25))


def play(L, s, name):
    """One 8-simulation search and the move it chooses: (root children and visits per game, actions)."""
    game, bs, G, _ = SEARCHES[name]
    NA = bs * bs + game
    ok(L, L.az_search_run(s))
    roots = root_visits(L, s, name)
    act, nch, term, res = (c_int * G)(), (c_int * G)(), (c_int * G)(), (c_int * G)()
    val, probs, cact = (ctypes.c_float * G)(), (ctypes.c_float * (G * NA))(), (c_int * (G * NA))()
    ok(L, L.az_search_select(s, 0, 1.0, act, val, probs, cact, nch))
    ok(L, L.az_search_apply(s, act, term, res))
    return roots, list(act)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SEARCHES))
def test_gpu_search_lifecycle_and_create_sweep(L, eng, name):
    kind = SEARCHES[name][3]
    net = make_net(L, eng, 9) if kind == EVAL_NET else None
    cb = uniform_evaluator(name) if kind == EVAL_CALLBACK else None
    base = baseline(L)
    s = vp()
    rc, K = allocs_of(L, lambda: search_create(L, eng, name, net, s, cb))
    ok(L, rc)
    created = mem(L)
    assert K > 0 and created[1] - base[1] == K
    start(L, s, name)
    ok(L, L.az_search_run(s))
    want = root_visits(L, s, name)
    assert mem(L) == created                               # root_children: one call per game, nothing kept
    assert any(sum(N) > 0 for _, N in want)
    for _ in range(2):
        ok(L, L.az_search_enable_eval_log(s, 0, 16))
        assert mem(L)[1] == created[1] + 4
    for _ in range(2):
        ok(L, L.az_search_profile(s, 1))
        assert mem(L)[1] == created[1] + 6
    ok(L, L.az_search_run(s))
    L.az_search_destroy(s)
    assert mem(L) == base
    print(f"search {name}: create K = {K}, {created[0] - base[0]} bytes")

    out = vp()
    sweep(L, lambda: search_create(L, eng, name, net, out, cb), K, base)
    assert out.value is None
    ok(L, search_create(L, eng, name, net, out, cb))
    assert mem(L) == created
    start(L, out, name)
    ok(L, L.az_search_run(out))
    assert root_visits(L, out, name) == want
    L.az_search_destroy(out)
    assert mem(L) == base
    if net:
        L.az_net_destroy(net)


@pytest.mark.gpu
def test_gpu_root_children_frees_its_temporaries(L, eng):
    name = "gomoku-random"
    base = baseline(L)
    s = vp()
    ok(L, search_create(L, eng, name, None, s))
    start(L, s, name)
    ok(L, L.az_search_run(s))
    created = mem(L)
    NA = 81
    act, N, n = (c_int * NA)(), (c_int * NA)(), c_int()
    call = lambda: L.az_search_root_children(s, 1, act, N, None, None, None, ref(n))   # noqa: E731
    seen = []
    for i in range(3):
        before = mem(L)
        rc, K = allocs_of(L, call)
        ok(L, rc)
        assert K == 8 and mem(L) == before == created, i
        seen.append((list(act[:n.value]), list(N[:n.value])))
    assert seen[0] == seen[1] == seen[2] and sum(seen[0][1]) > 0
    sweep(L, call, 8, created)
    ok(L, call())
    assert (list(act[:n.value]), list(N[:n.value])) == seen[0]
    L.az_search_destroy(s)
    assert mem(L) == base


@pytest.mark.gpu
def test_gpu_slot_nets_and_eval_log_are_all_or_nothing(L, eng):
    """set_slot_nets (1 -> 3 nets -> set_net) balances; a failure at any allocation of set_slot_nets (to 2
    nets) or enable_eval_log leaves the handle playing exactly as an untouched twin, and the log
    enabled before still reads back what it held."""
    name = "gomoku-net"
    G, NA, CAP = 4, 81, 256
    nets = [make_net(L, eng, seed) for seed in (9, 10, 11)]
    base = baseline(L)
    h, twin = vp(), vp()
    ok(L, search_create(L, eng, name, nets[0], h))
    one = mem(L)
    ok(L, search_create(L, eng, name, nets[0], twin))
    start(L, h, name)
    start(L, twin, name)
    ok(L, L.az_search_enable_eval_log(h, 0, CAP))
    fp = ctypes.POINTER(ctypes.c_float)

    def read_log():
        pol, val = np.zeros((CAP, NA), np.float32), np.zeros(CAP, np.float32)
        planes, n = np.zeros((CAP, 11, 9, 9), np.float32), c_int()
        ok(L, L.az_search_read_eval_log(h, pol.ctypes.data_as(fp), val.ctypes.data_as(fp), planes.ctypes.data_as(fp), ref(n)))
        k = n.value
        return k, pol[:k].tobytes(), val[:k].tobytes(), planes[:k].tobytes()

    assert play(L, h, name) == play(L, twin, name)
    log = [read_log()]
    first_log = log[0][0]
    assert first_log > 0
    armed = mem(L)
    arr2 = (vp * 2)(nets[0].value, nets[1].value)
    sn2 = (ctypes.c_uint8 * G)(0, 1, 1, 0)

    def still_the_twin(k):
        assert read_log() == log[0], (k, "the old log changed")
        assert play(L, h, name) == play(L, twin, name), k
        log[0] = read_log()
        assert log[0][0] <= CAP

    set2 = lambda: L.az_search_set_slot_nets(h, arr2, 2, sn2)                 # noqa: E731
    # the allocation counts of the two calls, on a third handle that is then dropped
    probe = vp()
    ok(L, search_create(L, eng, name, nets[0], probe))
    rc, K_slot = allocs_of(L, lambda: L.az_search_set_slot_nets(probe, arr2, 2, sn2))
    ok(L, rc)
    rc, K_log = allocs_of(L, lambda: L.az_search_enable_eval_log(probe, 1, 32))
    ok(L, rc)
    L.az_search_destroy(probe)
    assert mem(L) == armed and K_slot == 6 and K_log == 4
    print(f"all-or-nothing: set_slot_nets K = {K_slot}, enable_eval_log K = {K_log}")
    sweep(L, set2, K_slot, armed, still_the_twin)
    sweep(L, lambda: L.az_search_enable_eval_log(h, 1, 32), K_log, armed, still_the_twin)
    assert first_log < log[0][0] <= CAP                      # the old log went on filling under its old capacity

    # regions grown from 1 net to 3, back to one net: the old region buffers are freed, not kept
    arr3 = (vp * 3)(*[n.value for n in nets])
    sn3 = (ctypes.c_uint8 * G)(0, 1, 2, 0)
    ok(L, L.az_search_set_slot_nets(h, arr3, 3, sn3))
    assert mem(L)[1] == armed[1] + 1                          # + the slot assignment; 5 region buffers replaced
    ok(L, L.az_search_run(h))
    ok(L, L.az_search_set_slot_nets(h, arr2, 2, sn2))         # no growth: only the assignment is replaced
    assert mem(L)[1] == armed[1] + 1
    ok(L, L.az_search_set_net(h, nets[0]))
    ok(L, L.az_search_run(h))
    L.az_search_destroy(h)
    L.az_search_destroy(twin)
    assert mem(L) == base and one[1] > base[1]
    for n in nets:
        L.az_net_destroy(n)


# ---------------------------------------------------------------- dataset, dist
@pytest.mark.gpu
def test_gpu_dataset_lifecycle_and_create_sweep(L, eng):
    base = baseline(L)
    d = vp()
    rc, K = allocs_of(L, lambda: L.az_dataset_create(eng, 0, 9, ref(d)))
    ok(L, rc)
    created = mem(L)
    assert K == 1 and created[1] == base[1] + 1
    n_moves, actions, nch, res = (c_int * 1)(2), (c_int * 2)(0, 1), (c_int * 2)(2, 2), (c_int * 1)(1)
    pol = (ctypes.c_float * 4)(0.5, 0.5, 0.25, 0.75)
    E = c_int64()
    ok(L, L.az_dataset_extract(d, 1, n_moves, actions, nch, pol, res, 1, None, ref(E)))
    assert E.value == 16
    stored = mem(L)
    assert stored[1] == created[1] + 4                        # the rows; the per-call uploads are gone
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(c_int)
    idx = np.arange(16, dtype=np.int64)
    st, po = np.zeros((16, 11, 9, 9), np.float32), np.zeros((16, 81), np.float32)
    pl, va = np.zeros(16, np.int32), np.zeros(16, np.float32)
    gather = lambda: L.az_dataset_gather(d, idx.ctypes.data_as(ctypes.POINTER(c_int64)), 16, st.ctypes.data_as(fp),  # noqa: E731
                                         po.ctypes.data_as(fp), pl.ctypes.data_as(ip), va.ctypes.data_as(fp))
    rc, KG = allocs_of(L, gather)
    ok(L, rc)
    first = (st.copy(), po.copy(), pl.copy(), va.copy())
    assert mem(L) == stored and KG == 5 and pl.tolist() == [2] * 16
    sweep(L, gather, KG, stored)
    order = idx[::-1].copy()
    permute = lambda: L.az_dataset_permute(d, order.ctypes.data_as(ctypes.POINTER(c_int64)))   # noqa: E731
    sweep(L, permute, 5, stored)                             # a failed shuffle keeps the store
    ok(L, gather())
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip((st, po, pl, va), first))
    ok(L, permute())
    assert mem(L) == stored
    ok(L, gather())
    assert all(np.array_equal(a.view(np.uint32), b[::-1].view(np.uint32)) for a, b in zip((st, po, pl, va), first))
    L.az_dataset_destroy(d)
    assert mem(L) == base
    out = vp()
    sweep(L, lambda: L.az_dataset_create(eng, 0, 9, ref(out)), K, base)
    assert out.value is None


@pytest.mark.gpu
def test_gpu_dist_lifecycle_and_init_sweep(L, eng):
    base = baseline(L)
    uid = (ctypes.c_ubyte * 128)()
    ok(L, L.az_dist_unique_id(uid))
    out = vp()
    sweep(L, lambda: L.az_dist_init(eng, 0, 1, uid, 60000, ref(out)), 1, base)   # fails before any rank joins
    assert out.value is None
    d = vp()
    rc, K = allocs_of(L, lambda: L.az_dist_init(eng, 0, 1, uid, 60000, ref(d)))
    ok(L, rc)
    assert K == 1 and mem(L)[1] == base[1] + 1
    ok(L, L.az_dist_barrier(d))
    net = make_net(L, eng, 3)
    with_net = mem(L)
    ok(L, L.az_net_broadcast_weights(d, net, 0))
    assert mem(L)[1] == with_net[1] + 1                       # the blob staging buffer, kept for the next broadcast
    ok(L, L.az_net_broadcast_weights(d, net, 0))
    assert mem(L)[1] == with_net[1] + 1
    L.az_net_destroy(net)
    L.az_dist_destroy(d)
    assert mem(L) == base
