"""az_net_load_weights_device (HipNeuralNetwork.load_weights_device): a parameter blob in device memory,
packed by the kernels of csrc/weight_pack.hip, leaves a net in exactly the state az_net_load_weights
leaves after loading the same values on the host.

The first property is about bytes: every buffer of the weight pool -- what a broadcast compares and sends
-- is compared with a host-loaded twin through az_diag_net_compare_weights, after az_diag_net_fill_weights
poisoned the device-loaded net, so padding that no forward reads counts too.  The others are the lifecycle
contract of tests/test_gpu_net_lifecycle.py (whose shape classes, blobs and fresh states these tests use:
the smallest nets that reach every pack branch), a live search handle, the broadcast source and the closed
self-play -> replay -> SGD -> publish loop.  NaN weights are outside the bitwise contract (the fp16
conversions may differ in a NaN's payload); everything else is bit for bit."""
import ctypes

import numpy as np
import pytest
import torch    # before libaz_hip.so is loaded: the engine and torch then share one HIP runtime

from replay_util import root_record
from test_gpu_net_lifecycle import (ACCEPTED, BF16X3, F16X3, F32, FINAL, FP16, PNAME, SEED_A, SEED_B, SEED_C, SHAPES, TOL,
                                    _blob, _check, _copy_weights, _create, _desc, _fresh_state, _id, _x)

RW_SHAPES = {  # id: randwire_net_desc arguments, the precisions az_net_create_randwire accepts
    "rw-9-32": ((9, 32, 2, 11, 4), [F32]),
    "rw-9-16": ((9, 16, 1, 11, 4), [F32]),
    "rw-15-64": ((15, 64, 1, 11, 4), [F32, BF16X3, FP16]),   # the node convs' 16-bit weight copies
}
ALL_SHAPES = list(SHAPES) + list(RW_SHAPES)


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def _make(engine, shape, prec):
    import az_amd
    if shape in SHAPES:
        return _create(engine, shape, prec)
    d = az_amd.randwire_net_desc(*RW_SHAPES[shape][0])
    d.precision = prec
    return az_amd.HipNeuralNetwork(engine, d, randwire=True)


def _accepted(shape):
    return ACCEPTED[shape] if shape in SHAPES else RW_SHAPES[shape][1]


_rw_blobs = {}


def _any_blob(shape, seed):
    if shape in SHAPES:
        return _blob(shape, seed)
    if (shape, seed) not in _rw_blobs:
        import az_amd
        import randwire_oracle as RW
        b = RW.init_blob(az_amd.randwire_net_desc(*RW_SHAPES[shape][0]), RW.load_graphs(), seed)
        b.setflags(write=False)
        _rw_blobs[(shape, seed)] = b
    return _rw_blobs[(shape, seed)]


def _dev(blob):
    return torch.from_numpy(np.array(blob, np.float32)).cuda()


def _fill(net, byte):
    from az_amd import _lib
    _lib.check(_lib.lib().az_diag_net_fill_weights(net.h, byte))


def _first_difference(a, b, show=True):
    """(buffer, byte) of the first differing weight byte of two nets; (-1, 0) when all are equal."""
    from az_amd import _lib
    buf, off = ctypes.c_int(-7), ctypes.c_size_t(7)
    _lib.check(_lib.lib().az_diag_net_compare_weights(a.h, b.h, ctypes.byref(buf), ctypes.byref(off)))
    if buf.value >= 0 and show:
        print(_lib.lib().az_last_error().decode())      # the bytes around the difference
    return buf.value, off.value


def _device_mem():
    from az_amd import _lib
    b, k = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().az_diag_device_mem(ctypes.byref(b), ctypes.byref(k)))
    return b.value, k.value


def _assert_same_bytes(engine, shape, blob):
    """Every history of a device load of `blob` against one host-loaded net, for every precision the
    shape accepts: poisoned then loaded, loaded with nothing allocated before, and loaded over other weights."""
    other = _any_blob(shape, SEED_A)
    t = _dev(blob)
    host = _make(engine, shape, _accepted(shape)[0])
    try:
        host.load_weights(blob)
        for q in _accepted(shape):
            for history in ("poisoned", "fresh", "reloaded"):
                net = _make(engine, shape, q)
                try:
                    if history == "poisoned":
                        _fill(net, 0xA5)
                        assert _first_difference(host, net, show=False) != (-1, 0)       # the poison is seen
                    elif history == "reloaded":
                        net.load_weights(other)
                    net.load_weights_device(t)
                    assert _first_difference(host, net) == (-1, 0), (shape, PNAME[q], history)
                finally:
                    net.close()
    finally:
        host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_gpu_device_load_writes_every_weight_byte(engine, shape):
    """1: byte equality of every weight buffer, padding included, with a host-loaded net."""
    _assert_same_bytes(engine, shape, _any_blob(shape, SEED_B))


def _param_slices(desc):
    import net_oracle
    out, off = {}, 0
    for name, shp, _, _ in net_oracle.param_shapes(desc):
        n = int(np.prod(shp))
        out[name] = (off, shp)
        off += n
    return out


def _unit_var():
    """A running_var v with fp32 v + 1e-5 == 1 exactly: with gamma 1 the folded row is the row itself."""
    eps = np.float32(1e-5)
    v = np.float32(1) - eps
    for _ in range(8):
        s = np.float32(v + eps)
        if s == np.float32(1):
            return v
        v = np.nextafter(v, np.float32(2 if s < 1 else 0), dtype=np.float32)
    raise AssertionError("no unit variance found")


def _edge_blob(shape):
    """init_blob with planted rows: output channels of the first trunk conv and of the input conv, and
    rows of the policy FC (which reach the row scaling unfolded)."""
    desc = _desc(shape, F32)
    blob = np.array(_blob(shape, SEED_B))
    sl = _param_slices(desc)

    def view(name):
        off, shp = sl[name]
        return blob[off:off + int(np.prod(shp))].reshape(shp)

    def plant(w, r0):
        """Rows r0.. of w [rows][...]: returns the rows whose BN must be the identity."""
        rng = np.random.default_rng(5)
        w[r0] = 0.0                                                   # all zero: s = 0
        w[r0 + 1] = np.clip(w[r0 + 1], -0.03, 0.03)                   # max |w| exactly 2^-5 ...
        w[r0 + 1].flat[3] = -0.03125
        w[r0 + 2] = np.clip(w[r0 + 2], -0.03, 0.03)                   # ... and one ulp below
        w[r0 + 2].flat[4] = np.nextafter(np.float32(0.03125), np.float32(0))
        w[r0 + 3] = (rng.standard_normal(w[r0 + 3].shape) * 1e-30).astype(np.float32)    # s capped at 60
        w[r0 + 4] = (rng.standard_normal(w[r0 + 4].shape) * 1e-40).astype(np.float32)    # a subnormal row
        assert 0 < np.abs(w[r0 + 4]).max() < np.finfo(np.float32).tiny
        w[r0 + 5].flat[::3] = np.float32(3e-41)                       # subnormals among ordinary weights
        w[r0 + 5].flat[1::3] = -0.0
        w[r0 + 6].flat[2] = 1.0e6                                     # fp16 overflow in the unscaled copy
        w[r0 + 6].flat[5] = -0.0
        return range(r0, r0 + 7)

    for conv, bn in (("blocks.0.0", "blocks.0.1"), ("input_conv", "input_bn")):
        w = view(conv + ".weight")
        ident = plant(w, 1)
        g, var = view(bn + ".weight"), view(bn + ".running_var")
        g[list(ident)] = 1.0
        var[list(ident)] = _unit_var()
        var[9], var[10] = 0.0, 1e-12                                  # scale ~ 316 gamma: eps alone
        g[11] = 0.0                                                   # every folded weight +-0
        g[12] = -0.0
    plant(view("policy_fc.weight"), 2)
    plant(view("value_fc1.weight"), 249)                              # up to the last value row (256 hidden)
    assert np.isfinite(blob).all()
    return blob


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["g8-15", "small"])
def test_gpu_device_load_edge_rows(engine, shape):
    """2: zero rows, power-of-two and just-below row maxima, the shift's cap, subnormals, -0.0, fp16
    overflow, BN variance 0 and 1e-12, gamma 0: the same bytes as the host load."""
    blob = _edge_blob(shape)
    assert not np.array_equal(blob, _blob(shape, SEED_B))
    _assert_same_bytes(engine, shape, blob)


@pytest.mark.gpu
@pytest.mark.parametrize("sp", FINAL, ids=_id)
def test_gpu_device_load_lifecycle(engine, sp):
    """3: create(q); load_weights_device(B); set_precision(p) gives a fresh create(p); load_weights(B) --
    forward, sub-batch, trunk_kernel() and get_weights() bit for bit (the fresh outputs first held to the
    fp32 oracle) -- and so does every step of host load A -> device load B -> host load C."""
    shape, p = sp
    x = _x(shape)
    A, B, C = (_blob(shape, s) for s in (SEED_A, SEED_B, SEED_C))
    fa, fb, fc = (_fresh_state(engine, shape, p, s) for s in (SEED_A, SEED_B, SEED_C))
    assert not np.array_equal(fa[0], fb[0]) and not np.array_equal(fb[0], fc[0])
    tB = _dev(B)
    for q in [q for q in ACCEPTED[shape] if q != p] or [p]:
        net = _create(engine, shape, q)
        try:
            net.load_weights_device(tB)
            net.set_precision(p)
            _check(net, fb, B, x, ("device load", PNAME[q]))
        finally:
            net.close()
    net = _create(engine, shape, p)
    try:
        net.load_weights(A)
        _check(net, fa, A, x, ("A",))
        net.load_weights_device(tB)
        _check(net, fb, B, x, ("A -> device B",))
        net.load_weights(C)
        _check(net, fc, C, x, ("device B -> C",))
    finally:
        net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["small", "g8-9", "rw-9-16"])
def test_gpu_device_load_allocates_once(engine, shape):
    """4: the second and the third device load of a net allocate nothing."""
    tA, tB = _dev(_any_blob(shape, SEED_A)), _dev(_any_blob(shape, SEED_B))
    net = _make(engine, shape, F32)
    try:
        mem = []
        for t in (tA, tB, tA):
            net.load_weights_device(t)
            mem.append(_device_mem())
        assert mem[0] == mem[1] == mem[2], mem
        assert np.array_equal(net.get_weights(), _any_blob(shape, SEED_A))
        assert _device_mem() == mem[2]                                # nor does fetching the host blob
    finally:
        net.close()


G5, SIMS5, BS5 = 8, 32, 9
LOG5 = 6 * (SIMS5 + 2)      # room for the logged game's evaluations of four moves


def _handle(engine, blob):
    import az_amd
    bs, ci, ch, blocks, _, bias = SHAPES["g8-9"]
    net = az_amd.HipNeuralNetwork(engine, az_amd.NetDesc(bs, ci, ch, blocks, bs * bs, 32, 8, 256, 1, bias, F16X3, G5))
    net.load_weights(blob)
    m = az_amd.ParallelMCTS(engine, n_games=G5, board_size=BS5, num_simulations=SIMS5, evaluator=az_amd.AZ_EVAL_NET,
                            net=net, noise_seed=42, noise_seed_stride=1)
    m.enableEvalLog(1, LOG5)
    m.newGames()
    m.addDirichletNoise(0.03, 0.25)
    return net, m


def _plies(m, n):
    out = []
    for ply in range(n):
        m.search()
        act, val, probs, cact, nch = m.select(True, 1.0)
        assert all(int(act[g]) >= 0 and nch[g] > 0 for g in range(G5))
        out.append([root_record(m, g, act, val, probs, nch) for g in range(G5)])
        term, _ = m.updateWithMove(act)
        assert not term.any()
        if ply % 2 == 0:
            m.addDirichletNoise(0.03, 0.25)
    return out


@pytest.mark.gpu
def test_gpu_device_load_on_a_live_search_handle(engine):
    """5: weights published to the net of a search handle between two moves: the device route and the host
    route give the same roots (N / W / P bits), moves and logged evaluations, others than the old weights."""
    A, B = _blob("g8-9", SEED_A), _blob("g8-9", SEED_B)
    tB = _dev(B)
    runs = {}
    for route in ("device", "host", "kept"):
        net, m = _handle(engine, A)
        try:
            recs = _plies(m, 2)
            if route == "device":
                net.load_weights_device(tB)
            elif route == "host":
                net.load_weights(B)
            recs += _plies(m, 2)
            pol, val, planes = m.readEvalLog(LOG5)
            assert 0 < len(val) < LOG5
            runs[route] = (recs, pol.view(np.uint32).tolist(), val.view(np.uint32).tolist(), planes.tolist())
        finally:
            m.close()
            net.close()
    assert runs["device"][0][:2] == runs["kept"][0][:2]
    assert runs["device"] == runs["host"]
    assert runs["device"][0][2:] != runs["kept"][0][2:] and runs["device"][2] != runs["kept"][2]
    assert any(len(r["N"]) > 1 for r in runs["device"][0][3])


@pytest.mark.gpu
@pytest.mark.parametrize("shape,q1,q2,p", [("small", F32, FP16, F16X3), ("g8-9", F16X3, F32, BF16X3)],
                         ids=["small", "g8-9"])
def test_gpu_device_loaded_net_is_a_broadcast_source(engine, shape, q1, q2, p):
    """6: what a broadcast does to a non-root rank's net, from a device-loaded source: the buffers and the
    canonical blob (the source's host copy is fetched lazily) arrive."""
    x, B = _x(shape), _blob(shape, SEED_B)
    fresh = _fresh_state(engine, shape, p, SEED_B)
    src, dst = _create(engine, shape, q1), _create(engine, shape, q2)
    try:
        src.load_weights_device(_dev(B))
        _copy_weights(dst, src)
        dst.set_precision(p)
        _check(dst, fresh, B, x, ("broadcast receiver",))
        src.set_precision(p)
        _check(src, fresh, B, x, ("broadcast source",))
    finally:
        src.close()
        dst.close()


@pytest.mark.gpu
def test_gpu_device_load_arguments(engine):
    """7: a wrong count and a null pointer are AZ_ERR_ARG and leave the net as it was; a CPU tensor, a wrong
    dtype, a wrong size and a non-contiguous tensor raise ValueError before the engine is called."""
    from az_amd import _lib
    shape = "f32only"
    x, B = _x(shape), _blob(shape, SEED_B)
    fresh = _fresh_state(engine, shape, F32, SEED_B)
    net = _create(engine, shape, F32)
    try:
        net.load_weights(B)
        n = net.num_params
        t = _dev(_blob(shape, SEED_A))
        f = _lib.lib().az_net_load_weights_device
        assert f(net.h, ctypes.c_void_p(t.data_ptr()), n - 1) == _lib.AZ_ERR_ARG
        assert f(net.h, ctypes.c_void_p(t.data_ptr()), n + 1) == _lib.AZ_ERR_ARG
        assert f(net.h, None, n) == _lib.AZ_ERR_ARG
        assert f(None, ctypes.c_void_p(t.data_ptr()), n) == _lib.AZ_ERR_ARG
        wide = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
        for bad in (t.cpu(), t.double(), t[:-1], wide[::2], torch.zeros(n + 1, dtype=torch.float32, device="cuda"),
                    np.array(B)):
            with pytest.raises(ValueError):
                net.load_weights_device(bad)
        _check(net, fresh, B, x, ("after refused loads",))
    finally:
        net.close()


class _Net(torch.nn.Module):
    """The plain residual net of oracle/net_oracle.py as a torch module; its state_dict is in blob order."""

    def __init__(self, d):
        super().__init__()
        nn = torch.nn
        Fc, HC, PP = d.channels, d.head_channels, d.pool * d.pool
        self.pool = d.pool
        self.input_conv = nn.Conv2d(d.in_planes, Fc, 3, padding=1, bias=False)
        self.input_bn = nn.BatchNorm2d(Fc)
        self.blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(Fc, Fc, 3, padding=1, bias=False), nn.BatchNorm2d(Fc), nn.ReLU(),
                                                   nn.Conv2d(Fc, Fc, 3, padding=1, bias=False), nn.BatchNorm2d(Fc))
                                     for _ in range(d.blocks)])
        self.policy_conv = nn.Conv2d(Fc, HC, 1, bias=False)
        self.policy_bn = nn.BatchNorm2d(HC)
        self.policy_fc = nn.Linear(HC * PP, d.action_size)
        self.value_conv = nn.Conv2d(Fc, HC, 1, bias=False)
        self.value_bn = nn.BatchNorm2d(HC)
        self.value_fc1 = nn.Linear(HC * PP, d.fc_hidden)
        self.value_fc2 = nn.Linear(d.fc_hidden, 1)

    def forward(self, x):
        Fn = torch.nn.functional
        x = torch.relu(self.input_bn(self.input_conv(x)))
        for b in self.blocks:
            x = torch.relu(b(x) + x)
        x = Fn.adaptive_avg_pool2d(x, (self.pool, self.pool))
        pol = self.policy_fc(torch.relu(self.policy_bn(self.policy_conv(x))).flatten(1))
        v = torch.relu(self.value_fc1(torch.relu(self.value_bn(self.value_conv(x))).flatten(1)))
        return pol, torch.tanh(self.value_fc2(v)).reshape(-1)


@pytest.mark.gpu
def test_gpu_closed_loop_selfplay_train_publish(engine):
    """8: self-play fills the device ring, a torch module takes two SGD steps on sampled batches, its
    state_dict goes back through state_dict_blob and load_weights_device: the engine then computes the
    trained module (the fp32 oracle on the published blob at the F32 bound of tests/test_gpu_net.py, 1e-4)
    and exactly what a fresh host-loaded net computes."""
    import az_amd
    import net_oracle
    bs, G, N = 9, 8, 32
    desc = az_amd.gomoku_net_desc(board_size=bs, channels=16, blocks=1, precision=F32, max_batch=G)
    net = az_amd.HipNeuralNetwork(engine, desc)
    mgr = rb = fresh = None
    try:
        torch.manual_seed(0)
        model = _Net(desc).cuda()
        blob0 = az_amd.state_dict_blob(model.state_dict())
        assert blob0.is_cuda and blob0.numel() == net.num_params
        assert [k for k in model.state_dict() if not k.endswith("num_batches_tracked")] == \
            [name for name, *_ in net_oracle.param_shapes(desc)]
        net.load_weights_device(blob0)
        hb0 = blob0.cpu().numpy()
        rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, bs, 1024, 6)
        mgr = az_amd.SelfPlayManager(engine, net=net, numGames=G, numSimulations=16, board_size=bs, noise_seed=42,
                                     noise_seed_stride=1)
        mgr.mcts.attachReplay(rb)
        mgr.generateGames(G, max_moves=6)
        assert rb.info()["committed"] >= N, rb.info()
        st = torch.empty((N, rb.C, bs, bs), dtype=torch.float32, device="cuda")
        po = torch.empty((N, rb.NA), dtype=torch.float32, device="cuda")
        z = torch.empty(N, dtype=torch.float32, device="cuda")
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        model.train()
        with torch.backends.cudnn.flags(enabled=False):     # the framework's own kernels: no autotuning in a test
            for _ in range(2):
                rb.sample_into(st, po, z)
                logits, v = model(st)
                loss = -(po * torch.log_softmax(logits, 1)).sum(1).mean() + ((v - z) ** 2).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
        blob = az_amd.state_dict_blob(model.state_dict(), out=blob0)
        assert blob is blob0
        net.load_weights_device(blob)
        hb = blob.cpu().numpy()
        assert not np.array_equal(hb, hb0) and np.isfinite(hb).all()
        rb.sample_into(st[:G], po[:G])
        xs = st[:G].cpu().numpy()
        lo, val = net.forward(xs)
        rl, rv = net_oracle.forward(desc, hb, xs)
        el, ev = float(np.abs(lo - rl).max()), float(np.abs(val - rv).max())
        print(f"closed loop: max|dlogit|={el:.3e} max|dvalue|={ev:.3e}")
        assert el <= TOL and ev <= TOL, (el, ev)
        fresh = az_amd.HipNeuralNetwork(engine, desc)
        fresh.load_weights(hb)
        fl, fv = fresh.forward(xs)
        assert np.array_equal(fl, lo) and np.array_equal(fv, val)
        assert np.array_equal(net.get_weights(), hb)
    finally:
        if mgr is not None:
            mgr.mcts.close()
        if rb is not None:
            rb.close()
        if fresh is not None:
            fresh.close()
        net.close()


@pytest.mark.gpu
def test_gpu_host_network_load_weights_device():
    """The C++ surface (nn::HipNeuralNetwork::loadWeightsDevice through _alphazero_cpp): a blob published from
    a device pointer gives predictBatch bit for bit what loadWeights of the same values gives."""
    import _alphazero_cpp as az
    bs, _, ch, blocks, Bn, _ = SHAPES["small"]
    blob = np.array(_blob("small", SEED_B))
    t = _dev(blob)
    torch.cuda.synchronize()
    states = []
    rng = np.random.default_rng(4)
    for i in range(Bn):
        s = az.GomokuState(bs)
        for _ in range(i * 5):
            s.makeMove(int(rng.choice(s.getLegalMoves())))
        states.append(s)
    outs = []
    for route in ("device", "host"):
        net = az.HipNeuralNetwork(boardSize=bs, channels=ch, blocks=blocks, precision=F16X3, maxBatch=Bn)
        if route == "device":
            with pytest.raises(RuntimeError):
                net.loadWeightsDevice(t.data_ptr(), blob.size - 1)
            net.loadWeightsDevice(t.data_ptr(), blob.size)
        else:
            net.loadWeights(blob)
        pol, val = net.predictBatch(states)
        outs.append((np.asarray(pol, np.float32), np.asarray(val, np.float32)))
        del net
    assert np.isfinite(outs[0][0]).all() and outs[0][0].max() > 0
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
