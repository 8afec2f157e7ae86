"""Per-slot nets on one search handle (az_search_set_slot_nets; search_host.hip eval_slot_nets, tree_kernels.hip
k_scan_nets): every simulation step partitions its leaf batch by net -- net k owns rows [k * G, (k + 1) * G) of the
batch buffers -- and runs one forward per net.  What a slot plays must be bit for bit what it plays on a
single-net handle with its own net (the nets' outputs do not depend on the batch position,
test_gpu_net_partial_batch.py), so every check here is an equality of bit patterns against single-net handles."""
import numpy as np
import pytest

from replay_util import root_record


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def make_net(engine, game, bs, ch, blocks, prec, max_batch, seed):
    import az_amd
    import net_oracle
    go = game == "go"
    p = {"f32": az_amd.AZ_PREC_F32, "fp16": az_amd.AZ_PREC_FP16}[prec]
    desc = az_amd.NetDesc(bs, 8 if go else 11, ch, blocks, bs * bs + (1 if go else 0), 32, 8, 256, 1, 0, p, max_batch)
    net = az_amd.HipNeuralNetwork(engine, desc)
    net.load_weights(net_oracle.init_blob(desc, seed=seed))
    return net


def make_search(engine, net, G, bs, sims, go=False, **kw):
    import az_amd
    return az_amd.ParallelMCTS(engine, n_games=G, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                               net=net, noise_seed=42, noise_seed_stride=1,
                               game=az_amd.AZ_GAME_GO if go else az_amd.AZ_GAME_GOMOKU, **kw)


def play_ply(m, slots, noise_after):
    """search + select + the roots of `slots` + the move (+ noise): ({slot: root_record}, actions)."""
    m.search()
    act, val, probs, cact, nch = m.select(True, 1.0)
    roots = {g: root_record(m, g, act, val, probs, nch) for g in slots}
    m.updateWithMove(act)
    if noise_after:
        m.addDirichletNoise(0.03, 0.25)
    return roots, act


G, SLOT_NET, SIMS, PLIES = 8, [0, 1, 1, 0, 1, 0, 0, 1], 24, 3
# id: (game, board, channels, blocks, precision, input stage of net_input_path)
CASES = {
    "gemm-f32":   ("gomoku", 7, 32, 2, "f32"),      # NET_IN_GEMM: az_launch_rec_planes into the region's plane batch
    "small-fp16": ("gomoku", 15, 64, 1, "fp16"),    # NET_IN_SMALL: k_smallnet reads the region's leaf records
    "g8-15-fp16": ("gomoku", 15, 128, 1, "fp16"),   # NET_IN_G8: az_launch_rec_to_g8 on the region's records
    "g8-go-fp16": ("go", 9, 128, 1, "fp16"),        # NET_IN_G8, Go records
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_slot_nets_routing_parity(engine, case):
    """Two nets of one shape and different weights behind one handle of 8 slots: after every ply every slot's
    root equals the same slot of a single-net handle that plays all 8 slots with that slot's net; the logged
    evaluations of one slot per net are bitwise a dense forward on the slot's own net and differ on the other."""
    game, bs, ch, blocks, prec = CASES[case]
    go = game == "go"
    nets = [make_net(engine, game, bs, ch, blocks, prec, G, seed) for seed in (9, 10)]
    hs = []
    try:
        m = make_search(engine, nets[0], G, bs, SIMS, go)
        hs.append(m)
        ctl = [make_search(engine, n, G, bs, SIMS, go) for n in nets]
        hs += ctl
        m.setSlotNets(nets, SLOT_NET)
        cap = SIMS + 2
        logged = [0, 1, 3]          # per ply: a slot of net 0, of net 1, of net 0
        for h in hs:
            h.newGames()
            h.addDirichletNoise(0.03, 0.25)
        n_logged = [0, 0]
        for ply in range(PLIES):
            lg = logged[ply]
            m.enableEvalLog(lg, cap)
            roots, _ = play_ply(m, range(G), ply % 2 == 0)
            want = [play_ply(c, range(G), ply % 2 == 0)[0] for c in ctl]
            for g in range(G):
                assert roots[g] == want[SLOT_NET[g]][g], (ply, g)
            pol, val, planes = m.readEvalLog(cap)
            if len(pol) == 0:       # a finished Go game evaluates nothing
                assert go and ply > 0
                continue
            own, other = nets[SLOT_NET[lg]], nets[1 - SLOT_NET[lg]]
            dense = {}
            for name, n in (("own", own), ("other", other)):
                pv = [n.predictBatch(planes[i:i + G]) for i in range(0, len(planes), G)]
                dense[name] = (np.concatenate([p for p, _ in pv]), np.concatenate([v for _, v in pv]))
            same_v = dense["own"][1].view(np.uint32) == val.view(np.uint32)
            same_p = (dense["own"][0].view(np.uint32) == pol.view(np.uint32)).all(axis=1)
            oth_v = dense["other"][1].view(np.uint32) == val.view(np.uint32)
            oth_p = (dense["other"][0].view(np.uint32) == pol.view(np.uint32)).all(axis=1)
            print(f"slot nets {case} ply {ply} slot {lg} (net {SLOT_NET[lg]}): {len(pol)} evaluations, "
                  f"{int(same_v.sum())} values / {int(same_p.sum())} policies bitwise the own net's dense forward, "
                  f"{int(oth_v.sum())} / {int(oth_p.sum())} the other net's")
            assert same_v.all() and same_p.all(), (ply, np.flatnonzero(~same_v).tolist(), np.flatnonzero(~same_p).tolist())
            assert not oth_v.any() and not oth_p.any(), (ply, "the other net gives the logged outputs")
            n_logged[SLOT_NET[lg]] += len(pol)
        assert n_logged[0] > 0 and n_logged[1] > 0, n_logged
    finally:
        for h in hs:
            h.close()
        for n in nets:
            n.close()


BIG_G = 1100
STARTED = sorted({0, 5, 1023, 1024, 1099} | set(range(0, BIG_G, 7)))


@pytest.fixture(scope="module")
def edge_nets(engine):
    nets = [make_net(engine, "gomoku", 7, 32, 1, "f32", BIG_G, seed) for seed in (9, 10, 11)]
    yield nets
    for n in nets:
        n.close()


@pytest.fixture(scope="module")
def edge_control(engine, edge_nets):
    """The started slots on a single-net handle of 1100 slots, once per net: {net: ({slot: root}, {slot: evals})}."""
    small = dict(tt_log2=8, node_capacity=1024, prior_ring=4096)
    c = make_search(engine, edge_nets[0], BIG_G, 7, 4, **small)
    out = {}
    try:
        for k, n in enumerate(edge_nets):
            c.setNet(n)
            c.newGames(STARTED)
            e0 = {g: c.counters(g)["evals"] for g in STARTED}
            c.addDirichletNoise(0.03, 0.25)
            roots, _ = play_ply(c, STARTED, False)
            out[k] = (roots, {g: c.counters(g)["evals"] - e0[g] for g in STARTED})
    finally:
        c.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["mod3", "all-on-net-2"])
def test_gpu_slot_nets_partition_edges(engine, edge_nets, edge_control, layout):
    """1100 slots (more than one slot per scan thread), three nets, a sparse set of started slots that holds
    the first and last slot and both sides of the 1024 boundary; in the second layout every started slot
    belongs to net 2, so nets 0 and 1 have slots assigned and no leaf in any step."""
    small = dict(tt_log2=8, node_capacity=1024, prior_ring=4096)
    if layout == "mod3":
        slot_net = [g % 3 for g in range(BIG_G)]
    else:
        started = set(STARTED)
        slot_net = [2 if g in started else g % 2 for g in range(BIG_G)]
    assert all(slot_net.count(k) > 0 for k in range(3))
    m = make_search(engine, edge_nets[0], BIG_G, 7, 4, **small)
    try:
        m.setSlotNets(edge_nets, slot_net)
        m.newGames(STARTED)
        m.addDirichletNoise(0.03, 0.25)
        roots, act = play_ply(m, STARTED, False)
        idle = [g for g in range(BIG_G) if g not in set(STARTED)]
        assert (act[idle] == m.none).all()
        for g in STARTED:
            want_roots, want_evals = edge_control[slot_net[g]]
            assert roots[g] == want_roots[g], g
            assert m.counters(g)["evals"] == want_evals[g] > 0, g
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_slot_nets_single_slot(engine, edge_nets):
    """G = 1, two nets, the slot on net 1: net 0 has no slot and never runs."""
    small = dict(tt_log2=8, node_capacity=1024, prior_ring=4096)
    m = make_search(engine, edge_nets[0], 1, 7, 4, **small)
    c = make_search(engine, edge_nets[1], 1, 7, 4, **small)
    try:
        m.setSlotNets(edge_nets[:2], [1])
        for h in (m, c):
            h.newGames()
            h.addDirichletNoise(0.03, 0.25)
        for ply in range(2):
            assert play_ply(m, [0], True)[0] == play_ply(c, [0], True)[0], ply
        assert m.counters(0) == c.counters(0)
    finally:
        m.close()
        c.close()


@pytest.mark.gpu
def test_gpu_slot_nets_contract(engine):
    """Refused calls return the documented code and leave the handle playing as before; az_search_set_net after
    setSlotNets returns every slot to the one net."""
    import az_amd
    from az_amd._lib import AZ_ERR_ARG, AZ_ERR_STATE
    small = dict(tt_log2=8, node_capacity=4096, prior_ring=8192)
    a, b = (make_net(engine, "gomoku", 7, 32, 1, "f32", 4, seed) for seed in (9, 10))
    tiny = make_net(engine, "gomoku", 7, 32, 1, "f32", 1, 10)         # max_batch 1
    other = make_net(engine, "gomoku", 9, 32, 1, "f32", 4, 10)        # another board
    m = make_search(engine, a, 4, 7, 8, **small)
    c = make_search(engine, a, 4, 7, 8, **small)
    h = az_amd.ParallelMCTS(engine, n_games=4, board_size=7, num_simulations=8, evaluator=az_amd.AZ_EVAL_HASH, **small)
    try:
        for s in (m, c):
            s.newGames()
            s.addDirichletNoise(0.03, 0.25)
        assert play_ply(m, range(4), True)[0] == play_ply(c, range(4), True)[0]
        refused = [
            (m, [a, b, a, b, a], [0, 1, 2, 3], AZ_ERR_ARG),      # n_nets = 5
            (m, [a, other], [0, 1, 0, 1], AZ_ERR_ARG),           # a net of another board
            (m, [a, tiny], [0, 1, 1, 0], AZ_ERR_ARG),            # max_batch one below its two slots
            (m, [a, b], [0, 1, 2, 0], AZ_ERR_ARG),               # an index >= n_nets
            (h, [a, b], [0, 1, 0, 1], AZ_ERR_STATE),             # not an AZ_EVAL_NET handle
        ]
        for s, nets, sn, code in refused:
            with pytest.raises(az_amd.AzError) as ei:
                s.setSlotNets(nets, sn)
            assert ei.value.code == code, (ei.value, code)
        assert play_ply(m, range(4), True)[0] == play_ply(c, range(4), True)[0]
        # two nets, then one again: from fresh games the handle plays what the single-net control plays
        m.setSlotNets([a, b], [0, 1, 0, 1])
        split, _ = play_ply(m, range(4), True)
        ctl, _ = play_ply(c, range(4), True)
        assert split[0] == ctl[0] and split[2] == ctl[2]                 # net A's slots, as before
        assert split[1] != ctl[1] and split[3] != ctl[3]                 # net B's slots see other priors
        m.setNet(a)
        for s in (m, c):
            s.newGames()
            s.addDirichletNoise(0.03, 0.25)
        for ply in range(2):
            assert play_ply(m, range(4), True)[0] == play_ply(c, range(4), True)[0], ply
    finally:
        for s in (m, c, h):
            s.close()
        for n in (a, b, tiny, other):
            n.close()
