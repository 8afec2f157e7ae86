"""Leaf-parallel search on the device (az_search_set_leaves: K descents per game and simulation step, one
evaluator batch of up to G x K leaves) against the wave schedule derived from the CPU restatement
(tests/wave_model.cpp).  Bit-exact as tests/test_gpu_search.py: raw N / VL, fp32 bits of W, P, visit
distributions and root values, actions, TT lookup / hit counters and evaluation counts."""
import ctypes

import numpy as np
import pytest

import az_oracle as O
import wave_cases
import wave_model as W
from replay_util import bits, compare_roots, root_record
from test_gpu_search import children_rows, play_and_compare

DEV_EVAL = {O.EVAL_HASH: "AZ_EVAL_HASH", O.EVAL_RANDOM: "AZ_EVAL_RANDOM", O.EVAL_UNIFORM: "AZ_EVAL_UNIFORM"}


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def make(engine, kw, leaves=1, **more):
    import az_amd
    return az_amd.ParallelMCTS(engine, n_games=kw.get("n_games", 1), board_size=kw["bs"], num_simulations=kw["sims"],
                               evaluator=getattr(az_amd, DEV_EVAL[kw["eval_kind"]]), eval_seed=kw.get("eval_seed", 7),
                               noise_seed=42, noise_seed_stride=kw.get("seed_stride", 0), tt_log2=kw.get("tt_log2", 20),
                               game=kw.get("game", 0), leaves=leaves, **more)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(wave_cases.CASES))
def test_gpu_wave_matches_model(engine, case):
    K, kw, _ = wave_cases.CASES[case]
    refs = W.play(K, **kw)
    m = make(engine, kw, leaves=K)
    try:
        assert m.getLeafParallelism() == K
        play_and_compare(m, refs, kw.get("n_games", 1), kw.get("max_moves"))
    finally:
        m.close()


def one_ply(m, ref_move, g=0):
    """One search + move of a single-game handle against a model move (play_and_compare's checks)."""
    m.search()
    act, val, probs, cact, nch = m.select(True, 1.0)
    N, VL, Wr = m.rootNode(g)
    assert [N, VL, bits([Wr])[0]] == ref_move["root"]
    assert children_rows(m, g) == ref_move["children"]
    assert bits(probs[g, :nch[g]]) == ref_move["probs"]
    assert int(act[g]) == ref_move["action"] and bits([val[g]])[0] == ref_move["value"]
    c = m.counters(g)
    assert (c["tt_lookups"], c["tt_hits"], c["evals"]) == (ref_move["tt_lookups"], ref_move["tt_hits"], ref_move["evals"])
    m.updateWithMove(act)


@pytest.mark.gpu
def test_gpu_wave_k_changes_between_searches(engine):
    """K = 1, 4, 1, 8 over four plies with the tree kept, then K = 1 again for two more: every ply against the
    model's per-ply list.  The K = 1 plies are the plain search (Search::simulate) continuing from the tree the
    waves left; ply 0 is also az_oracle.play's."""
    kw = dict(bs=6, sims=64, eval_kind=O.EVAL_HASH)
    ks = [1, 4, 1, 8, 1, 1]
    ref = W.play(ks, max_moves=len(ks), **kw)[0]
    assert ref["moves"][0] == O.play(max_moves=1, **kw)[0]["moves"][0]
    m = make(engine, kw)
    try:
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        assert children_rows(m, 0) == ref["init_root"]
        for ply, K in enumerate(ks):
            m.setLeafParallelism(K)
            assert m.getLeafParallelism() == K
            one_ply(m, ref["moves"][ply])
            if ply % 2 == 0:
                m.addDirichletNoise(0.03, 0.25)
    finally:
        m.close()


def wave_replay(K, pol, val, planes, n_moves, **search):
    """replay_util.replay_eval_log under the wave schedule: the model replays the logged evaluations of game 0,
    asking for exactly the logged planes in the logged order, and must consume the whole log."""
    k, bad = [0], []

    def replay(game, x):
        i = k[0]
        if i >= len(pol):
            bad.append(f"the model asks for evaluation {i}, the log holds {len(pol)}")
            raise O.StopPlay()
        if not np.array_equal(x, planes[i]):
            bad.append(f"feature planes differ at evaluation {i}")
            raise O.StopPlay()
        k[0] += 1
        return pol[i], float(val[i])

    r = W.play(K, eval_kind=O.EVAL_REPLAY, evaluator=replay, noise_seed=42, max_moves=n_moves, **search)
    assert not bad and r is not None, bad
    assert k[0] == len(pol), f"{len(pol)} logged evaluations, the model asked for {k[0]}"
    return r[0]


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["identity", "compacted"])
@pytest.mark.parametrize("prec,bs,ch,blocks", [("f32", 7, 32, 2), ("fp16", 9, 128, 1)], ids=["f32", "fp16"])
def test_gpu_wave_network_replay(engine, prec, bs, ch, blocks, masked):
    """7x7, 2 blocks x 32 filters in F32 (the fp16 trunk takes no 7x7 board or 32 filters: its run is 9x9, one
    block of 128), max_batch 16 = G x K: game 0's evaluations are logged and replayed through the model
    (consumed evaluations only, in completion order); planes, N / VL / W / P, probs, action and value bitwise.
    masked: slot 2 sits every search out (az_search_run_masked), so the compacted G x K batch runs."""
    import az_amd
    import net_oracle
    G, K, sims, moves = 4, 4, 32, 5
    p = az_amd.AZ_PREC_F32 if prec == "f32" else az_amd.AZ_PREC_FP16
    desc = az_amd.NetDesc(bs, 11, ch, blocks, bs * bs, 32, 8, 256, 1, 0, p, G * K)
    net = az_amd.HipNeuralNetwork(engine, desc)
    m = None
    try:
        net.load_weights(net_oracle.init_blob(desc, seed=9))
        m = az_amd.ParallelMCTS(engine, n_games=G, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                                net=net, noise_seed=42, noise_seed_stride=1, leaves=K)
        cap = (sims + 2) * (moves + 1)
        m.enableEvalLog(0, cap)
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        mask = np.array([1, 1, 0, 1], np.uint8) if masked else None
        dev = []
        for ply in range(moves):
            m.search(mask)
            act, val, probs, cact, nch = m.select(True, 1.0, mask)
            dev.append(root_record(m, 0, act, val, probs, nch))
            m.updateWithMove(act)
            if ply % 2 == 0:
                m.addDirichletNoise(0.03, 0.25, mask)
        pol, valv, planes = m.readEvalLog(cap)
        evals = m.counters(0)["evals"]
    finally:
        if m is not None:
            m.close()
        net.close()
    assert 0 < len(pol) < cap and evals == len(pol)
    ref = wave_replay(K, pol, valv, planes, moves, bs=bs, sims=sims)
    compare_roots(dev, ref["moves"])


@pytest.mark.gpu
def test_gpu_wave_selfplay_step_matches_model(engine):
    """az_selfplay_step at K = 4 on 4 slots of 6x6 for 40 moves: games end and slots restart as the next game
    id; every MoveData against the model's record of the game id its slot plays."""
    bs, sims, steps, total, slots, K = 6, 48, 40, 16, 4, 4
    kw = dict(bs=bs, sims=sims, eval_kind=O.EVAL_HASH, n_games=total, seed_stride=1)
    refs = W.play(K, **kw)
    m = make(engine, dict(kw, n_games=slots), leaves=K)
    gid, ply, nxt, restarts = list(range(slots)), [0] * slots, slots, 0
    try:
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        for step in range(steps):
            mv, _ = m.selfplayStep()
            recs = m.stepMoves(materialize=True)
            assert mv == len(recs) == slots, step
            for s, md in recs:
                assert gid[s] < total, "more games than the model played"
                rm = refs[gid[s]]["moves"][ply[s]]
                where = (step, s, gid[s], ply[s])
                assert md.action == rm["action"], where
                assert bits(md.policy) == rm["probs"], where
                assert bits([md.value])[0] == rm["value"], where
                assert list(md.child_actions) == [r[0] for r in rm["children"]], where
                ply[s] += 1
            for s in range(slots):
                if ply[s] == len(refs[gid[s]]["moves"]):
                    assert refs[gid[s]]["terminal"], gid[s]
                    gid[s], ply[s], nxt = nxt, 0, nxt + 1
                    restarts += 1
    finally:
        m.close()
    assert restarts >= 1


@pytest.mark.gpu
def test_gpu_wave_guards(engine):
    """Every AZ_ERR_ARG of az_search_set_leaves, in both orders; a refused call leaves the handle playing, its
    next search bit-equal to the model."""
    import az_amd
    import net_oracle
    from az_amd import _lib
    lib = _lib.lib
    kw = dict(bs=6, sims=32, eval_kind=O.EVAL_HASH)
    ref = W.play([4], max_moves=2, **kw)[0]

    def refused(fn, *words):
        with pytest.raises(az_amd.AzError) as e:
            fn()
        assert e.value.code == _lib.AZ_ERR_ARG, str(e.value)
        for w in words:
            assert str(w) in str(e.value), (w, str(e.value))

    m = make(engine, kw, leaves=4)
    try:
        # the range, naming the numbers
        refused(lambda: m.setLeafParallelism(0), 0, 32)
        refused(lambda: m.setLeafParallelism(33), 33, 32)
        assert az_amd.AZ_MAX_LEAVES == 32 and m.getLeafParallelism() == 4
        # K > 1 first, then what the wave model cannot pin
        refused(lambda: m.setSearchOptions(use_td=True), 4)
        refused(lambda: m.setSearchOptions(selection=az_amd.AZ_SEL_UCB), 4)
        refused(lambda: m.setSearchOptions(max_search_depth=3), 4)
        refused(lambda: m.setSearchOptions(use_widening=True), 4)
        m.setSearchOptions(selection=az_amd.AZ_SEL_RAVE)          # plays PUCT: a default search, allowed
        m.setSearchOptions(selection=az_amd.AZ_SEL_PUCT)
        refused(lambda: az_amd.check(lib().az_search_set_gomoku_rules(m.h, ctypes.byref(az_amd.GomokuRules(1, 0, 0)))), 4)
        assert m.searchOptions()["use_td"] is False and m.gomokuRules() == (False, False)
        # after the refusals the handle plays the model's game
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        assert children_rows(m, 0) == ref["init_root"]
        one_ply(m, ref["moves"][0])
        m.addDirichletNoise(0.03, 0.25)
        refused(lambda: m.setLeafParallelism(64), 64)
        one_ply(m, ref["moves"][1])
    finally:
        m.close()
    # the other order: options / rules first, then K > 1; K = 1 stays allowed
    for more in (dict(use_td=True), dict(max_search_depth=4), dict(gomoku_renju=True), dict(gomoku_omok=True)):
        h = make(engine, kw, **more)
        try:
            refused(lambda: h.setLeafParallelism(2), 2)
            h.setLeafParallelism(1)
            assert h.getLeafParallelism() == 1
        finally:
            h.close()
    with pytest.raises(az_amd.AzError):
        make(engine, kw, leaves=2, use_td=True)
    # the host-callback evaluator
    cb = az_amd.ParallelMCTS(engine, n_games=1, board_size=6, num_simulations=8, evaluator=az_amd.AZ_EVAL_CALLBACK,
                             callback=lambda g, mv, x: (np.full((len(g), 36), 1 / 36, np.float32), np.zeros(len(g), np.float32)))
    try:
        refused(lambda: cb.setLeafParallelism(2), 2)
    finally:
        cb.close()
    # the net's batch capacity: max_batch = G x K - 1, at creation order and through az_search_set_net; per-slot nets
    bs, G, K = 6, 2, 4
    mk = lambda mb: az_amd.HipNeuralNetwork(engine, az_amd.NetDesc(bs, 11, 32, 1, bs * bs, 32, 8, 256, 1, 0, az_amd.AZ_PREC_F32, mb))
    small, full = mk(G * K - 1), mk(G * K)
    n = None
    try:
        for net in (small, full):
            net.load_weights(net_oracle.init_blob(net.desc, seed=3))
        n = az_amd.ParallelMCTS(engine, n_games=G, board_size=bs, num_simulations=16, evaluator=az_amd.AZ_EVAL_NET, net=small)
        refused(lambda: n.setLeafParallelism(K), G * K - 1, G, K)
        assert n.getLeafParallelism() == 1
        n.setLeafParallelism(K - 1)                               # G x (K - 1) = 6 <= 7 rows
        n.setLeafParallelism(1)
        n.setNet(full)
        n.setLeafParallelism(K)
        refused(lambda: n.setNet(small), G * K - 1, G, K)
        refused(lambda: n.setSlotNets([full, full], [0, 1]), K)
        n.newGames()
        n.addDirichletNoise(0.03, 0.25)
        n.search()                                                # still plays, on the full net
        assert all(c > 0 for c in n.select(True, 1.0)[4])
        n.setLeafParallelism(1)
        n.setSlotNets([full, full], [0, 1])
        refused(lambda: n.setLeafParallelism(2), 2)
    finally:
        if n is not None:
            n.close()
        small.close()
        full.close()
