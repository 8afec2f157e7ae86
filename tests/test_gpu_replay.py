"""The device replay buffer (az_replay_*, az_amd.ReplayBuffer) on the GPU.  Every check is bit- or integer-exact;
expected values come from the CPU restatement (az_oracle.play: the root children's visit counts, root values,
results), the leaf-parallel model (tests/wave_model.py), the reference's golden games and the host GomokuState /
GoState (feature planes), never from the buffer itself."""
import ctypes

import numpy as np
import pytest
import torch    # before libaz_hip.so is loaded: the engine and torch then share one HIP runtime (sample_into)

BS, SIMS, SLOTS, STEPS, TOTAL = 6, 48, 3, 70, 24      # the shape of test_gpu_selfplay_step_matches_oracle


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


@pytest.fixture(scope="module")
def refs():
    import az_oracle as O
    return O.play(seed_stride=1, bs=BS, sims=SIMS, eval_kind=O.EVAL_HASH, eval_seed=5, n_games=TOTAL)


def schedule(lengths, slots, steps=None, total=None, max_moves=0):
    """The positions a driver stages, step by step: slot s plays game gid[s]; every playing slot moves once per step;
    a game ends after lengths[gid] plies or is cut at max_moves; finished slots take the next ids in slot order
    (while ids remain, when `total` is given).  Returns (games finished in commit order, [(gid, plies played)] of the
    games still running)."""
    n0 = slots if total is None else min(slots, total)
    gid = list(range(n0)) + [None] * (slots - n0)
    ply = [0] * slots
    nxt, done, step = n0, [], 0
    while any(g is not None for g in gid) and (steps is None or step < steps):
        step += 1
        fin = []
        for s in range(slots):
            if gid[s] is None:
                continue
            ply[s] += 1
            if ply[s] == lengths[gid[s]] or (max_moves and ply[s] >= max_moves):
                fin.append(s)
        for s in fin:
            done.append((gid[s], ply[s]))
            gid[s], ply[s] = None, 0
        for s in fin:
            if total is None or nxt < total:
                gid[s], nxt = nxt, nxt + 1
    return done, [(gid[s], ply[s]) for s in range(slots) if gid[s] is not None]


def expected_rows(refs, done, NA, first=None):
    """Per committed position, in commit order: (gid, ply, counts [NA], sum, value bits, z)."""
    rows = []
    for gid, n in done:
        g = refs[gid]
        for ply in range(n if first is None else min(n, first)):
            mv = g["moves"][ply]
            c = np.zeros(NA, np.int32)
            for a, N, *_ in mv["children"]:
                c[NA - 1 if a < 0 else a] = max(0, N)
            finished = g["terminal"] and n == len(g["moves"])
            res = g["result"] if finished else 0
            z = 0.0 if res in (0, 1) else (1.0 if (res == 2) == (ply % 2 == 0) else -1.0)
            rows.append((gid, ply, c, int(c.sum()), mv["value"], z))
    return rows


def check_rows(rb, idx, rows):
    out = rb.gather(idx)
    cnt, sm = rb.counts(idx)
    assert out["game_id"].tolist() == [r[0] for r in rows]
    assert out["ply"].tolist() == [r[1] for r in rows]
    for i, (gid, ply, c, s, vbits, z) in enumerate(rows):
        where = (i, gid, ply)
        assert np.array_equal(cnt[i], c), where
        assert int(sm[i]) == s and s > 0, where
        assert np.array_equal(out["policy"][i], c.astype(np.float32) / np.float32(s)), where
        assert bits([out["q"][i]])[0] == vbits, where
        assert float(out["z"][i]) == z, where
    return out


def run_steps(engine, capacity, max_plies, steps=STEPS):
    import az_amd
    m = az_amd.ParallelMCTS(engine, n_games=SLOTS, board_size=BS, num_simulations=SIMS, evaluator=az_amd.AZ_EVAL_HASH,
                            eval_seed=5, noise_seed=42, noise_seed_stride=1)
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, BS, capacity, max_plies)
    try:
        m.attachReplay(rb)
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        for _ in range(steps):
            mv, _ev = m.selfplayStep()
            assert mv == SLOTS
    except BaseException:
        rb.close()
        raise
    finally:
        m.close()                      # the buffer outlives its search handle
    return rb


@pytest.fixture(scope="module")
def filled(engine, refs):
    """The run of test 1, shared by the tests that only read the ring."""
    rb = run_steps(engine, 4096, 36)
    lengths = [len(g["moves"]) for g in refs]
    done, running = schedule(lengths, SLOTS, steps=STEPS)
    yield rb, done, running
    rb.close()


@pytest.mark.gpu
def test_gpu_replay_contents_match_oracle_through_restarts(filled, refs):
    """70 selfplaySteps on 3 slots with restarts: the ring holds exactly the finished games' plies in commit order
    (slot order within a step, ply order within a game) with the oracle's visit counts by action -- the T = 0 plies
    from 30 on included, where the record's child-order policy is NaN -- root values and outcomes."""
    import az_amd
    rb, done, running = filled
    assert len(done) >= 4 and max(n for _, n in done) > 30 and all(refs[g]["terminal"] for g, _ in done)
    rows = expected_rows(refs, done, BS * BS)
    info = rb.info()
    assert info == dict(committed=len(rows), total_committed=len(rows), games=len(done), dropped=0, skipped=0)
    check_rows(rb, np.arange(len(rows)), rows)
    assert any(np.isnan(np.asarray(refs[g]["moves"][n - 1]["probs"], np.uint32).view(np.float32)).any() for g, n in done)
    # nothing of the unfinished games
    assert running and not set(g for g, _ in running) & set(r[0] for r in rows)
    with pytest.raises(az_amd.AzError) as e:
        rb.gather([len(rows)])
    assert e.value.code == -1


def gomoku_planes(bs, moves, sym=0):
    import _alphazero_cpp as H
    import az_amd
    s = H.GomokuState(bs)
    for a in moves:
        s.makeMove(az_amd.replay_sym_cell(bs, sym, a))
    return np.asarray(s.getEnhancedTensorRepresentation(), np.float32).reshape(11, bs, bs)


@pytest.mark.gpu
def test_gpu_replay_planes_and_symmetries(filled, refs):
    """Identity gathers are the host GomokuState's planes after the game's first `ply` moves; under symmetry s they are
    the planes of the game whose every move was mapped by az_replay_sym_cell, and the policy is permuted by the map."""
    import az_amd
    rb, done, _ = filled
    rows = expected_rows(refs, done, BS * BS)
    n = len(rows)
    ident = rb.gather(np.arange(n))
    actions = {g: [mv["action"] for mv in refs[g]["moves"]] for g, _ in done}
    for i, (gid, ply, *_r) in enumerate(rows):
        assert np.array_equal(ident["states"][i], gomoku_planes(BS, actions[gid][:ply])), (gid, ply)
    pick = np.arange(24)                                       # the first game's plies 0..23
    assert rows[0][1] == 0 and rows[23][1] == 23 and rows[23][0] == rows[0][0]
    A = BS * BS
    for sym in range(8):
        out = rb.gather(pick, np.full(pick.size, sym, np.int32))
        cell = [az_amd.replay_sym_cell(BS, sym, a) for a in range(A)]
        for i in pick:
            gid, ply = rows[i][0], rows[i][1]
            assert np.array_equal(out["states"][i], gomoku_planes(BS, actions[gid][:ply], sym)), (sym, gid, ply)
            assert np.array_equal(out["policy"][i][cell], ident["policy"][i]), (sym, gid, ply)
            assert bits(out["q"][i:i + 1]) == bits(ident["q"][i:i + 1]) and out["z"][i] == ident["z"][i]
        if sym:
            assert not np.array_equal(out["states"][6], ident["states"][6])


def go_planes(bs, moves, sym=0):
    import _alphazero_cpp as H
    import az_amd
    s = H.GoState(bs)
    for a in moves:
        s.makeMove(a if a < 0 else az_amd.replay_sym_cell(bs, sym, a))
    return np.asarray(s.getEnhancedTensorRepresentation(), np.float32).reshape(8, bs, bs)


def go_check_planes(rb, rows, actions, bs, pick, syms, ident):
    import az_amd
    A = bs * bs
    for sym in syms:
        o = rb.gather(pick, np.full(len(pick), sym, np.int32))
        cell = [az_amd.replay_sym_cell(bs, sym, a) for a in range(A)] + [A]      # the pass stays
        for k, i in enumerate(pick):
            gid, ply = rows[i][0], rows[i][1]
            assert np.array_equal(o["states"][k], go_planes(bs, actions[gid][:ply], sym)), (sym, gid, ply)
            assert np.array_equal(o["policy"][k][cell], ident["policy"][i]), (sym, gid, ply)


@pytest.mark.gpu
def test_gpu_replay_go(engine):
    """Go 9x9, random evaluator, 30 simulations, az_selfplay_run with 3 games on 2 slots: counts with the pass at
    index 81, planes against the host GoState for the identity and two symmetries, outcomes.  These games end by two
    passes after two plies, so they hold no stone and no ko point, and the second run's max_moves = 6 cuts nothing;
    stones, liberties, a ko point and cut games are test_gpu_replay_go_stones_ko_and_cut_games'."""
    import az_amd
    import az_oracle as O
    bs, sims, total = 9, 30, 3
    grefs = O.play(seed_stride=1, bs=bs, sims=sims, eval_kind=O.EVAL_RANDOM, eval_seed=5, n_games=total, game=O.GAME_GO)
    lengths = [len(g["moves"]) for g in grefs]
    assert all(g["terminal"] for g in grefs)
    mgr = az_amd.SelfPlayManager(engine, numGames=2, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_RANDOM,
                                 eval_seed=5, noise_seed=42, noise_seed_stride=1, game=az_amd.AZ_GAME_GO)
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GO, bs, 4096, 2 * bs * bs)
    try:
        mgr.mcts.attachReplay(rb)
        actions = {g: [mv["action"] for mv in grefs[g]["moves"]] for g in range(total)}
        for max_moves in (0, 6):
            rb.clear()
            assert rb.info()["committed"] == 0
            recs = mgr.generateGames(totalGames=total, max_moves=max_moves)
            assert [len(r.moves) for r in recs] == lengths
            done, running = schedule(lengths, 2, total=total, max_moves=max_moves)
            assert not running and sorted(g for g, _ in done) == list(range(total))
            rows = expected_rows(grefs, done, bs * bs + 1)
            assert rb.info() == dict(committed=len(rows), total_committed=len(rows), games=total, dropped=0, skipped=0)
            out = check_rows(rb, np.arange(len(rows)), rows)
            assert any(r[2][bs * bs] > 0 for r in rows)                       # the pass was visited
            for i, (gid, ply, *_r) in enumerate(rows):
                assert np.array_equal(out["states"][i], go_planes(bs, actions[gid][:ply])), (gid, ply)
            go_check_planes(rb, rows, actions, bs, np.arange(len(rows)), (3, 6), out)
    finally:
        rb.close()
        mgr.mcts.close()


@pytest.mark.gpu
def test_gpu_replay_go_stones_ko_and_cut_games(engine):
    """Go 9x9 with the hash evaluator (120 simulations), two games cut at 46 plies: boards with stones, captures and
    ko points (the oracle's games have one before plies 41 and 44).  Liberties and the ko point against the host
    GoState under the identity and two symmetries, and z == 0 on every position of a cut game."""
    import az_amd
    import az_oracle as O
    bs, sims, total, mm = 9, 120, 2, 46
    grefs = O.play(seed_stride=1, bs=bs, sims=sims, eval_kind=O.EVAL_HASH, eval_seed=5, n_games=total, game=O.GAME_GO,
                   max_moves=mm)
    assert [len(g["moves"]) for g in grefs] == [mm] * total and not any(g["terminal"] for g in grefs)
    mgr = az_amd.SelfPlayManager(engine, numGames=total, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_HASH,
                                 eval_seed=5, noise_seed=42, noise_seed_stride=1, game=az_amd.AZ_GAME_GO)
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GO, bs, 256, mm)
    try:
        mgr.mcts.attachReplay(rb)
        mgr.generateGames(totalGames=total, max_moves=mm)
        rows = expected_rows(grefs, [(0, mm), (1, mm)], bs * bs + 1)
        assert rb.info() == dict(committed=total * mm, total_committed=total * mm, games=total, dropped=0, skipped=0)
        out = check_rows(rb, np.arange(len(rows)), rows)
        assert not out["z"].any()
        actions = {g: [mv["action"] for mv in grefs[g]["moves"]] for g in range(total)}
        for i, (gid, ply, *_r) in enumerate(rows):
            assert np.array_equal(out["states"][i], go_planes(bs, actions[gid][:ply])), (gid, ply)
        ko = [i for i, (gid, ply, *_r) in enumerate(rows) if O.go_position(bs, actions[gid][:ply])["ko"] >= 0]
        assert ko and all(out["states"][i][5].sum() == 1.0 for i in ko)
        pick = np.array(sorted(set(ko + [0, 1, mm - 1, 2 * mm - 1] + list(range(30, 40)))))
        go_check_planes(rb, rows, actions, bs, pick, (1, 4), out)
    finally:
        rb.close()
        mgr.mcts.close()


@pytest.mark.gpu
def test_gpu_replay_ring_wrap_and_staging_overflow(engine, refs):
    """The run of test 1 in a ring of 16: the ring is the last 16 committed positions at their wrapped rows.  Then a
    staging area of 3 plies: every game commits exactly its plies 0-2 and the rest count as dropped (the games still
    running at the end have dropped theirs too)."""
    import az_amd
    lengths = [len(g["moves"]) for g in refs]
    done, running = schedule(lengths, SLOTS, steps=STEPS)
    rows = expected_rows(refs, done, BS * BS)
    cap = 16
    rb = run_steps(engine, cap, 36)
    try:
        ring, head = [None] * cap, 0
        for r in rows:
            ring[head % cap] = r
            head += 1
        info = rb.info()
        assert info == dict(committed=cap, total_committed=len(rows), games=len(done), dropped=0, skipped=0)
        check_rows(rb, np.arange(cap), ring)
        with pytest.raises(az_amd.AzError):
            rb.gather([cap])
    finally:
        rb.close()
    rb = run_steps(engine, 4096, 3)
    try:
        rows3 = expected_rows(refs, done, BS * BS, first=3)
        info = rb.info()
        assert info["committed"] == len(rows3) == 3 * len(done) and info["games"] == len(done)
        assert info["dropped"] == sum(n - 3 for _, n in done) + sum(max(0, n - 3) for _, n in running)
        check_rows(rb, np.arange(len(rows3)), rows3)
    finally:
        rb.close()


@pytest.mark.gpu
def test_gpu_replay_sampling(filled):
    """sample = az_replay_sample_plan of (seed, call) + gather; the device form writes the same bytes."""
    import az_amd
    assert torch.cuda.is_available()
    rb, done, _ = filled
    committed = rb.info()["committed"]
    n, seed = 32, 0x5EED1234ABCD
    rb.seed(seed)
    host = [rb.sample(n, augment=True) for _ in range(2)]
    for call, s in enumerate(host):
        idx, sym = az_amd.replay_sample_plan(seed, call, n, committed, True)
        assert np.array_equal(s["idx"], idx) and np.array_equal(s["sym"], sym)
        g = rb.gather(idx, sym)
        for k in ("states", "policy", "z", "q"):
            assert np.array_equal(s[k].view(np.uint32), g[k].view(np.uint32)), (call, k)
    assert len(set(host[0]["sym"].tolist())) > 1 and not np.array_equal(host[0]["idx"], host[1]["idx"])
    plain = rb.sample(n, augment=False)                       # call 2
    assert not plain["sym"].any() and np.array_equal(plain["idx"], az_amd.replay_sample_plan(seed, 2, n, committed, False)[0])
    dev = torch.device("cuda:0")
    st = torch.empty((n, 11, BS, BS), dtype=torch.float32, device=dev)
    po = torch.empty((n, BS * BS), dtype=torch.float32, device=dev)
    z = torch.empty(n, dtype=torch.float32, device=dev)
    q = torch.empty(n, dtype=torch.float32, device=dev)
    rb.seed(seed)
    for call in range(2):
        for t in (st, po, z, q):
            t.fill_(float("nan"))
        torch.cuda.synchronize()
        rb.sample_into(st, po, z, q, augment=True)
        for k, t in (("states", st), ("policy", po), ("z", z), ("q", q)):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), host[call][k].view(np.uint32)), (call, k)
    with pytest.raises(ValueError):
        rb.sample_into(st[:, :10], po)


def device_mem():
    from az_amd import _lib
    b, k = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().az_diag_device_mem(ctypes.byref(b), ctypes.byref(k)))
    return b.value, k.value


@pytest.mark.gpu
def test_gpu_replay_guards_and_lifecycle(engine, refs):
    import az_amd
    from test_gpu_search import play_and_compare
    mk = dict(board_size=BS, num_simulations=SIMS, evaluator=az_amd.AZ_EVAL_HASH, eval_seed=5, noise_seed=42,
              noise_seed_stride=1)
    m = az_amd.ParallelMCTS(engine, n_games=1, **mk)
    m2 = az_amd.ParallelMCTS(engine, n_games=1, **mk)
    mem0 = device_mem()
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, BS, 64, 40)
    other = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, BS + 1, 64, 40)
    go = az_amd.ReplayBuffer(engine, az_amd.GAME_GO, 9, 64, 40)

    def code(fn):
        with pytest.raises(az_amd.AzError) as e:
            fn()
        return e.value.code

    try:
        assert device_mem()[0] > mem0[0]
        assert code(lambda: m.attachReplay(other)) == -1 and code(lambda: m.attachReplay(go)) == -1
        assert code(lambda: az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, BS, 0, 9)) == -1
        assert code(lambda: rb.sample(4)) == -5                  # empty
        m.attachReplay(rb)
        m.attachReplay(rb)                                       # again: a no-op
        assert code(lambda: m2.attachReplay(rb)) == -5
        # staged plies of an abandoned game are dropped by newGames: the next finished game commits its own plies only
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        for _ in range(5):
            m.selfplayStep()
        assert rb.info()["committed"] == 0 and code(lambda: rb.sample(4)) == -5
        m.newGames([0], ids=[0])
        m.addDirichletNoise(0.03, 0.25)
        n0 = len(refs[0]["moves"])
        for _ in range(n0):
            m.selfplayStep()
        rows = expected_rows(refs, [(0, n0)], BS * BS)
        assert rb.info() == dict(committed=n0, total_committed=n0, games=1, dropped=0, skipped=0)
        check_rows(rb, np.arange(n0), rows)
        assert code(lambda: rb.gather([n0])) == -1 and code(lambda: rb.gather([-1])) == -1
        assert code(lambda: rb.gather([0], [8])) == -1 and code(lambda: rb.counts([n0])) == -1
        # detached, the handle plays the oracle's games bit for bit, and the buffer keeps its ring
        m.attachReplay(None)
        m2.attachReplay(rb)                                      # free again
        m2.attachReplay(None)
        play_and_compare(m, refs[:1], 1, max_moves=2)
        assert rb.info()["committed"] == n0
        check_rows(rb, np.arange(n0), rows)
        rb.clear()
        assert rb.info() == dict(committed=0, total_committed=0, games=0, dropped=0, skipped=0)
    finally:
        for h in (rb, other, go):
            h.close()
        assert device_mem() == mem0
        m.close()
        m2.close()


@pytest.mark.gpu
def test_gpu_replay_leaf_parallel_roots(engine):
    """Leaf parallelism K = 4: the staged counts are the wave model's root children."""
    import az_amd
    import az_oracle as O
    import wave_model as W
    total, mm = 2, 8
    wrefs = W.play(4, seed_stride=1, bs=BS, sims=SIMS, eval_kind=O.EVAL_HASH, eval_seed=5, n_games=total, max_moves=mm)
    mgr = az_amd.SelfPlayManager(engine, numGames=total, numSimulations=SIMS, board_size=BS, evaluator=az_amd.AZ_EVAL_HASH,
                                 eval_seed=5, noise_seed=42, noise_seed_stride=1, leaves=4)
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, BS, 64, mm)
    try:
        mgr.mcts.attachReplay(rb)
        mgr.generateGames(totalGames=total, max_moves=mm)
        rows = expected_rows(wrefs, [(0, mm), (1, mm)], BS * BS)
        assert rb.info()["committed"] == len(rows) == total * mm
        check_rows(rb, np.arange(len(rows)), rows)
    finally:
        rb.close()
        mgr.mcts.close()


@pytest.mark.gpu
def test_gpu_replay_widening_clamps_negative_counts(engine):
    """Progressive widening leaves negative N on children outside the window (the reference's golden game): they are
    stored as 0 and the sum is over the clamped counts."""
    import az_amd
    from test_gpu_search_opts import BY
    ref = BY["widening"]
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    n = len(ref["moves"])
    raw = [N for mv in ref["moves"] for _a, N, *_ in mv["children"]]
    assert min(raw) < 0
    sp = az_amd.SelfPlayManager(engine, numGames=1, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_HASH,
                                c_puct=cp, fpu_reduction=fpu, eval_seed=es, use_widening=True)
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, bs, 256, 256)
    try:
        sp.mcts.attachReplay(rb)
        rec = sp.generateGames(1, max_moves=mm)[0]
        assert len(rec.moves) == n
        rows = expected_rows([ref], [(0, n)], bs * bs)
        assert rb.info()["committed"] == n
        check_rows(rb, np.arange(n), rows)
        cnt, sm = rb.counts(np.arange(n))
        assert cnt.min() == 0 and sm.tolist() == [sum(max(0, N) for _a, N, *_ in mv["children"]) for mv in ref["moves"]]
    finally:
        rb.close()
        sp.mcts.close()


@pytest.mark.gpu
def test_gpu_replay_host_api_fills_the_buffer():
    """_alphazero_cpp: SelfPlayManager.setReplayBuffer makes generateGames fill a ReplayBuffer -- 8 games on 3 slots,
    cut at 30 plies, against the oracle's root children; sample is the plan + gather; a buffer of another board is
    refused when the run starts."""
    import _alphazero_cpp as H
    import az_oracle as O
    total, bs, sims, mm = 8, 7, 64, 30
    hrefs = O.play(seed_stride=1, bs=bs, sims=sims, max_moves=mm, eval_kind=O.EVAL_RANDOM, eval_seed=5, n_games=total)
    lengths = [len(g["moves"]) for g in hrefs]
    net = H.RandomPolicyNetwork(H.GameType.GOMOKU, bs, 5)
    mgr = H.SelfPlayManager(net, total, sims, 4)
    mgr.setConcurrentGames(3)
    mgr.setMaxMoves(mm)
    mgr.setSeeds(42, 1)
    rb = H.ReplayBuffer(H.GameType.GOMOKU, bs, 1024, mm)
    mgr.setReplayBuffer(rb)
    recs = mgr.generateGames(H.GameType.GOMOKU, bs, False)
    assert [len(r.getMoves()) for r in recs] == lengths
    done, running = schedule(lengths, 3, total=total, max_moves=mm)
    assert not running
    rows = expected_rows(hrefs, done, bs * bs)
    assert rb.info() == dict(committed=len(rows), total_committed=len(rows), games=total, dropped=0, skipped=0)
    idx = list(range(len(rows)))
    out = rb.gather(idx)
    cnt, sm = rb.counts(idx)
    assert out["game_id"].tolist() == [r[0] for r in rows] and out["ply"].tolist() == [r[1] for r in rows]
    for i, (gid, ply, c, s, vbits, z) in enumerate(rows):
        assert np.array_equal(cnt[i], c) and int(sm[i]) == s, (gid, ply)
        assert np.array_equal(out["policy"][i], c.astype(np.float32) / np.float32(s)), (gid, ply)
        assert bits([out["q"][i]])[0] == vbits and float(out["z"][i]) == z, (gid, ply)
    assert out["states"].shape == (len(rows), 11, bs, bs)
    actions = [mv["action"] for mv in hrefs[rows[5][0]]["moves"]]
    assert np.array_equal(out["states"][5], gomoku_planes(bs, actions[:rows[5][1]]))
    rb.seed(11)
    s0 = rb.sample(16, True)
    pidx, psym = H.ReplayBuffer.samplePlan(11, 0, 16, len(rows), True)
    assert s0["idx"].tolist() == list(pidx) and s0["sym"].tolist() == list(psym)
    g0 = rb.gather(list(pidx), list(psym))
    for k in ("states", "policy", "z", "q"):
        assert np.array_equal(s0[k].view(np.uint32), g0[k].view(np.uint32)), k
    assert H.ReplayBuffer.symCell(bs, 1, 1) == 1 * bs + (bs - 1)
    mgr.setReplayBuffer(H.ReplayBuffer(H.GameType.GOMOKU, bs + 2, 64, 8))
    with pytest.raises(RuntimeError, match="replay"):
        mgr.generateGames(H.GameType.GOMOKU, bs, False)
    mgr.setReplayBuffer(None)
