"""Full hot path with the ConvNet evaluator: device feature planes -> HIP ConvNet ->
softmax -> TT/expand/backup.  The engine logs every evaluation of one game; the CPU
restatement replays those (policy, value) outputs and must reproduce the device
search bit for bit, and must have asked for exactly the logged feature planes.
The logged network outputs are separately checked against the fp32 reference
network (tolerance 1e-4, BASELINE.json north_star)."""
import numpy as np
import pytest

from replay_util import compare_moves, compare_roots, replay_eval_log, slot_schedule


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("logged", [0, 3])
def test_gpu_net_selfplay_matches_oracle_replay(prec, logged):
    import az_amd
    import net_oracle
    bs, sims, G, moves = 9, 48, 4, 6
    eng = az_amd.Engine(0)
    desc = az_amd.gomoku_net_desc(board_size=bs, channels=32, blocks=2, precision=prec, max_batch=G)
    net = az_amd.HipNeuralNetwork(eng, desc)
    blob = net_oracle.init_blob(desc, seed=9)
    net.load_weights(blob)
    m = az_amd.ParallelMCTS(eng, n_games=G, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                            net=net, noise_seed=42, noise_seed_stride=1)
    cap = (sims + 2) * (moves + 1)
    m.enableEvalLog(logged, cap)
    m.newGames()
    m.addDirichletNoise(0.03, 0.25)
    dev = []
    for ply in range(moves):
        m.search()
        T = 1.0 if ply < 30 else 0.0
        act, val, probs, cact, nch = m.select(True, T)
        a, N, VL, W, P = m.rootChildren(logged)
        dev.append(dict(action=int(act[logged]), value=float(val[logged]), N=N.tolist(), VL=VL.tolist(),
                        W=W.view(np.uint32).tolist(), P=P.view(np.uint32).tolist(),
                        probs=probs[logged, :nch[logged]].view(np.uint32).tolist()))
        term, _ = m.updateWithMove(act)
        if ply % 2 == 0:
            m.addDirichletNoise(0.03, 0.25)
        if term[logged]:
            break
    pol, valv, planes = m.readEvalLog(cap)
    assert len(pol) > sims
    ref = replay_eval_log(pol, valv, planes, [(logged, len(dev))], bs=bs, sims=sims)[0]
    compare_roots(dev, ref["moves"])
    # the logged network outputs against the fp32 reference network
    rl, rv = net_oracle.forward(desc, blob, planes)
    assert np.abs(valv - rv).max() <= 1e-4
    assert np.abs(pol - net_oracle.softmax_policy(rl)).max() <= 1e-4
    m.close()
    net.close()


def _full_size_replay(bs, sims, G, moves, logged, channels, blocks, prec=None, trained=False):
    """Play `moves` moves of G games at a BASELINE.json size (fp16 trunk unless `prec`), log game
    `logged` and replay it through the CPU restatement bit for bit; check a sample of its logged
    network outputs against the fp32 reference network (1e-4) and size-independent properties of
    every game's root (one child per empty cell, visit sum, probability sum, value range).
    trained: heads scaled to a trained net's output magnitudes (|logit|max 8, |value| ~0.9,
    test_gpu_trained_scale.trained_scale_blob), and the raw logits of a full B = G forward of the
    logged leaves checked against the fp32 network too."""
    import az_amd
    import net_oracle
    eng = az_amd.Engine(0)
    desc = az_amd.gomoku_net_desc(board_size=bs, channels=channels, blocks=blocks,
                                  precision=az_amd.AZ_PREC_FP16 if prec is None else prec, max_batch=G)
    net = az_amd.HipNeuralNetwork(eng, desc)
    if trained:
        from test_gpu_trained_scale import _planes as ts_planes, trained_scale_blob
        blob = trained_scale_blob(desc, 1234, ts_planes("c3", 16, seed=17))
    else:
        blob = net_oracle.init_blob(desc, seed=1234)
    net.load_weights(blob)
    m = az_amd.ParallelMCTS(eng, n_games=G, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                            net=net, noise_seed=42, noise_seed_stride=1)
    cap = (sims + 2) * (moves + 1)
    m.enableEvalLog(logged, cap)
    m.newGames()
    m.addDirichletNoise(0.03, 0.25)
    dev = []
    for ply in range(moves):
        m.search()
        act, val, probs, cact, nch = m.select(True, 1.0)
        # every game: one child per empty cell, probabilities sum to 1, values within [-1, 1]
        assert (nch == bs * bs - ply).all()
        sums = np.array([probs[g, :nch[g]].astype(np.float64).sum() for g in range(G)])
        assert np.abs(sums - 1.0).max() < 1e-5
        assert (np.abs(val) <= 1.0 + 1e-6).all()
        a, N, VL, W, P = m.rootChildren(logged)
        assert int(np.sum(N)) >= sims - 1
        dev.append(dict(action=int(act[logged]), value=float(val[logged]), N=N.tolist(), VL=VL.tolist(),
                        W=W.view(np.uint32).tolist(), P=P.view(np.uint32).tolist(),
                        probs=probs[logged, :nch[logged]].view(np.uint32).tolist()))
        m.updateWithMove(act)
        if ply % 2 == 0:
            m.addDirichletNoise(0.03, 0.25)
    pol, valv, planes = m.readEvalLog(cap)
    assert len(pol) > sims   # TT hits and terminal leaves are not evaluated
    ref = replay_eval_log(pol, valv, planes, [(logged, moves)], bs=bs, sims=sims)[0]
    compare_roots(dev, ref["moves"])
    idx = np.random.default_rng(0).choice(len(pol), 48, replace=False)
    rl, rv = net_oracle.forward(desc, blob, planes[idx])
    assert np.abs(valv[idx] - rv).max() <= 1e-4
    assert np.abs(pol[idx] - net_oracle.softmax_policy(rl)).max() <= 1e-4
    # RAW logits and values of a full-capacity forward (B = G boards: the logged leaves, cycled) --
    # post-softmax probabilities of ~1/A each would hide a logit error A times larger
    xb = planes[np.arange(G) % len(planes)]
    lo, v = net.forward(xb)
    jdx = np.unique(np.concatenate([[0, G - 1], np.random.default_rng(1).choice(G, 14, replace=False)]))
    jl, jv = net_oracle.forward(desc, blob, xb[jdx])
    el = float(np.abs(lo[jdx] - jl).max())
    ev = float(np.abs(v[jdx] - jv).max())
    print(f"full-size raw outputs ({'trained-scale' if trained else 'init'} weights): |logit|max "
          f"{np.abs(jl).max():.3f} max|dlogit|={el:.3e} max|dvalue|={ev:.3e} over {len(jdx)} boards of B = {G}")
    assert el <= 1e-4 and ev <= 1e-4
    if trained:
        assert np.abs(jl).max() > 2.0
    m.close()
    net.close()


@pytest.mark.gpu
def test_gpu_c3_full_size_replay():
    """C3 at full size (BASELINE.json configs[2]: 2048 games, 15x15, 800 sims, the 20 x 256 net):
    the first two moves of every game, game 1337 (in the middle of the batch) replayed."""
    _full_size_replay(bs=15, sims=800, G=2048, moves=2, logged=1337, channels=256, blocks=20)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
def test_gpu_c3_full_size_replay_x3(prec):
    """C3 at full size in the split precisions (AZ_PREC_F16X3 -- the parity precision -- and
    AZ_PREC_BF16X3, both on conv3x3_v9x3) with trained-scale heads: two moves of all 2048 games, game
    1337 replayed bit for bit, sampled logits / values of the logged leaves and of a B = 2048 forward
    within 1e-4 of the fp32 network."""
    _full_size_replay(bs=15, sims=800, G=2048, moves=2, logged=1337, channels=256, blocks=20,
                      prec={"f16x3": 4, "bf16x3": 1}[prec], trained=True)


@pytest.mark.gpu
def test_gpu_c2_full_size_replay():
    """C2 at full size (BASELINE.json configs[1]: 256 games, 15x15, 400 sims, the 6 x 64 net of
    python/simple_export.py's shape family): the first four moves of every game (noise after plies
    0 and 2, subtree reuse across three moves), game 137 replayed."""
    _full_size_replay(bs=15, sims=400, G=256, moves=4, logged=137, channels=64, blocks=6)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "bf16x3"])
def test_gpu_c2_full_size_replay_x3(prec):
    """C2 at full size in the split precisions (k_smallnet_x3 with fp16 / bf16 pieces, fed the
    search's leaf records) with trained-scale heads: four moves of all 256 games, game 137 replayed
    bit for bit, sampled outputs of the logged leaves and of a B = 256 forward within 1e-4 of fp32."""
    _full_size_replay(bs=15, sims=400, G=256, moves=4, logged=137, channels=64, blocks=6,
                      prec={"f16x3": 4, "bf16x3": 1}[prec], trained=True)


# ------------------------------------------------- the self-play drivers with the network, through game ends
def _restart_net(eng, prec, slots):
    """The 6x6 net of the restart tests (32 channels x 2 blocks, init weights) at `slots` boards."""
    import az_amd
    import net_oracle
    desc = az_amd.gomoku_net_desc(board_size=6, channels=32, blocks=2, precision=prec, max_batch=slots)
    net = az_amd.HipNeuralNetwork(eng, desc)
    blob = net_oracle.init_blob(desc, seed=9)
    net.load_weights(blob)
    return desc, net, blob


def _check_logged_outputs(desc, blob, pol, valv, planes):
    """Every logged network output against the fp32 reference network on the logged planes (1e-4)."""
    import net_oracle
    rl, rv = net_oracle.forward(desc, blob, planes)
    ev = float(np.abs(valv - rv).max())
    ep = float(np.abs(pol - net_oracle.softmax_policy(rl)).max())
    print(f"{len(pol)} logged evaluations: max|dvalue|={ev:.3e} max|dpolicy|={ep:.3e} vs fp32")
    assert ev <= 1e-4 and ep <= 1e-4, (ev, ep)


def _finished(bs, moves):
    import az_oracle as O
    return O.position(bs, moves)[2] != 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("logged", [0, 3])
def test_gpu_net_selfplay_step_restarts_match_oracle_replay(prec, logged):
    """az_selfplay_step with AZ_EVAL_NET and restart_finished, as test_gpu_selfplay_step_matches_oracle
    does with the hash / random evaluators: 4 slots of 6x6 Gomoku stepped 80 moves (a 6x6 game has at
    most 36 plies: every slot restarts at least twice).  A restart's root step is a compacted batch of
    the restarted slots only.  The logged slot's sequence of games -- a finished slot takes the next
    game id in slot order -- is replayed through the oracle from its evaluation log, and every
    MoveData of the slot compared bit for bit; every logged output within 1e-4 of the fp32 network."""
    import az_amd
    bs, sims, slots, steps = 6, 32, 4, 80
    eng = az_amd.Engine(0)
    desc, net, blob = _restart_net(eng, prec, slots)
    m = az_amd.ParallelMCTS(eng, n_games=slots, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                            net=net, noise_seed=42, noise_seed_stride=1)
    cap = steps * (sims + 2)
    gid = list(range(slots))                 # the game id each slot plays
    hist = [[] for _ in range(slots)]        # its moves so far
    nxt = slots
    restarts = [0] * slots
    played = [[logged, []]]                  # the logged slot's games: [game id, MoveData so far]
    try:
        m.enableEvalLog(logged, cap)
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        for step in range(steps):
            mv, _ = m.selfplayStep(restart_finished=True)
            recs = m.stepMoves(materialize=True)
            assert mv == len(recs) == slots, step            # every slot moves (finished slots restarted)
            assert [s for s, _ in recs] == list(range(slots))
            for s, md in recs:
                assert len(md.policy) == len(md.child_actions) == bs * bs - len(hist[s]), (step, s)
                hist[s].append(md.action)
                if s == logged:
                    played[-1][1].append(md)
            for s in range(slots):                           # finished: the slot takes the next id
                if _finished(bs, hist[s]):
                    gid[s], hist[s], nxt = nxt, [], nxt + 1
                    restarts[s] += 1
                    if s == logged:
                        played.append([gid[s], []])
        pol, valv, planes = m.readEvalLog(cap)
    finally:
        m.close()
        net.close()
    assert min(restarts) >= 2, restarts
    assert len(pol) < cap
    # the last game is cut at its current ply (0 moves right after a restart: its first root only)
    refs = replay_eval_log(pol, valv, planes, [(g, len(mds)) for g, mds in played], bs=bs, sims=sims)
    for i, ((g, mds), ref) in enumerate(zip(played, refs)):
        if i + 1 < len(played):
            assert ref["terminal"] and len(ref["moves"]) == len(mds), (g, len(mds))
        compare_moves(mds, ref, (g,))
    _check_logged_outputs(desc, blob, pol, valv, planes)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("logged", [0, 3])
def test_gpu_net_selfplay_step_to_the_end_matches_oracle_replay(prec, logged):
    """az_selfplay_step without restarts until every slot has finished: finished slots stay idle
    while the others simulate (the compacted simulation batch, reached through natural game ends),
    a step with every slot idle reports 0 moves, and the logged slot's game replays bit for bit."""
    import az_amd
    bs, sims, slots = 6, 32, 4
    eng = az_amd.Engine(0)
    desc, net, blob = _restart_net(eng, prec, slots)
    m = az_amd.ParallelMCTS(eng, n_games=slots, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                            net=net, noise_seed=42, noise_seed_stride=1)
    cap = (bs * bs + 1) * (sims + 2)
    hist = [[] for _ in range(slots)]
    live = [True] * slots
    mds = []
    moved = []
    try:
        m.enableEvalLog(logged, cap)
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        for step in range(bs * bs + 1):                      # at most 36 plies, then one idle step
            mv, _ = m.selfplayStep(restart_finished=False)
            recs = m.stepMoves(materialize=True)
            assert mv == len(recs) and [s for s, _ in recs] == [s for s in range(slots) if live[s]], step
            moved.append(mv)
            if mv == 0:
                break
            for s, md in recs:
                hist[s].append(md.action)
                live[s] = not _finished(bs, hist[s])
                if s == logged:
                    mds.append(md)
        pol, valv, planes = m.readEvalLog(cap)
    finally:
        m.close()
        net.close()
    assert moved[-1] == 0 and not any(live), moved
    assert any(0 < n < slots for n in moved), moved          # some slots idle while others played
    assert len(pol) < cap
    ref = replay_eval_log(pol, valv, planes, [(logged, len(mds))], bs=bs, sims=sims)[0]
    assert ref["terminal"] and len(ref["moves"]) == len(mds)
    compare_moves(mds, ref, (logged,))
    _check_logged_outputs(desc, blob, pol, valv, planes)


@pytest.mark.gpu
@pytest.mark.parametrize("fpu,each_search", [(0.0, False), (0.1, True)], ids=["prefetch", "binary-cfg"])
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("logged", [0, 2])
def test_gpu_net_selfplay_run_matches_oracle_replay(prec, logged, fpu, each_search):
    """az_selfplay_run (SelfPlayManager.generateGames) with the network: 7 games of 6x6 Gomoku on 3
    slots, with the noise prefetch on (fpu 0, noise at the root once) and in the self_play binary's
    configuration (fpu 0.1, noise on every search).  The slot that played each game follows from the
    game lengths (replay_util.slot_schedule); the logged slot's games are replayed through the oracle
    from its evaluation log and each of its GameRecords compared move by move, bit for bit, with its
    result.  In the run's tail a slot is idle while another plays: a compacted simulation batch."""
    import az_amd
    bs, sims, slots, total = 6, 32, 3, 7
    eng = az_amd.Engine(0)
    desc, net, blob = _restart_net(eng, prec, slots)
    mgr = az_amd.SelfPlayManager(eng, net=net, numGames=slots, numSimulations=sims, board_size=bs,
                                 fpu_reduction=fpu, use_dirichlet_each_search=each_search, noise_seed=42,
                                 noise_seed_stride=1)
    cap = total * (bs * bs + 1) * (sims + 2)
    try:
        mgr.mcts.enableEvalLog(logged, cap)
        recs = mgr.generateGames(totalGames=total)
        pol, valv, planes = mgr.mcts.readEvalLog(cap)
    finally:
        mgr.mcts.close()
        net.close()
    assert [r.game_id for r in recs] == list(range(total))
    games, sched = slot_schedule(slots, [len(r.moves) for r in recs])
    assert sorted(g for gs in games for g in gs) == list(range(total))
    assert any(None in row and any(g is not None for g in row) for row in sched), sched   # the idle tail
    mine = games[logged]
    assert mine[0] == logged and len(pol) < cap
    refs = replay_eval_log(pol, valv, planes, [(g, len(recs[g].moves)) for g in mine], bs=bs, sims=sims, fpu=fpu,
                           noise_each_search=int(each_search))
    for g, ref in zip(mine, refs):
        assert ref["terminal"] and len(ref["moves"]) == len(recs[g].moves), g
        compare_moves(recs[g].moves, ref, (g,))
        assert recs[g].result == ref["result"], g
    _check_logged_outputs(desc, blob, pol, valv, planes)
