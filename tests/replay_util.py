"""Shared pieces of the eval-log replay tests (tests/test_gpu_selfplay_net.py, test_gpu_go.py,
test_gpu_net_partial_batch.py, test_gpu_self_play_main.py): the engine logs every network evaluation
of one device slot (policy, value, feature planes); the CPU restatement (oracle/az_oracle.cpp) replays
those outputs, must have asked for exactly the logged planes in the logged order, and its records are
then compared bit for bit with what the device played."""
import numpy as np


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


def replay_eval_log(pol, val, planes, games, **search):
    """Replay one slot's evaluation log through the oracle.

    pol [n][A], val [n], planes [n][C][bs][bs]: the log as ParallelMCTS.readEvalLog returns it.
    games: [(game_id, n_moves)] in the order the logged slot played them (game_id seeds the game's
    noise stream: 42 + game_id); the oracle plays n_moves moves of each (a game that ends earlier
    ends there).  search: the az_oracle.play settings (bs, sims, game, fpu, noise_each_search, ...).

    Every evaluation the oracle asks for must carry exactly the logged planes (np.array_equal), and
    the games together must consume the whole log.  Returns the oracle's record of each game."""
    import az_oracle as O
    k = [0]
    bad = []

    def replay(game, x):
        i = k[0]
        if i >= len(pol):
            bad.append(f"the oracle asks for evaluation {i}, the log holds {len(pol)}")
            raise O.StopPlay()
        if not np.array_equal(x, planes[i]):
            bad.append(f"feature planes differ at evaluation {i}")
            raise O.StopPlay()
        k[0] += 1
        return pol[i], float(val[i])

    refs = []
    for game_id, n_moves in games:
        r = O.play(eval_kind=O.EVAL_REPLAY, evaluator=replay, noise_seed=42 + game_id, max_moves=n_moves, **search)
        assert not bad and r is not None, (bad, game_id, n_moves)
        refs.append(r[0])
    assert k[0] == len(pol), f"{len(pol)} logged evaluations, the oracle asked for {k[0]}"
    return refs


def root_record(m, g, act, val, probs, nch):
    """Game g's root after a search, as compare_roots takes it (select()'s arrays + rootChildren)."""
    a, N, VL, W, P = m.rootChildren(g)
    return dict(action=int(act[g]), value=float(val[g]), N=N.tolist(), VL=VL.tolist(), W=bits(W), P=bits(P),
                probs=bits(probs[g, :nch[g]]))


def compare_roots(dev, ref_moves, value=True):
    """The device's roots (root_record per ply) against the oracle's moves: raw N / VL, the fp32 bit
    patterns of W, P and the visit distribution, the action and (value=True) the root value's bits."""
    assert len(dev) <= len(ref_moves), (len(dev), len(ref_moves))
    for ply, (d, r) in enumerate(zip(dev, ref_moves)):
        kids = r["children"]
        assert d["N"] == [c[1] for c in kids] and d["VL"] == [c[2] for c in kids], ply
        assert d["W"] == [c[3] for c in kids] and d["P"] == [c[4] for c in kids], ply
        assert d["probs"] == r["probs"] and d["action"] == r["action"], ply
        if value:
            assert np.float32(d["value"]).view(np.uint32) == r["value"], ply


def compare_moves(moves, ref, where=()):
    """MoveData records (az_selfplay_step_moves / a GameRecord's moves) against the first len(moves)
    moves of an oracle record: action, child-order visit distribution bits (the T = 0 NaNs included),
    root value bits and the child actions."""
    assert len(moves) <= len(ref["moves"]), (where, len(moves), len(ref["moves"]))
    for ply, (md, rm) in enumerate(zip(moves, ref["moves"])):
        at = (*where, ply)
        assert md.action == rm["action"], at
        assert bits(md.policy) == rm["probs"], at
        assert bits([md.value])[0] == rm["value"], at
        assert list(md.child_actions) == [c[0] for c in rm["children"]], at


def slot_schedule(n_slots, lengths):
    """Which slot plays which game in az_selfplay_run, from the games' lengths (moves per game id).

    Slots 0..n_slots-1 start ids 0..n_slots-1; every live slot moves once per step; the slots whose
    game ended in a step take the next ids in slot order while ids remain, the others stay idle.
    Returns (games, steps): games[s] the ids slot s played, in order; steps[t][s] the id slot s
    moved in step t, or None while it was idle."""
    total = len(lengths)
    assert n_slots >= 1 and all(n >= 1 for n in lengths)
    cur = [s if s < total else None for s in range(n_slots)]
    ply = [0] * n_slots
    nxt = min(n_slots, total)
    games = [[g] if g is not None else [] for g in cur]
    steps = []
    while any(g is not None for g in cur):
        steps.append(tuple(cur))
        for s in range(n_slots):
            if cur[s] is None:
                continue
            ply[s] += 1
            if ply[s] == lengths[cur[s]]:
                cur[s], ply[s] = None, 0
                if nxt < total:
                    cur[s], nxt = nxt, nxt + 1
                    games[s].append(cur[s])
    return games, steps
