"""The two-net evaluation match on the device (az_arena_*, csrc/arena.hip; the game loop of the reference's
python/scripts/evaluate.py:186-291 on one search handle with per-slot nets).

Composition parity: the arena's games equal, ply by ply and bit for bit, the same loop written here with two
separate single-net handles (one per net, one slot per table) through the masked entry points -- whose own
parity with the reference build the api goldens and test_search_group_matches_standalone pin."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

from replay_util import bits, root_record, slot_schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "alphazero-multi-game_amd", "build", "evaluate")
SMALL = dict(tt_log2=12)


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def make_net(engine, go, bs, ch, blocks, prec, max_batch, seed):
    import az_amd
    import net_oracle
    desc = az_amd.NetDesc(bs, 8 if go else 11, ch, blocks, bs * bs + (1 if go else 0), 32, 8, 256, 1, 0, prec, max_batch)
    net = az_amd.HipNeuralNetwork(engine, desc)
    net.load_weights(net_oracle.init_blob(desc, seed=seed))
    return net


def a_first(swap, gid):
    return (not swap) or gid % 2 == 0


def compose(engine, nets, T, bs, sims, go, total, max_moves, swap, noise, temperature, sample_moves):
    """evaluate.py's loop on two single-net handles of T slots (handle p: net p's tree of every table), in lock
    step over the tables, with the arena's schedule: ({gid: game dict}, steps)."""
    import az_amd
    hs = [az_amd.ParallelMCTS(engine, n_games=T, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                              net=nets[p], noise_seed=42, noise_seed_stride=1,
                              game=az_amd.AZ_GAME_GO if go else az_amd.AZ_GAME_GOMOKU, **SMALL) for p in (0, 1)]
    try:
        none = hs[0].none
        gid, ply, nxt = [-1] * T, [0] * T, 0
        games, steps = {}, []

        def start(tables):
            nonlocal nxt
            for i in tables:
                gid[i], ply[i] = nxt, 0
                games[nxt] = dict(roots=[], movers=[], result=0, a_is_player1=a_first(swap, nxt))
                for p in (0, 1):
                    hs[p].newGames([i], ids=[2 * nxt + p])
                nxt += 1

        start(range(min(T, total)))
        while any(g >= 0 for g in gid):
            assert len(steps) < 400
            steps.append(tuple(g if g >= 0 else None for g in gid))
            masks = [np.zeros(T, np.uint8), np.zeros(T, np.uint8)]
            mover = {}
            for i in range(T):
                if gid[i] >= 0:
                    mover[i] = 0 if (ply[i] % 2 == 0) == a_first(swap, gid[i]) else 1
                    masks[mover[i]][i] = 1
            sel = []
            for p in (0, 1):
                if noise:
                    hs[p].addDirichletNoise(noise[0], noise[1], mask=masks[p])
                hs[p].search(mask=masks[p])
                sel.append(hs[p].select(True, temperature))
            acts = np.full(T, none, np.int32)
            for i, p in mover.items():
                act, val, probs, cact, nch = sel[p]
                r = root_record(hs[p], i, act, val, probs, nch)
                if ply[i] < sample_moves:
                    r["action"] = hs[p].selectActionFor(i, True, temperature, useBatchInference=False)
                acts[i] = r["action"]
                games[gid[i]]["roots"].append(r)
                games[gid[i]]["movers"].append(p)
            term, res = hs[0].updateWithMove(acts)
            term1, res1 = hs[1].updateWithMove(acts)
            restart = []
            for i in mover:
                assert term[i] == term1[i] and res[i] == res1[i]
                ply[i] += 1
                if term[i] or (max_moves > 0 and ply[i] >= max_moves):
                    games[gid[i]]["result"] = int(res[i]) if term[i] else 0
                    gid[i] = -1
                    if nxt + len(restart) < total:
                        restart.append(i)
            start(restart)
        return games, steps
    finally:
        for h in hs:
            h.close()


def arena_games(engine, nets, T, bs, sims, go, total, max_moves, swap, noise, temperature, sample_moves):
    """The same match on the arena: ({gid: game dict}, steps, records, summary); every mover's root is read
    from the underlying handle in the progress callback (after the move is chosen, before it is applied)."""
    import az_amd
    ar = az_amd.Arena(engine, nets[0], nets[1], T, board_size=bs, num_simulations=sims, swap_colors=swap,
                      temperature=temperature, sample_moves=sample_moves, noise_alpha=noise[0] if noise else 0.03,
                      noise_eps=noise[1] if noise else 0.0, game=az_amd.AZ_GAME_GO if go else az_amd.AZ_GAME_GOMOKU,
                      **SMALL)
    try:
        kids, steps, seen = {}, [], set()

        def on_move(gid, ply, total_games, total_moves):
            tables = ar.tableGames()
            snap = tuple(g if g >= 0 else None for g in tables)
            if not steps or snap != steps[-1] or gid in seen:
                steps.append(snap)
                seen.clear()
            seen.add(gid)
            p = 0 if (ply % 2 == 0) == a_first(swap, gid) else 1
            a, N, VL, W, P = ar.search.rootChildren(2 * tables.index(gid) + p)
            kids.setdefault(gid, []).append(dict(N=N.tolist(), VL=VL.tolist(), W=bits(W), P=bits(P)))

        ar.progressCallback = on_move
        recs = ar.run(total, max_moves)
        games = {}
        for r in recs:
            assert len(kids[r.game_id]) == len(r.moves)
            roots = [dict(action=m.action, value=float(m.value), probs=bits(m.policy), **k)
                     for m, k in zip(r.moves, kids[r.game_id])]
            games[r.game_id] = dict(roots=roots, movers=r.movers, result=r.result, a_is_player1=r.a_is_player1)
        return games, steps, recs, ar.summary()
    finally:
        ar.close()


def same_root(x, y):
    return all(x[k] == y[k] for k in ("action", "N", "VL", "W", "P", "probs")) and bits([x["value"]]) == bits([y["value"]])


# id: (go, board, channels, blocks, precision, tables, games, max_moves, sims, noise, temperature, sample_moves)
MATCHES = {
    "gomoku-cut":    (False, 7, 32, 2, "f32", 4, 6, 5, 24, (0.03, 0.25), 0.1, 0),
    "go-natural":    (True, 9, 128, 1, "fp16", 4, 6, 0, 24, (0.03, 0.25), 0.1, 0),
    "gomoku-sample": (False, 7, 32, 2, "f32", 2, 3, 4, 24, (0.03, 0.25), 1.0, 2),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(MATCHES))
def test_gpu_arena_composition_parity(engine, case):
    import az_amd
    go, bs, ch, blocks, prec, T, total, max_moves, sims, noise, temp, sample = MATCHES[case]
    p = {"f32": az_amd.AZ_PREC_F32, "fp16": az_amd.AZ_PREC_FP16}[prec]
    nets = [make_net(engine, go, bs, ch, blocks, p, T, seed) for seed in (9, 10)]
    try:
        args = (engine, nets, T, bs, sims, go, total, max_moves, True, noise, temp, sample)
        got, steps, recs, summ = arena_games(*args)
        want, want_steps = compose(*args)
        assert sorted(got) == sorted(want) == list(range(total))
        for gid in range(total):
            g, w = got[gid], want[gid]
            assert g["movers"] == w["movers"] and g["result"] == w["result"], gid
            assert g["a_is_player1"] == w["a_is_player1"] == (gid % 2 == 0), gid
            assert len(g["roots"]) == len(w["roots"]), gid
            for ply, (x, y) in enumerate(zip(g["roots"], w["roots"])):
                assert same_root(x, y), (gid, ply)
        lengths = [len(got[gid]["roots"]) for gid in range(total)]
        sched = [tuple(s) for s in slot_schedule(T, lengths)[1]]
        print(f"arena {case}: game lengths {lengths}, results {[got[g]['result'] for g in range(total)]}, "
              f"{len(steps)} steps")
        assert steps == want_steps == sched
        if max_moves:
            assert lengths == [max_moves] * total and all(got[g]["result"] == 0 for g in got)
            assert summ["draws"] == total and all(r.score_a == 0.5 for r in recs)
        if sample:   # the drawn plies are the mover's stochastic selectAction, the others the deterministic rule
            assert summ["moves"] == sum(lengths)
    finally:
        for n in nets:
            n.close()


@pytest.fixture(scope="module")
def mirror_match(engine):
    """Net A against a copy of itself, colours swapped every game, no noise, deterministic selection: 4 games on
    2 tables played to the end; (records, summary, evals of every slot of the handle after the run)."""
    import az_amd
    T, total, bs = 2, 4, 7
    nets = [make_net(engine, False, bs, 32, 2, az_amd.AZ_PREC_F32, T, 9) for _ in range(2)]
    ar = az_amd.Arena(engine, nets[0], nets[1], T, board_size=bs, num_simulations=16, swap_colors=True, **SMALL)
    try:
        recs = ar.run(total)
        return recs, ar.summary(), [ar.search.counters(g)["evals"] for g in range(2 * T)], T
    finally:
        ar.close()
        for n in nets:
            n.close()


@pytest.mark.gpu
def test_gpu_arena_symmetry(mirror_match):
    recs, summ, _, _ = mirror_match
    assert [r.game_id for r in recs] == [0, 1, 2, 3]
    for k in (0, 2):
        a, b = recs[k], recs[k + 1]
        assert a.a_is_player1 and not b.a_is_player1
        assert [m.action for m in a.moves] == [m.action for m in b.moves] and a.result == b.result
        assert [bits(m.policy) for m in a.moves] == [bits(m.policy) for m in b.moves]
        assert a.movers == [1 - p for p in b.movers]
        assert a.score_a + b.score_a == 1.0
    assert summ["wins_a"] == summ["wins_b"] and summ["games"] == 4


@pytest.mark.gpu
def test_gpu_arena_summary_matches_records(mirror_match):
    recs, summ, slot_evals, T = mirror_match
    scores = [r.score_a for r in recs]
    for r in recs:   # evaluate.py:259-278
        want = 0.5 if r.result in (0, 1) else float((r.result == 2) == r.a_is_player1)
        assert r.score_a == want, r.game_id
    assert summ["games"] == len(recs)
    assert (summ["wins_a"], summ["wins_b"], summ["draws"]) == (scores.count(1.0), scores.count(0.0), scores.count(0.5))
    assert summ["moves"] == sum(len(r.moves) for r in recs)
    assert summ["evals_a"] == sum(r.evals_a for r in recs) > 0 and summ["evals_b"] == sum(r.evals_b for r in recs) > 0
    # the handle's per-slot counters still hold the last game of every table
    played, _ = slot_schedule(T, [len(r.moves) for r in recs])
    for t in range(T):
        last = recs[played[t][-1]]
        assert (slot_evals[2 * t], slot_evals[2 * t + 1]) == (last.evals_a, last.evals_b), t
    ra = rb = 1500.0   # elo.py:12-40, :70-101 in game-id order
    for s in scores:
        ea = 1.0 / (1.0 + math.pow(10, (rb - ra) / 400.0))
        eb = 1.0 / (1.0 + math.pow(10, (ra - rb) / 400.0))
        ra, rb = ra + 32.0 * (s - ea), rb + 32.0 * ((1.0 - s) - eb)
    assert abs(summ["elo_a"] - ra) <= 1e-9 and abs(summ["elo_b"] - rb) <= 1e-9


JSON_KEYS = {"model_a", "model_b", "model_a_short", "model_b_short", "game_type", "board_size", "variant_rules",
             "games_played", "wins_a", "wins_b", "draws", "win_rate_a", "win_rate_b", "draw_rate", "elo_a", "elo_b",
             "simulations", "threads", "temperature", "time_control", "timestamp", "avg_move_time", "total_moves"}


@pytest.mark.gpu
def test_gpu_evaluate_binary_matches_arena(engine, tmp_path):
    """build/evaluate on two .azw files (7x7, 4 games, 2 tables) in a child process: its result file has the
    summary keys of evaluate.py:429-460 and the scalars of az_amd.Arena at the same settings."""
    import _alphazero_cpp as A
    import az_amd
    import net_oracle
    bs, sims, games, tables = 7, 16, 4, 2
    desc = az_amd.gomoku_net_desc(bs, 32, 2, az_amd.AZ_PREC_F32, max_batch=8)
    blobs = [net_oracle.init_blob(desc, seed=seed) for seed in (9, 10)]
    paths = []
    for name, blob in zip(("cand", "best"), blobs):
        n = A.HipNeuralNetwork(bs, 32, 2, 11, az_amd.AZ_PREC_F32, 8)
        n.loadWeights(blob)
        paths.append(str(tmp_path / f"{name}.azw"))
        n.save(paths[-1])
        del n
    out = tmp_path / "results"
    r = subprocess.run([BIN, "--model-a", paths[0], "--model-b", paths[1], "--game", "gomoku", "--size", str(bs),
                        "--games", str(games), "--simulations", str(sims), "--threads", "4", "--output-dir", str(out),
                        "--temperature", "0.1", "--swap", "--seed", "42", "--tables", str(tables), "--precision", "f32"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    js = json.load(open(out / "gomoku_cand_vs_best.json"))
    assert set(js) == JSON_KEYS
    nets = []
    for blob in blobs:
        n = az_amd.HipNeuralNetwork(engine, desc)
        n.load_weights(blob)
        nets.append(n)
    ar = az_amd.Arena(engine, nets[0], nets[1], tables, board_size=bs, num_simulations=sims, swap_colors=True,
                      temperature=0.1, noise_seed=42)
    try:
        ar.run(games)
        s = ar.summary()
    finally:
        ar.close()
        for n in nets:
            n.close()
    assert (js["games_played"], js["wins_a"], js["wins_b"], js["draws"], js["total_moves"]) == \
        (s["games"], s["wins_a"], s["wins_b"], s["draws"], s["moves"]) and s["games"] == games
    assert js["elo_a"] == s["elo_a"] and js["elo_b"] == s["elo_b"]
    assert js["win_rate_a"] == s["wins_a"] / games * 100 and js["draw_rate"] == s["draws"] / games * 100
    assert (js["game_type"], js["board_size"], js["simulations"], js["threads"]) == ("gomoku", bs, sims, 4)
    assert js["variant_rules"] is False and js["time_control"] is None and js["model_a_short"] == "cand"


@pytest.mark.gpu
def test_gpu_pybind_arena_matches_az_amd(engine):
    """alphazero::evaluation::Arena through _alphazero_cpp (GIL released around run) plays the games az_amd.Arena
    plays at the same settings: every move, mover, result and score, and the same summary."""
    import _alphazero_cpp as A
    import az_amd
    import net_oracle
    bs, sims, games, tables, cut = 7, 16, 3, 2, 6
    desc = az_amd.gomoku_net_desc(bs, 32, 2, az_amd.AZ_PREC_F32, max_batch=4)
    blobs = [net_oracle.init_blob(desc, seed=seed) for seed in (9, 10)]
    cnets = []
    for blob in blobs:
        n = A.HipNeuralNetwork(bs, 32, 2, 11, az_amd.AZ_PREC_F32, 4)
        n.loadWeights(blob)
        cnets.append(n)
    cfg = A.ArenaConfig()
    cfg.boardSize, cfg.tables, cfg.numSimulations, cfg.swapColors, cfg.ttLog2 = bs, tables, sims, True, 12
    cfg.noiseEpsilon, cfg.noiseAlpha = 0.25, 0.03
    seen = []
    ca = A.Arena(cnets[0], cnets[1], cfg)
    ca.setProgressCallback(lambda g, mv, tg, tm: seen.append((g, mv)))
    crecs = ca.run(games, cut)
    cs = ca.summary()
    del ca
    nets = []
    for blob in blobs:
        n = az_amd.HipNeuralNetwork(engine, desc)
        n.load_weights(blob)
        nets.append(n)
    ar = az_amd.Arena(engine, nets[0], nets[1], tables, board_size=bs, num_simulations=sims, swap_colors=True,
                      noise_eps=0.25, noise_alpha=0.03, **SMALL)
    try:
        recs = ar.run(games, cut)
        s = ar.summary()
    finally:
        ar.close()
        for n in nets:
            n.close()
    assert len(crecs) == len(recs) == games and sorted(seen) == [(g, mv) for g in range(games) for mv in range(cut)]
    for c, r in zip(crecs, recs):
        assert (c.gameId, c.aIsPlayer1, int(c.result), c.scoreA) == (r.game_id, r.a_is_player1, r.result, r.score_a)
        assert list(c.movers) == r.movers and (c.evalsA, c.evalsB) == (r.evals_a, r.evals_b)
        assert [m.action for m in c.moves] == [m.action for m in r.moves]
        assert [bits(m.policy) for m in c.moves] == [bits(m.policy) for m in r.moves]
        assert bits([m.value for m in c.moves]) == bits([m.value for m in r.moves])
    assert (cs.games, cs.winsA, cs.winsB, cs.draws, cs.moves, cs.evalsA, cs.evalsB, cs.eloA, cs.eloB) == \
        tuple(s[k] for k in ("games", "wins_a", "wins_b", "draws", "moves", "evals_a", "evals_b", "elo_a", "elo_b"))
