"""GPU parity of the search options (az_search_opts, az_search_set_options: selection strategy, depth cap, TD(lambda)
backup, progressive widening) against golden vectors of the patched REFERENCE search under those
options (tests/golden/ref_search_opts_games.json.gz, written by tests/golden/gen_search_opts_golden.py).
Bit-exact, as tests/test_gpu_search.py: raw N / VL / W / P bits of the root's children, probabilities,
action, value and the transposition-table counters at every ply."""
import ctypes
import glob
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_search import GAMES as PLAIN_GAMES
from test_gpu_search import children_rows, play_and_compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "alphazero-multi-game_amd", "build", "self_play")
with gzip.open(os.path.join(GOLD, "ref_search_opts_games.json.gz"), "rt") as _f:
    GAMES = json.load(_f)
BY = {g["name"]: g for g in GAMES}


def bits(xs):
    return np.asarray(xs, np.float32).view(np.uint32).tolist()


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def handle(engine, ref, n_games=1, opts=None, **kw):
    import az_amd
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    kw.setdefault("noise_seed", ref["noise_seed"])
    if (ref["opts"] if opts is None else opts).get("selection") == 0:
        # UCB descends one chain of first children, so nearly every node ever created stays in the reused
        # subtree: the pool holds the whole game's nodes (the default is sized for three searches' worth)
        kw.setdefault("node_capacity", (mm + 2) * sims * (bs * bs + 1))
    return az_amd.ParallelMCTS(engine, n_games=n_games, board_size=bs, num_simulations=sims, c_puct=cp, fpu_reduction=fpu,
                               virtual_loss=ref["virtual_loss"],
                               evaluator=az_amd.AZ_EVAL_HASH if ev == "hash" else az_amd.AZ_EVAL_RANDOM, eval_seed=es,
                               use_dirichlet_each_search=bool(nes), game=ref["go"],
                               **(ref["opts"] if opts is None else opts), **kw)


GOLDEN = [g["name"] for g in GAMES if g["name"] != "switch"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN)
def test_gpu_search_opts_match_reference_golden(engine, name):
    ref = BY[name]
    m = handle(engine, ref)
    try:
        got = m.searchOptions()
        assert {k: got[k] for k in ("selection", "max_search_depth", "use_td", "use_widening", "widening_min_visits")} == \
            {k: type(got[k])(ref["opts"][k]) for k in ("selection", "max_search_depth", "use_td", "use_widening", "widening_min_visits")}
        play_and_compare(m, [ref], 1)
    finally:
        m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["td0.3-5x5", "widening-min1-vl1"])
def test_gpu_search_opts_split_and_fused_kernels_agree(engine, name):
    """With az_search_profile on, the sampled simulation steps run k_select / k_expand_backup apart and the
    others the fused k_expand_select: the same golden game either way."""
    ref = BY[name]
    m = handle(engine, ref)
    try:
        m.profile(True)
        play_and_compare(m, [ref], 1)
        p = m.profile_read()
        assert p["sim_steps"] > 0 and p["fused_launches"] > 0
    finally:
        m.close()


def plain_handle(engine, ref, **opts):
    import az_amd
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    return az_amd.ParallelMCTS(engine, n_games=1, board_size=bs, num_simulations=sims, c_puct=cp, fpu_reduction=fpu,
                               evaluator=az_amd.AZ_EVAL_HASH if ev == "hash" else az_amd.AZ_EVAL_RANDOM, eval_seed=es,
                               use_dirichlet_each_search=bool(nes), **opts)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [dict(use_td=True, td_lambda=1.0), dict(selection=3), dict(max_search_depth=96),
                                  dict(selection=1, max_search_depth=1000, use_td=False, use_widening=False)],
                         ids=["td-lambda-1", "rave", "depth-96", "defaults-spelled-out"])
def test_gpu_search_opts_that_are_the_plain_search(engine, opts):
    """TD with lambda = 1 is bitwise the plain backup, RAVE falls back to PUCT, and a cap the path capacity
    reaches first is no cap: each plays the existing plain golden game bit for bit."""
    ref = min(PLAIN_GAMES, key=lambda g: g["case"][1] * len(g["moves"]))
    m = plain_handle(engine, ref, **opts)
    try:
        play_and_compare(m, [ref], 1)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_search_opts_three_games_on_one_handle(engine):
    refs = [BY[f"td-seed{s}"] for s in (42, 43, 44)]
    assert len({tuple(m["action"] for m in g["moves"]) for g in refs}) == 3
    m = handle(engine, refs[0], n_games=3, noise_seed=42, noise_seed_stride=1)
    try:
        play_and_compare(m, refs, 3)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_search_opts_switch_on_a_live_handle(engine):
    """6 plies of PUCT, then PROGRESSIVE_BIAS + TD through az_search_set_options: the tree is kept (the
    golden game's statistics after the switch include the subtree searched before it)."""
    ref = BY["switch"]
    k = ref["switch_ply"]
    m = handle(engine, ref, opts={})
    try:
        assert m.searchOptions() == dict(selection=1, max_search_depth=1000, use_td=False, td_lambda=np.float32(0.8),
                                         use_widening=False, widening_min_visits=10, widening_base=2.0, widening_exponent=0.5)
        play_and_compare(m, [ref], 1, max_moves=k)
        before = m.rootNode(0)
        m.setSearchOptions(selection=ref["switch"]["selection"], use_td=bool(ref["switch"]["use_td"]),
                           td_lambda=ref["switch"]["td_lambda"])
        assert m.rootNode(0) == before and m.searchOptions()["selection"] == 2 and m.searchOptions()["use_td"]
        rest = dict(ref, moves=ref["moves"][k:], init_root=children_rows(m, 0))   # the root as it stands
        assert k % 2 == 0 and len(ref["moves"]) < 30          # the noise parity and T = 1 carry over
        play_and_compare(m, [rest], 1, start=False)
    finally:
        m.close()


def same_record(rec, ref, n=None):
    moves = ref["moves"][:n]
    assert [m.action for m in rec.moves] == [m["action"] for m in moves]
    assert [bits(m.policy) for m in rec.moves] == [m["probs"] for m in moves]
    assert [bits([m.value])[0] for m in rec.moves] == [m["value"] for m in moves]


@pytest.mark.gpu
def test_gpu_search_opts_selfplay_driver(engine):
    """az_selfplay_run under progressive widening: game 0's record is the golden game; az_selfplay_step with
    restarts on the Go case, whose game ends after two passes: every restart replays it."""
    import az_amd
    ref = BY["widening"]
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    sp = az_amd.SelfPlayManager(engine, numGames=1, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_HASH,
                                c_puct=cp, fpu_reduction=fpu, eval_seed=es, use_widening=True)
    try:
        same_record(sp.generateGames(1, max_moves=mm)[0], ref)
    finally:
        sp.mcts.close()
    ref = BY["widening-go"]
    assert ref["terminal"] and len(ref["moves"]) == 2
    m = handle(engine, ref)
    try:
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        for step in range(6):
            mv, _ = m.selfplayStep(restart_finished=True)
            (slot, md), = m.stepMoves()
            r = ref["moves"][step % 2]
            assert (mv, slot, md.action, bits(md.policy), bits([md.value])[0]) == (1, 0, r["action"], r["probs"], r["value"]), step
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_search_opts_arena_slot_trees_equal_single_handles(engine):
    """An arena with options: at every move of the first plies the mover's root children equal those of a
    single handle with the same net and options that is fed the same moves."""
    import az_amd
    import net_oracle
    bs, sims, opts = 9, 60, dict(selection=az_amd.AZ_SEL_PROGRESSIVE_BIAS, use_td=True, td_lambda=0.7, use_widening=True,
                                 widening_min_visits=4)
    nets = []
    for seed in (21, 22):
        desc = az_amd.gomoku_net_desc(board_size=bs, channels=32, blocks=1, max_batch=2)
        net = az_amd.HipNeuralNetwork(engine, desc)
        net.load_weights(net_oracle.init_blob(desc, seed=seed))
        nets.append(net)
    ar = az_amd.Arena(engine, nets[0], nets[1], 1, board_size=bs, num_simulations=sims, temperature=0.1, tt_log2=12, **opts)
    singles = [az_amd.ParallelMCTS(engine, n_games=1, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                                   net=nets[k], tt_log2=12, noise_seed_stride=1, **opts) for k in (0, 1)]
    seen, errors = [], []

    def on_move(gid, ply, total, moves):
        # called after the mover chose and before the move is applied; an exception here would not reach
        # pytest (a ctypes callback), so mismatches are collected
        try:
            k = ply % 2                                       # A moves first in game 0
            s = singles[k]
            s.search()
            mine, theirs = s.rootChildren(0), ar.search.rootChildren(k)
            for a, b in zip(mine, theirs):
                if (bits(a) if a.dtype == np.float32 else a.tolist()) != (bits(b) if b.dtype == np.float32 else b.tolist()):
                    errors.append((ply, "children"))
            if s.rootNode(0) != ar.search.rootNode(k):
                errors.append((ply, "root"))
            seen.append(int(mine[1].min()))
            act = s.select(True, 0.1)[0]                      # the arena's deterministic selectAction(true, T)
            for t in singles:                                 # the move goes to both trees of the table
                t.updateWithMove(act)
        except Exception as e:  # noqa: BLE001
            errors.append((ply, repr(e)))

    try:
        assert ar.search.searchOptions()["use_widening"] and ar.search.searchOptions()["selection"] == 2
        for k in (0, 1):
            singles[k].newGames(ids=[k])
        ar.progressCallback = on_move
        rec = ar.run(1, max_moves=6)[0]
        assert [m.action for m in rec.moves] and not errors, errors
    finally:
        ar.close()
        for s in singles:
            s.close()
        for n in nets:
            n.close()
    assert len(rec.moves) == 6 and len(seen) >= 1 and min(seen) < 0      # widening's negative counts were compared


@pytest.mark.gpu
def test_gpu_search_opts_search_group_and_setters():
    """A SearchGroup member plays what a standalone object with the group's options plays; a member whose
    setter names other options throws; the standalone object's setSelectionStrategy keeps its tree."""
    az = pytest.importorskip("_alphazero_cpp")
    cfg = az.MCTSConfig()
    cfg.numSimulations = 60
    cfg.selectionStrategy = az.MCTSNodeSelection.PROGRESSIVE_BIAS
    cfg.useTemporalDifference, cfg.tdLambda = True, 0.6
    cfg.useProgressiveWidening, cfg.minVisitsForWidening = True, 5
    root = az.GomokuState(9)
    for a in (40, 41, 31):
        root.makeMove(a)

    def stats(m, searches=1):
        m.setDeterministicMode(True)
        for _ in range(searches):
            m.search()
        r = m.getRootNode()
        return [r.visitCount, list(r.actions), [(c.visitCount, c.valueSum, c.prior) for c in r.children]]

    group = az.SearchGroup(None, cfg, az.GomokuState(9), 2)
    member = az.ParallelMCTS(root, group)
    alone = az.ParallelMCTS(root, cfg, None, None)
    got = stats(member)
    assert member.inGroup() and got == stats(alone) and min(c[0] for c in got[2]) < 0
    plain = az.MCTSConfig()
    plain.numSimulations = 60
    assert got != stats(az.ParallelMCTS(root, plain, None, None))
    with pytest.raises(Exception, match="options"):
        member.setSelectionStrategy(az.MCTSNodeSelection.PUCT)
    other = az.MCTSConfig()
    other.numSimulations, other.useTemporalDifference = 60, True
    with pytest.raises(Exception, match="options"):
        member.setConfig(other)
    assert member.inGroup() and group.members() == 1
    # setSelectionStrategy on a live tree: the visits stay (a rebuilt handle would start from an empty root),
    # and the next search plays the new strategy on top of them, as two handles driven alike agree
    n0 = alone.getRootNode().visitCount
    alone.setSelectionStrategy(az.MCTSNodeSelection.PUCT)
    assert alone.getRootNode().visitCount == n0 > 0
    alone.search()
    assert alone.getRootNode().visitCount == 2 * n0           # a root keeps one virtual loss per simulation


@pytest.mark.gpu
def test_gpu_self_play_binary_progressive_widening(tmp_path, engine):
    """self_play --progressive-widening plays with widening: its records equal an in-process widening run
    and differ from a run without the flag; the metadata says what was played."""
    import az_amd
    n, bs, sims = 2, 7, 48
    runs = {}
    for flag in (True, False):
        out = tmp_path / ("wid" if flag else "plain")
        r = subprocess.run([BIN, "--game", "gomoku", "--size", str(bs), "--num-games", str(n), "--simulations", str(sims),
                            "--batch-size", str(n), "--output-dir", str(out)] + (["--progressive-widening"] if flag else []),
                           capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout + r.stderr
        recs = []
        for g in range(n):
            (f,) = glob.glob(str(out / f"{g:03d}_*.json"))
            recs.append(json.load(open(f)))
        (md,) = glob.glob(str(out / "metadata_*.json"))
        assert json.load(open(md))["progressive_widening"] is flag
        runs[flag] = recs
    assert [[m["action"] for m in r["moves"]] for r in runs[True]] != [[m["action"] for m in r["moves"]] for r in runs[False]]
    sp = az_amd.SelfPlayManager(engine, numGames=n, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_RANDOM,
                                eval_seed=0, fpu_reduction=0.1, use_dirichlet_each_search=True, noise_seed_stride=1,
                                use_widening=True)
    try:
        mine = sp.generateGames(n)
    finally:
        sp.mcts.close()
    for rec, ref in zip(mine, runs[True]):
        assert [m.action for m in rec.moves] == [m["action"] for m in ref["moves"]]
        for m, rm in zip(rec.moves, ref["moves"]):
            p = np.asarray(m.policy, np.float32)
            assert [None if np.isnan(x) else float(x) for x in p] == rm["policy"]
        assert rec.result == ref["result"]


@pytest.mark.gpu
def test_gpu_search_opts_refusals_and_round_trip(engine):
    import az_amd
    from az_amd import _lib
    base = dict(n_games=1, board_size=9, num_simulations=8)
    bad = [(dict(selection=-1), "selection"), (dict(selection=4), "selection"), (dict(td_lambda=float("nan")), "td_lambda"),
           (dict(td_lambda=float("inf")), "td_lambda"), (dict(widening_base=0.0), "widening_base"),
           (dict(widening_base=-2.0), "widening_base"), (dict(widening_base=float("inf")), "widening_base"),
           (dict(widening_base=float("nan")), "widening_base"), (dict(widening_exponent=0.0), "widening_exponent"),
           (dict(widening_exponent=1.25), "widening_exponent"), (dict(widening_exponent=-0.5), "widening_exponent"),
           (dict(widening_exponent=float("nan")), "widening_exponent")]
    for opts, word in bad:
        with pytest.raises(az_amd.AzError, match=word) as e:
            az_amd.ParallelMCTS(engine, **base, **opts)
        assert e.value.code == _lib.AZ_ERR_ARG, opts
    # a refused construction leaves no handle behind
    def device_mem():
        b, n = ctypes.c_int64(), ctypes.c_int64()
        assert _lib.lib().az_diag_device_mem(ctypes.byref(b), ctypes.byref(n)) == 0
        return b.value, n.value

    mem = device_mem()
    with pytest.raises(az_amd.AzError):
        az_amd.ParallelMCTS(engine, **base, widening_exponent=2.0)
    assert device_mem() == mem
    opts = dict(selection=az_amd.AZ_SEL_UCB, max_search_depth=-3, use_td=True, td_lambda=-0.25, use_widening=True,
                widening_min_visits=0, widening_base=0.75, widening_exponent=1.0)
    m = az_amd.ParallelMCTS(engine, **base, **opts)
    try:
        assert m.searchOptions() == opts
        for o, word in bad:                                   # refused on the live handle too, which stays as it was
            with pytest.raises(az_amd.AzError, match=word) as e:
                m.setSearchOptions(**o)
            assert e.value.code == _lib.AZ_ERR_ARG and m.searchOptions() == opts
        # a depth cap <= 0 makes the root the leaf: the search expands the root and descends no further
        m.newGames()
        m.search()
        assert m.rootNode(0)[0] == 8 * (1 + 3) and m.rootChildren(0)[1].max() <= 0 and m.counters(0)["evals"] == 1
        m.setSearchOptions(max_search_depth=1000, use_widening=False, selection=az_amd.AZ_SEL_PUCT, use_td=False)
        assert m.searchOptions() == dict(opts, max_search_depth=1000, use_widening=False, selection=1, use_td=False)
        # az_search_set_params leaves the options alone; a null az_search_set_options is the defaults
        cfg = _lib.SearchCfg.from_buffer_copy(m.cfg)
        cfg.num_simulations = 4
        now = m.searchOptions()
        assert _lib.lib().az_search_set_params(m.h, ctypes.byref(cfg)) == 0 and m.searchOptions() == now
        assert _lib.lib().az_search_set_options(m.h, None) == 0
        assert m.searchOptions() == dict(az_amd.SEARCH_OPT_DEFAULTS, td_lambda=np.float32(0.8))
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_search_opts_truncated_widening_table_is_a_capacity_error(engine):
    """A widening table cut short (the test-only limit) and a visit count past it: the sticky capacity
    error, not a guessed count."""
    import az_amd
    from az_amd import _lib
    old = _lib.lib().az_diag_set_widening_cap(16)
    try:
        m = az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=64, use_widening=True, widening_base=1.0)
        try:
            m.newGames()
            with pytest.raises(az_amd.AzError, match="capacity") as e:
                m.search()
            assert e.value.code == _lib.AZ_ERR_CAPACITY
        finally:
            m.close()
    finally:
        _lib.lib().az_diag_set_widening_cap(old)
    # the whole table: the same search runs
    m = az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=64, use_widening=True, widening_base=1.0)
    try:
        m.newGames()
        m.search()
        assert m.rootNode(0)[0] == 64 * (1 + 3)           # a root keeps one virtual loss (3) per simulation
    finally:
        m.close()
