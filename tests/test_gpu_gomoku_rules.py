"""GPU parity of the Gomoku rule variants (az_search_set_gomoku_rules: Renju, Omok) against golden vectors of
the patched REFERENCE search and GomokuState under those rules (tests/golden/ref_gomoku_rules_games.json.gz,
ref_gomoku_rules_positions.json.gz, written by tests/golden/gen_gomoku_rules_golden.py).  Bit-exact, as
tests/test_gpu_search.py: the forbidden cells are missing from every Black-to-move node's children, Black
without a legal cell is a DRAW, and the rules' feature keys are part of every hash (transposition slots,
hits and the hash evaluator's outputs)."""
import ctypes
import gzip
import json
import os

import numpy as np
import pytest

from test_gpu_search import play_and_compare

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with gzip.open(os.path.join(GOLD, "ref_gomoku_rules_games.json.gz"), "rt") as _f:
    GAMES = json.load(_f)
with gzip.open(os.path.join(GOLD, "ref_gomoku_rules_positions.json.gz"), "rt") as _f:
    POSITIONS = json.load(_f)
DEFAULT_OPTS = [1, 1000, 0, 0.8]


def case_id(g):
    rules = "+".join(n for n, on in zip(("renju", "omok"), g["rules"]) if on)
    return f"{g['case'][0]}x{g['case'][1]}-{rules}-seed{g['noise_seed']}-tt{g['tt_log2']}" + \
           ("" if g["opts"] == DEFAULT_OPTS else "-opts")


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def handle(engine, ref, n_games=1, **kw):
    import az_amd
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    sel, depth, td, lam = ref["opts"]
    opts = {} if ref["opts"] == DEFAULT_OPTS else dict(selection=sel, max_search_depth=depth, use_td=bool(td), td_lambda=lam)
    return az_amd.ParallelMCTS(engine, n_games=n_games, board_size=bs, num_simulations=sims, c_puct=cp, fpu_reduction=fpu,
                               evaluator=az_amd.AZ_EVAL_HASH, eval_seed=es, use_dirichlet_each_search=bool(nes),
                               tt_log2=ref["tt_log2"], gomoku_renju=bool(ref["rules"][0]), gomoku_omok=bool(ref["rules"][1]),
                               **opts, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(GAMES)), ids=[case_id(g) for g in GAMES])
def test_gpu_gomoku_rules_search_matches_reference_golden(engine, idx):
    ref = GAMES[idx]
    m = handle(engine, ref, noise_seed=ref["noise_seed"])
    try:
        assert m.gomokuRules() == (bool(ref["rules"][0]), bool(ref["rules"][1]))
        play_and_compare(m, [ref], 1)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_gomoku_rules_three_games_on_one_handle(engine):
    """The three-seed Renju case on one handle with stride 1: game g draws its noise from seed 42 + g."""
    refs = [g for g in GAMES if g["noise_seed"] in (43, 44)]
    refs = [g for g in GAMES if g["noise_seed"] == 42 and g["case"] == refs[0]["case"] and g["rules"] == refs[0]["rules"]
            and g["tt_log2"] == refs[0]["tt_log2"] and g["opts"] == refs[0]["opts"]] + refs
    assert [g["noise_seed"] for g in refs] == [42, 43, 44]
    assert len({tuple(m["action"] for m in g["moves"]) for g in refs}) == 3
    m = handle(engine, refs[0], n_games=3, noise_seed=42, noise_seed_stride=1)
    try:
        play_and_compare(m, refs, 3)
    finally:
        m.close()


def position_cases():
    return [(f"{key}[{i}]", p) for key in sorted(POSITIONS) for i, p in enumerate(POSITIONS[key])]


@pytest.mark.gpu
def test_gpu_gomoku_rules_positions(engine):
    """Every position fixture on a one-game handle: the moves applied, then a one-simulation search -- the root's
    children are the fixture's legal list in order; a finished position reports the fixture's result, Black's
    stalemate with empty cells left (DRAW) and the constructed overline / double-four / double-three cells included."""
    import az_amd
    handles = {}
    seen = set()
    try:
        for name, p in position_cases():
            key = (p["bs"], p["renju"], p["omok"])
            if key not in handles:
                handles[key] = az_amd.ParallelMCTS(engine, n_games=1, board_size=p["bs"], num_simulations=1,
                                                   evaluator=az_amd.AZ_EVAL_HASH, tt_log2=8, gomoku_renju=bool(p["renju"]),
                                                   gomoku_omok=bool(p["omok"]))
            m = handles[key]
            m.newGames()
            term, res = [0], [0]
            for a in p["moves"]:
                assert not term[0], name
                term, res = m.updateWithMove(np.array([a], np.int32))
            assert int(term[0]) == p["terminal"], name
            if p["terminal"]:
                assert int(res[0]) == p["result"], (name, "result")
                seen.add("stalemate" if p["result"] == 1 and len(p["moves"]) < p["bs"] ** 2 else "over")
                continue
            m.search()
            act = m.rootChildren(0)[0]
            assert [int(a) for a in act] == p["legal"], (name, "legal")
            if p["player"] == 1 and len(p["legal"]) < p["bs"] ** 2 - len(p["moves"]):
                seen.add(("forbidden", p["renju"], p["omok"]))
    finally:
        for m in handles.values():
            m.close()
    assert {"stalemate", ("forbidden", 1, 0), ("forbidden", 0, 1), ("forbidden", 1, 1)} <= seen


@pytest.mark.gpu
def test_gpu_gomoku_rules_selfplay_driver(engine):
    """az_selfplay_run on a Renju handle: game 0's record is the golden game (a 7x7 game played to its end)."""
    import az_amd
    ref = [g for g in GAMES if g["rules"] == [1, 0] and g["case"][0] == 7][0]
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    sp = az_amd.SelfPlayManager(engine, numGames=1, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_HASH,
                                c_puct=cp, fpu_reduction=fpu, eval_seed=es, tt_log2=ref["tt_log2"], gomoku_renju=True)
    try:
        assert sp.mcts.gomokuRules() == (True, False)
        rec = sp.generateGames(1, max_moves=mm)[0]
    finally:
        sp.mcts.close()
    assert [m.action for m in rec.moves] == [m["action"] for m in ref["moves"]]
    assert [np.asarray(m.policy, np.float32).view(np.uint32).tolist() for m in rec.moves] == [m["probs"] for m in ref["moves"]]
    assert rec.result == ref["result"]


@pytest.mark.gpu
def test_gpu_gomoku_rules_argument_errors(engine):
    import az_amd
    from az_amd import _lib
    L = _lib.lib()
    with pytest.raises(az_amd.AzError, match="Go handle") as e:
        az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=8, game=az_amd.AZ_GAME_GO, gomoku_renju=True)
    assert e.value.code == _lib.AZ_ERR_ARG
    m = az_amd.ParallelMCTS(engine, n_games=1, board_size=15, num_simulations=8)
    try:
        assert m.gomokuRules() == (False, False)
        assert L.az_search_set_gomoku_rules(m.h, ctypes.byref(_lib.GomokuRules(1, 0, 1))) == _lib.AZ_ERR_ARG
        assert b"pro-long" in L.az_last_error()
        assert L.az_search_set_gomoku_rules(m.h, ctypes.byref(_lib.GomokuRules(0, 1, 0))) == 0
        assert m.gomokuRules() == (False, True)
        assert L.az_search_set_gomoku_rules(m.h, ctypes.byref(_lib.GomokuRules(1, 0, 0))) == 0       # nothing has moved yet
        m.newGames()                                                                                 # keeps the rules
        assert m.gomokuRules() == (True, False)
        # the constructed overline position: (7, 5) would make six in a row
        p = [q for q in POSITIONS["constructed"] if q["name"] == "overline"][0]
        for a in p["moves"]:
            m.updateWithMove(np.array([a], np.int32))
        assert L.az_search_set_gomoku_rules(m.h, ctypes.byref(_lib.GomokuRules(0, 0, 0))) == _lib.AZ_ERR_STATE
        with pytest.raises(az_amd.AzError, match="forbidden") as e:
            m.updateWithMove(np.array([7 * 15 + 5], np.int32))
        assert e.value.code == _lib.AZ_ERR_ARG
        m.search()                                                      # the refused move left the game as it was
        assert [int(a) for a in m.rootChildren(0)[0]] == p["legal"]
        cfg = _lib.SearchCfg.from_buffer_copy(m.cfg)
        cfg.num_simulations = 4
        assert L.az_search_set_params(m.h, ctypes.byref(cfg)) == 0 and L.az_search_clear_tt(m.h) == 0
        m.setSearchOptions(use_td=True)
        assert m.gomokuRules() == (True, False)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_default_rules_after_setting_none_play_the_standard_game(engine):
    """az_search_set_gomoku_rules({0, 0, 0}) on a new handle: tests/golden/ref_games.json.gz case 0 bit for bit."""
    import az_amd
    from az_amd import _lib
    from test_gpu_search import GAMES as STANDARD
    ref = STANDARD[0]
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    m = az_amd.ParallelMCTS(engine, n_games=1, board_size=bs, num_simulations=sims, c_puct=cp, fpu_reduction=fpu,
                            evaluator=az_amd.AZ_EVAL_HASH if ev == "hash" else az_amd.AZ_EVAL_RANDOM, eval_seed=es,
                            use_dirichlet_each_search=bool(nes))
    try:
        assert _lib.lib().az_search_set_gomoku_rules(m.h, ctypes.byref(_lib.GomokuRules(0, 0, 0))) == 0
        assert m.gomokuRules() == (False, False)
        play_and_compare(m, [ref], 1)
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_host_self_play_manager_variant_plays_renju():
    """SelfPlayManager.generateGames(GOMOKU, 9, True) through pybind: the records are flagged variant and replay on
    the host Renju state without a throw, to the result the record holds."""
    az = pytest.importorskip("_alphazero_cpp")
    total, bs = 3, 9
    mgr = az.SelfPlayManager(az.RandomPolicyNetwork(az.GameType.GOMOKU, bs, 5), total, 48, 4)
    recs = mgr.generateGames(az.GameType.GOMOKU, bs, True)
    assert len(recs) == total
    for rec in recs:
        t, b, variant = rec.getMetadata()
        assert (t, b, variant) == (az.GameType.GOMOKU, bs, True)
        s = az.GomokuState.withRules(bs, True, False)
        for k, mv in enumerate(rec.getMoves()):
            assert not s.isTerminal()
            assert len(mv.policy) == len(s.getLegalMoves()), k        # the children are the Renju state's legal moves
            s.makeMove(mv.action)
        assert s.isTerminal() and int(s.getGameResult()) == int(rec.getResult()) != 0
    with pytest.raises(Exception, match="variant"):
        mgr.generateGames(az.GameType.GO, 9, True)
    # a dataset takes the flagged records: the planes do not depend on the rules
    ds = az.Dataset()
    for rec in recs:
        ds.addGameRecord(rec)
    ds.extractExamples(False)
    assert ds.size() == sum(len(r.getMoves()) for r in recs)


@pytest.mark.gpu
def test_gpu_gomoku_rules_arena(engine):
    """Two tables under Omok played to the end: every recorded move is legal for the host Omok state, and every
    game's result is that state's."""
    import az_amd
    import net_oracle
    az = pytest.importorskip("_alphazero_cpp")
    bs, T = 9, 2
    nets = []
    for seed in (9, 10):
        desc = az_amd.gomoku_net_desc(board_size=bs, channels=32, blocks=2, max_batch=4)
        net = az_amd.HipNeuralNetwork(engine, desc)
        net.load_weights(net_oracle.init_blob(desc, seed=seed))
        nets.append(net)
    ar = az_amd.Arena(engine, nets[0], nets[1], T, board_size=bs, num_simulations=64, swap_colors=True, noise_eps=0.25,
                      tt_log2=12, gomoku_omok=True)
    try:
        assert ar.search.gomokuRules() == (False, True)
        recs = ar.run(T)
    finally:
        ar.close()
        for n in nets:
            n.close()
    assert len(recs) == T
    for r in recs:
        s = az.GomokuState.withRules(bs, False, True)
        for mv in r.moves:
            assert s.isLegalMove(mv.action), (r.game_id, mv.action)
            s.makeMove(mv.action)
        assert s.isTerminal() and r.result == int(s.getGameResult()) != 0, r.game_id


@pytest.mark.gpu
def test_gpu_gomoku_rules_host_objects():
    """The host ParallelMCTS takes its state's rules (a Renju root after the constructed overline position: the
    forbidden cell is no child), a SearchGroup its prototype's; a member whose state names other rules is refused."""
    az = pytest.importorskip("_alphazero_cpp")
    p = [q for q in POSITIONS["constructed"] if q["name"] == "overline"][0]
    cfg = az.MCTSConfig()
    cfg.numSimulations = 24
    root = az.GomokuState.withRules(15, True, False)
    for a in p["moves"]:
        root.makeMove(a)

    def stats(m):
        m.setDeterministicMode(True)
        m.search()
        r = m.getRootNode()
        return [r.visitCount, list(r.actions), [(c.visitCount, c.valueSum, c.prior) for c in r.children]]

    alone = stats(az.ParallelMCTS(root, cfg, None, None))
    assert alone[1] == p["legal"] and 7 * 15 + 5 not in alone[1]
    group = az.SearchGroup(None, cfg, az.GomokuState.withRules(15, True, False), 2)
    member = az.ParallelMCTS(root, group)
    assert member.inGroup() and stats(member) == alone
    for other in (az.GomokuState(15), az.GomokuState.withRules(15, False, True), az.GomokuState.withRules(15, True, True)):
        with pytest.raises(Exception, match="rules"):
            az.ParallelMCTS(other, group)
    assert group.members() == 1
