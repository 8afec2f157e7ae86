"""GPU parity of the Go rule options (az_search_cfg go_komi / go_chinese_rules / go_superko: komi,
Chinese area or Japanese territory scoring with the reference's prisoner crediting, positional
superko or the ko point only) against golden vectors of the patched REFERENCE search and GoState
under those settings (tests/golden/ref_go_rules_games.json.gz, ref_go_rules_positions.json.gz,
written by tests/golden/gen_go_rules_golden.py).  Bit-exact, as tests/test_gpu_go.py."""
import ctypes
import gzip
import json
import os
import struct

import numpy as np
import pytest

from test_gpu_search import play_and_compare

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with gzip.open(os.path.join(GOLD, "ref_go_rules_games.json.gz"), "rt") as _f:
    GAMES = json.load(_f)
with gzip.open(os.path.join(GOLD, "ref_go_rules_positions.json.gz"), "rt") as _f:
    POSITIONS = json.load(_f)
KO_LIST = [3, 9, 11, 10, 1, -1, 0, 2]


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def case_id(g):
    return f"{g['case'][0]}x{g['case'][1]}-komi{g['rules'][0]}-{'cn' if g['rules'][1] else 'jp'}-" \
           f"{'superko' if g['rules'][2] else 'ko'}-seed{g['noise_seed']}-tt{g['tt_log2']}"


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def handle(engine, ref, n_games=1, **kw):
    import az_amd
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    komi, chinese, superko = ref["rules"]
    return az_amd.ParallelMCTS(engine, n_games=n_games, board_size=bs, num_simulations=sims, c_puct=cp, fpu_reduction=fpu,
                               evaluator=az_amd.AZ_EVAL_HASH, eval_seed=es, use_dirichlet_each_search=bool(nes),
                               tt_log2=ref["tt_log2"], game=az_amd.AZ_GAME_GO, go_komi=komi,
                               go_chinese_rules=bool(chinese), go_superko=bool(superko), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(GAMES)), ids=[case_id(g) for g in GAMES])
def test_gpu_go_rules_search_matches_reference_golden(engine, idx):
    ref = GAMES[idx]
    m = handle(engine, ref, noise_seed=ref["noise_seed"])
    try:
        assert m.goRules() == (ref["rules"][0], bool(ref["rules"][1]), bool(ref["rules"][2]))
        play_and_compare(m, [ref], 1)
    finally:
        m.close()


def test_golden_games_cover_the_rules():
    """What the fixtures exist for (the generator asserts the same on the reference's output)."""
    with gzip.open(os.path.join(GOLD, "ref_go_games.json.gz"), "rt") as f:
        d3 = [g for g in json.load(f) if g["case"][4] == 3][0]
    assert any(g["case"][4] == 3 and [m["action"] for m in g["moves"]] != [m["action"] for m in d3["moves"]] for g in GAMES)
    for chinese in (0, 1):
        assert any(g["rules"][1] == chinese and g["terminal"] and g["result"] != 0 for g in GAMES)
    k0 = [g for g in GAMES if g["rules"][0] == 0.0][0]
    assert k0["terminal"] and k0["result"] == 1                      # komi 0, empty board: DRAW
    assert any(g["tt_log2"] == 6 for g in GAMES) and any(g["case"][0] == 13 for g in GAMES)


@pytest.mark.gpu
def test_gpu_go_rules_three_games_on_one_handle(engine):
    """The three-seed case on one handle with stride 1: game g draws its noise from seed 42 + g and keeps
    capture counters of its own."""
    refs = [g for g in GAMES if g["noise_seed"] in (43, 44)]
    refs = [g for g in GAMES if g["noise_seed"] == 42 and g["case"] == refs[0]["case"] and g["rules"] == refs[0]["rules"]
            and g["tt_log2"] == refs[0]["tt_log2"]] + refs
    assert [g["noise_seed"] for g in refs] == [42, 43, 44]
    assert len({tuple(m["action"] for m in g["moves"]) for g in refs}) == 3
    m = handle(engine, refs[0], n_games=3, noise_seed=42, noise_seed_stride=1)
    try:
        play_and_compare(m, refs, 3)
    finally:
        m.close()


def position_cases():
    out = []
    for key in sorted(POSITIONS):
        bs = 9 if key == "ko" else int(key.split("-")[0])
        out += [(f"{key}[{i}]", bs, p) for i, p in enumerate(POSITIONS[key])]
    return out


@pytest.mark.gpu
def test_gpu_go_rules_positions(engine):
    """Every position fixture on a one-game handle: the moves applied, then a one-simulation search -- the
    root's children are the fixture's legal list in order; a finished position reports the fixture's
    result.  The constructed send-two-return-one position is in the list under both ko rules."""
    import az_amd
    handles = {}
    try:
        for name, bs, p in position_cases():
            rules = (f32(p["komi_bits"]), bool(p["chinese"]), bool(p["superko"]))
            key = (bs,) + rules
            if key not in handles:
                handles[key] = az_amd.ParallelMCTS(engine, n_games=1, board_size=bs, num_simulations=1,
                                                   evaluator=az_amd.AZ_EVAL_HASH, tt_log2=8, game=az_amd.AZ_GAME_GO,
                                                   go_komi=rules[0], go_chinese_rules=rules[1], go_superko=rules[2])
            m = handles[key]
            m.newGames()
            term, res = [0], [0]
            for a in p["moves"]:
                assert not term[0], name
                term, res = m.updateWithMove(np.array([a], np.int32))
            assert int(term[0]) == p["terminal"], name
            if p["terminal"]:
                assert int(res[0]) == p["result"], (name, "result")
                continue
            m.search()
            act = m.rootChildren(0)[0]
            assert [int(a) for a in act] == p["legal"], (name, "legal")
    finally:
        for m in handles.values():
            m.close()
    sk, simple = POSITIONS["ko"]
    assert sk["moves"] == simple["moves"] == KO_LIST and set(simple["legal"]) - set(sk["legal"]) == {1}


@pytest.mark.gpu
def test_gpu_go_rules_selfplay_driver(engine):
    """az_selfplay_run on a (7.0, Japanese, simple ko) handle: game 0's record is the golden game."""
    import az_amd
    ref = [g for g in GAMES if g["rules"] == [7.0, 0, 0] and g["tt_log2"] == 6][0]
    bs, sims, mm, ev, es, nes, cp, fpu = ref["case"]
    sp = az_amd.SelfPlayManager(engine, numGames=1, numSimulations=sims, board_size=bs, evaluator=az_amd.AZ_EVAL_HASH,
                                c_puct=cp, fpu_reduction=fpu, eval_seed=es, tt_log2=6, game=az_amd.AZ_GAME_GO,
                                go_komi=7.0, go_chinese_rules=False, go_superko=False)
    try:
        rec = sp.generateGames(1, max_moves=mm)[0]
    finally:
        sp.mcts.close()
    assert [m.action for m in rec.moves] == [m["action"] for m in ref["moves"]]
    assert [np.asarray(m.policy, np.float32).view(np.uint32).tolist() for m in rec.moves] == [m["probs"] for m in ref["moves"]]
    assert rec.result == ref["result"]


@pytest.mark.gpu
def test_gpu_go_rules_arena(engine):
    """Two tables under (5.5, Japanese, simple ko) played to the end: every game's result is the host GoState's
    for the recorded moves under the same rules (which replay without an illegal move)."""
    import az_amd
    import net_oracle
    az = pytest.importorskip("_alphazero_cpp")
    bs, T, rules = 9, 2, (5.5, False, False)
    nets = []
    for seed in (9, 10):
        desc = az_amd.NetDesc(bs, 8, 128, 1, bs * bs + 1, 32, 8, 256, 1, 0, az_amd.AZ_PREC_FP16, T)
        net = az_amd.HipNeuralNetwork(engine, desc)
        net.load_weights(net_oracle.init_blob(desc, seed=seed))
        nets.append(net)
    ar = az_amd.Arena(engine, nets[0], nets[1], T, board_size=bs, num_simulations=120, swap_colors=True, noise_eps=0.25,
                      tt_log2=12, game=az_amd.AZ_GAME_GO, go_komi=rules[0], go_chinese_rules=rules[1], go_superko=rules[2])
    try:
        assert ar.search.goRules() == rules
        recs = ar.run(T)
    finally:
        ar.close()
        for n in nets:
            n.close()
    assert len(recs) == T
    unequal = 0
    for r in recs:
        s = az.GoState(bs, *rules)
        for mv in r.moves:
            s.makeMove(mv.action)
        assert s.isTerminal() and r.result == int(s.getGameResult()) != 0, r.game_id
        unequal += s.getCapturedStones(1) != s.getCapturedStones(2)
        print(f"arena game {r.game_id}: {len(r.moves)} moves, captures {s.getCapturedStones(1)}/{s.getCapturedStones(2)}, "
              f"score {s.calculateScore()}, result {r.result}")
    assert unequal                     # a game whose territory score depends on who is credited with the prisoners


@pytest.mark.gpu
def test_gpu_go_rules_pybind_callback_evaluator():
    """The host ParallelMCTS on GoState(9, 7.5, Chinese, simple ko) with a Python evaluator: the handle takes the
    state's rules, and every host replay (the callback's leaf states) plays them -- through the constructed
    list and then point 1, which only simple ko allows."""
    az = pytest.importorskip("_alphazero_cpp")
    from test_gpu_callback_eval import _hash_eval

    class HashEvaluator(az.NeuralNetwork):
        def __init__(self):
            super().__init__()
            self.calls = 0

        def predict(self, state):
            self.calls += 1
            assert not state.isEnforcingSuperko() and state.getKomi() == 7.5
            return _hash_eval(state.getHash(), list(state.getMoveHistory()), state.getActionSpaceSize())

    net = HashEvaluator()
    host = az.GoState(9, 7.5, True, False)
    m = az.ParallelMCTS(host, net, None, 1, 40, 1.5, 0.0, 3)
    m.setDeterministicMode(True)
    for a in KO_LIST + [1]:
        host.makeMove(a)
        m.updateWithMove(a)
    m.search()
    r = m.getRootNode()
    assert list(r.actions) == host.getLegalMoves() and r.visitCount > 0 and net.calls > 0
    # the same list under superko: point 1 is refused by the host state
    with pytest.raises(Exception):
        sk = az.GoState(9, 7.5, True, True)
        for a in KO_LIST + [1]:
            sk.makeMove(a)


@pytest.mark.gpu
def test_gpu_go_rules_search_group():
    """A SearchGroup takes its prototype's rules; a member replays its history under them (point 1 after the
    constructed list: simple ko only) and plays what a standalone object plays; a state with other rules is
    refused."""
    az = pytest.importorskip("_alphazero_cpp")
    cfg = az.MCTSConfig()
    cfg.numSimulations = 40
    root = az.GoState(9, 6.5, False, False)
    for a in KO_LIST + [1]:
        root.makeMove(a)

    def stats(m):
        m.setDeterministicMode(True)
        m.search()
        r = m.getRootNode()
        return [r.visitCount, list(r.actions), [(c.visitCount, c.valueSum, c.prior) for c in r.children]]

    group = az.SearchGroup(None, cfg, az.GoState(9, 6.5, False, False), 2)
    member = az.ParallelMCTS(root, group)
    assert member.inGroup()
    got = stats(member)
    assert got[1] == root.getLegalMoves() and got == stats(az.ParallelMCTS(root, cfg, None, None))
    for other in (az.GoState(9), az.GoState(9, 6.5, True, False), az.GoState(9, 6.5, False, True), az.GoState(9, 7.0, False, False)):
        with pytest.raises(Exception, match="rules"):
            az.ParallelMCTS(other, group)
    assert group.members() == 1


@pytest.mark.gpu
def test_gpu_go_rules_argument_errors(engine):
    import az_amd
    from az_amd import _lib
    with pytest.raises(az_amd.AzError, match="Gomoku") as e:
        az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=8, go_komi=6.5)
    assert e.value.code == _lib.AZ_ERR_ARG
    for bad in (float("nan"), float("inf"), 1024.5, -2000.0):
        with pytest.raises(az_amd.AzError, match="komi") as e:
            az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=8, game=az_amd.AZ_GAME_GO, go_komi=bad)
        assert e.value.code == _lib.AZ_ERR_ARG
    m = az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=8, game=az_amd.AZ_GAME_GO, go_komi=0.0,
                            go_chinese_rules=False)
    try:
        assert m.goRules() == (0.0, False, True)                      # komi 0 is a komi, not "unset"
        cfg = _lib.SearchCfg.from_buffer_copy(m.cfg)
        cfg.num_simulations = 4
        assert _lib.lib().az_search_set_params(m.h, ctypes.byref(cfg)) == 0          # the same rules: accepted
        for field, value in (("go_komi", 0.5), ("go_chinese_rules", 1), ("go_superko", 0), ("go_rules", 0),
                             ("go_komi", float("nan"))):
            other = _lib.SearchCfg.from_buffer_copy(cfg)
            setattr(other, field, value)
            assert _lib.lib().az_search_set_params(m.h, ctypes.byref(other)) == _lib.AZ_ERR_ARG, field
            assert b"rules" in _lib.lib().az_last_error()
        assert m.goRules() == (0.0, False, True)
    finally:
        m.close()
    # a default-rules handle: zero-initialised fields and the defaults spelled out are the same rules
    d = az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=8, game=az_amd.AZ_GAME_GO)
    try:
        assert d.goRules() == (7.5, True, True)
        z = _lib.SearchCfg.from_buffer_copy(d.cfg)
        z.go_rules, z.go_komi, z.go_chinese_rules, z.go_superko = 0, 0.0, 0, 0
        assert _lib.lib().az_search_set_params(d.h, ctypes.byref(z)) == 0
    finally:
        d.close()
