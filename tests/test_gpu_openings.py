"""Openings on the device: az_search_new_games_moves starts the listed slots and plays each slot's move sequence
in one launch (k_open_games).  Its contract is equivalence: afterwards the handle behaves, bit for bit, as after
az_search_new_games_ids on the same slots and ids followed by one az_search_apply per move -- checked here by
playing two handles of one configuration side by side (AZ_EVAL_HASH, so every result depends on the position
hash and the move history; root noise in every search, so the host's generators count too).  Every move is
judged against the rules first and a refused call leaves the handle exactly as it was."""
import ctypes

import numpy as np
import pytest

SIMS = 16
KO_LIST = [3, 9, 11, 10, 1, -1, 0, 2]      # tests/test_gpu_go_rules.py: after it, point 1 repeats a position
# Go 9x9 (point = 9 row + column): Black 79 / 71 capture the corner stone 80, White 10 goes into the mouth of
# Black 1 / 9 / 19, Black passes, and Black 11 takes 10 back in a ko -- 10 is then the ko point
GO_SEQ = [1, 2, 9, 12, 19, 20, 79, 80, 71, 10, -1, 40, 11]
# Renju 9x9: Black 37 38 39 . 41 42 on row 4 -- from ply 10 on cell 40 would be an overline
RENJU_SEQ = [37, 0, 38, 2, 39, 4, 41, 6, 42, 8, 20, 22]
FIVE = [0, 9, 1, 10, 2, 11, 3, 12, 4]      # Black's row 0 .. 4: the ninth ply wins


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def handle(engine, n_games, **kw):
    import az_amd
    return az_amd.ParallelMCTS(engine, n_games=n_games, board_size=9, num_simulations=SIMS, evaluator=az_amd.AZ_EVAL_HASH,
                               tt_log2=8, noise_seed=42, noise_seed_stride=1, use_dirichlet_each_search=True, **kw)


def snapshot(m):
    """Everything the C ABI reads back of every slot: root children (N, VL, W and P bits, actions), the root
    node, its flags and the five counters."""
    from az_amd import _lib
    out = []
    for g in range(m.G):
        act, N, VL, W, P = m.rootChildren(g)
        fl = ctypes.c_int()
        _lib.check(_lib.lib().az_search_root_flags(m.h, g, ctypes.byref(fl)))
        rn = m.rootNode(g)
        out.append((act.tolist(), N.tolist(), VL.tolist(), W.view(np.uint32).tolist(), P.view(np.uint32).tolist(),
                    (rn[0], rn[1], np.float32(rn[2]).view(np.uint32).item()), fl.value, m.counters(g)))
    return out


def compose(m, seqs, ids):
    """The state new_games_moves must reproduce: fresh games, then one az_search_apply per ply."""
    m.newGames(ids=ids)
    for ply in range(max(len(q) for q in seqs)):
        m.updateWithMove(np.array([q[ply] if ply < len(q) else m.none for q in seqs], np.int32))


def play_both(a, b, rounds=3):
    """`rounds` moves on both handles -- search, select, apply -- with every readback equal after each step."""
    assert snapshot(a) == snapshot(b), "start"
    first = None
    for r in range(rounds):
        a.search()
        b.search()
        assert snapshot(a) == snapshot(b), ("search", r)
        sa, sb = a.select(True, 1.0), b.select(True, 1.0)
        assert sa[0].tolist() == sb[0].tolist(), ("actions", r)
        assert sa[1].view(np.uint32).tolist() == sb[1].view(np.uint32).tolist(), ("values", r)
        assert sa[4].tolist() == sb[4].tolist(), ("n_children", r)
        for g, k in enumerate(sa[4]):                          # probabilities and child actions: the first n_children
            assert sa[2][g, :k].view(np.uint32).tolist() == sb[2][g, :k].view(np.uint32).tolist(), ("probs", r, g)
            assert sa[3][g, :k].tolist() == sb[3][g, :k].tolist(), ("child actions", r, g)
        ta, tb = a.updateWithMove(sa[0]), b.updateWithMove(sb[0])
        assert ta[0].tolist() == tb[0].tolist() and ta[1].tolist() == tb[1].tolist(), ("apply", r)
        assert snapshot(a) == snapshot(b), ("apply", r)
        first = sa[0] if first is None else first
    return first


def equivalent(engine, seqs, ids, **kw):
    a, b = handle(engine, len(seqs), **kw), handle(engine, len(seqs), **kw)
    try:
        a.new_games_moves(seqs, ids=ids)
        compose(b, seqs, ids)
        first = play_both(a, b)
        assert sum(int(x) != a.none for x in first) >= len(seqs) - 1     # the opened games were searched and moved
        # a second start in the same slots: trees, tables, counters and generators begin again
        a.new_games_moves(seqs[::-1], ids=ids)
        compose(b, seqs[::-1], ids)
        play_both(a, b, rounds=1)
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_gpu_openings_gomoku_equivalence(engine):
    """Sequences of 0, 1, 6 and 8 plies (the last wraps the six-move history) under stream ids of their own."""
    seqs = [[], [40], [40, 41, 31, 32, 49, 50], [40, 41, 31, 32, 49, 50, 22, 58]]
    equivalent(engine, seqs, [5, 6, 7, 8])


@pytest.mark.gpu
@pytest.mark.parametrize("superko", [True, False], ids=["superko", "simple-ko"])
def test_gpu_openings_go_equivalence(engine, superko):
    """A capture, a ko capture and a pass; a slot whose sequence ends in a pass (one more ends the game), one that
    is a single pass and one fresh."""
    import az_amd
    seqs = [GO_SEQ, [40, -1], [-1], []]
    equivalent(engine, seqs, None, game=az_amd.AZ_GAME_GO, go_superko=superko)


@pytest.mark.gpu
@pytest.mark.parametrize("superko", [True, False], ids=["superko", "simple-ko"])
def test_gpu_openings_go_ko_recapture_refused(engine, superko):
    """White's immediate recapture at the ko point: refused as the thirteenth ply of a sequence, and refused by
    az_search_apply on the handle that was composed move by move."""
    import az_amd
    from az_amd import _lib
    a = handle(engine, 1, game=az_amd.AZ_GAME_GO, go_superko=superko)
    b = handle(engine, 1, game=az_amd.AZ_GAME_GO, go_superko=superko)
    try:
        a.newGames()
        before = snapshot(a)
        with pytest.raises(az_amd.AzError, match=r"entry 0 .*ply 13.*ko") as e:
            a.new_games_moves([GO_SEQ + [10]])
        assert e.value.code == _lib.AZ_ERR_ARG
        assert snapshot(a) == before
        compose(b, [GO_SEQ], None)
        with pytest.raises(az_amd.AzError, match="ko") as e:
            b.updateWithMove(np.array([10], np.int32))
        assert e.value.code == _lib.AZ_ERR_ARG
        a.new_games_moves([GO_SEQ])
        play_both(a, b, rounds=1)                              # the refused move left the composed handle as it was
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_gpu_openings_renju(engine):
    """A sequence through positions in which a cell is forbidden to Black; the same sequence with Black's next
    move on that cell is refused."""
    import az_amd
    from az_amd import _lib
    equivalent(engine, [RENJU_SEQ, RENJU_SEQ[:10], [40], []], [3, 2, 1, 0], gomoku_renju=True)
    m = handle(engine, 1, gomoku_renju=True)
    try:
        m.new_games_moves([RENJU_SEQ])
        m.search()
        assert 40 not in m.rootChildren(0)[0].tolist()         # the overline cell is no child
        before = snapshot(m)
        with pytest.raises(az_amd.AzError, match=r"entry 0 .*ply 12.*forbidden") as e:
            m.new_games_moves([RENJU_SEQ + [40]])
        assert e.value.code == _lib.AZ_ERR_ARG
        assert snapshot(m) == before
    finally:
        m.close()


# One judge behind both entry points: (rules, the plies before, the refused move, the word of its reason)
VERDICTS = {
    # White at 0 between Black 1 and 9, each with two liberties left: nothing is captured
    "go-suicide": ("go", [1, 40, 9], 0, "suicide"),
    "go-occupied": ("go", [1, 40, 9], 40, "occupied"),
    "go-superko": ("go", KO_LIST, 1, "superko"),
    "renju-forbidden": ("renju", RENJU_SEQ, 40, "forbidden"),
    # Black's own stone: GomokuState::make_move throws "already occupied" whatever the rules
    "renju-occupied": ("renju", RENJU_SEQ, 37, "occupied"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(VERDICTS))
def test_gpu_openings_both_entry_points_give_the_same_verdict(engine, case):
    """The same position reached by an opening and move by move: the move the rules refuse is refused as the next
    ply of the sequence and by az_search_apply, for the same reason, and both handles stay as they were."""
    import az_amd
    from az_amd import _lib
    rules, prefix, bad, why = VERDICTS[case]
    kw = dict(game=az_amd.AZ_GAME_GO, go_superko=True) if rules == "go" else dict(gomoku_renju=True)
    a, b = handle(engine, 1, **kw), handle(engine, 1, **kw)
    try:
        a.new_games_moves([prefix])
        compose(b, [prefix], None)
        before_a, before_b = snapshot(a), snapshot(b)
        with pytest.raises(az_amd.AzError, match=rf"entry 0 .*ply {len(prefix)},.*{why}") as e:
            a.new_games_moves([prefix + [bad]])
        assert e.value.code == _lib.AZ_ERR_ARG
        with pytest.raises(az_amd.AzError, match=why) as e:
            b.updateWithMove(np.array([bad], np.int32))
        assert e.value.code == _lib.AZ_ERR_ARG
        assert snapshot(a) == before_a and snapshot(b) == before_b
        play_both(a, b, rounds=1)                              # equal and playable after the refusals
    finally:
        a.close()
        b.close()


def raw_call(m, games, seqs, stride, n_moves=None):
    from az_amd import _lib
    games = np.asarray(games, np.int32)
    mv = np.full((len(seqs), max(stride, 1)), -7, np.int32)
    for i, q in enumerate(seqs):
        mv[i, :min(len(q), stride)] = q[:stride]
    nm = np.asarray([len(q) for q in seqs] if n_moves is None else n_moves, np.int32)
    rc = _lib.lib().az_search_new_games_moves(m.h, games.ctypes.data, None, games.size, mv.ctypes.data, nm.ctypes.data, stride)
    return rc, _lib.lib().az_last_error().decode()


@pytest.mark.gpu
def test_gpu_openings_refusals_leave_the_handle_as_it_was(engine):
    import az_amd
    from az_amd import _lib
    m = handle(engine, 3)
    g = handle(engine, 2, game=az_amd.AZ_GAME_GO, go_superko=True)
    try:
        for h in (m, g):
            h.newGames()
            h.search()
            h.updateWithMove(h.select(True, 1.0)[0])
            h.search()
        before = snapshot(m)
        ok = [40, 41]
        cases = [("occupied", [ok, [40, 40], ok], 1, 1, "occupied"),
                 ("range", [ok, ok, [81]], 2, 0, "out of range"),
                 ("negative", [[-1], ok, ok], 0, 0, "out of range"),
                 ("after five", [ok, FIVE + [13], ok], 1, 9, "ended")]
        for name, seqs, entry, ply, why in cases:
            rc, msg = raw_call(m, [0, 1, 2], seqs, 10)
            assert rc == _lib.AZ_ERR_ARG, name
            assert f"entry {entry} " in msg and f"ply {ply}," in msg and why in msg, (name, msg)
            assert snapshot(m) == before, name
        rc, msg = raw_call(m, [0, 1, 2], [ok, ok, ok], 1, n_moves=[1, 2, 1])
        assert rc == _lib.AZ_ERR_ARG and "entry 1 " in msg and "stride" in msg, msg
        rc, msg = raw_call(m, [0, 1, 2], [ok, ok, ok], 2, n_moves=[1, -1, 1])
        assert rc == _lib.AZ_ERR_ARG and "entry 1 " in msg, msg
        rc, msg = raw_call(m, [0, 3, 2], [ok, ok, ok], 2)
        assert rc == _lib.AZ_ERR_ARG and "entry 1" in msg and "out of range" in msg, msg
        assert snapshot(m) == before
        m.search()                                              # ... and it plays on
        # Go: a positional superko repeat that the ko point does not cover
        gb = snapshot(g)
        rc, msg = raw_call(g, [1, 0], [[40], KO_LIST + [1]], 12)
        assert rc == _lib.AZ_ERR_ARG and "entry 1 " in msg and f"ply {len(KO_LIST)}," in msg and "superko" in msg, msg
        rc, msg = raw_call(g, [0], [[40, 40]], 2)
        assert rc == _lib.AZ_ERR_ARG and "ply 1," in msg and "occupied" in msg, msg
        assert snapshot(g) == gb
        # the last move of a sequence may end the game: the slot is inactive with that winner
        m.new_games_moves([FIVE, ok], games=[1, 2])
        term, res = m.updateWithMove(np.full(3, -1, np.int32))
        assert term.tolist() == [0, 1, 0] and res.tolist() == [0, 2, 0]
        assert snapshot(m)[0] != before[0]                      # slot 0 was not listed: it kept the game it searched
        m.search()
        assert m.select(True, 1.0)[0][1] == -1 and m.rootChildren(1)[0].size == 0
    finally:
        m.close()
        g.close()


@pytest.mark.gpu
def test_gpu_openings_simple_ko_allows_the_superko_repeat(engine):
    """The move the superko handle refuses is legal under simple ko, and equivalent there."""
    import az_amd
    equivalent(engine, [KO_LIST + [1], KO_LIST], None, game=az_amd.AZ_GAME_GO, go_superko=False)


# ---------------------------------------------------------------------------- the drivers
BOOK = [[40, 41], [30, 31, 32], [50, 49, 48, 47]]
DROP = 3                                    # temperature 1 below ply 3, 0 from it on
MAXM = 9


def selfplay(engine, slots, book, random_plies=0, seed=0, total=7, max_moves=MAXM, replay=None, sims=SIMS, **kw):
    import az_amd
    sp = az_amd.SelfPlayManager(engine, numGames=slots, numSimulations=sims, board_size=9, evaluator=az_amd.AZ_EVAL_HASH,
                                tt_log2=8, noise_seed=42, noise_seed_stride=1, **kw)
    try:
        sp.setExplorationParams(0.03, 0.25, 1.0, DROP, 0.0)
        if book is not None or random_plies:
            sp.setOpenings(book, random_plies, seed)
            assert sp.mcts.openings() == (len(book or []), random_plies, seed)
        if replay is not None:
            sp.mcts.attachReplay(replay)
        return sp.generateGames(total, max_moves=max_moves)
    finally:
        sp.mcts.close()


def flat(recs):
    return [(r.game_id, r.result, [(m.action, np.asarray(m.policy, np.float32).view(np.uint32).tolist(),
                                    np.float32(m.value).view(np.uint32).item(), list(m.child_actions)) for m in r.moves])
            for r in recs]


def n_opening(rec):
    """The plies at the head of a record that no search stands behind."""
    n = 0
    while n < len(rec.moves) and not rec.moves[n].policy:
        n += 1
    return n


def hand_game(engine, opening, gid, sims, temps):
    """One game of az_selfplay_run played through the per-call ABI from new_games_moves: the start noise, then per ply
    search, select at temps(ply), apply, noise after every even ply -- its searched moves as flat() lists them."""
    import az_amd
    m = az_amd.ParallelMCTS(engine, n_games=1, board_size=9, num_simulations=sims, evaluator=az_amd.AZ_EVAL_HASH, tt_log2=8,
                            noise_seed=42, noise_seed_stride=1)
    try:
        m.new_games_moves([opening], ids=[gid])
        m.addDirichletNoise(0.03, 0.25, mask=[1])
        hand = []
        for ply in range(len(opening), MAXM):
            m.search()
            act, val, probs, cact, nch = m.select(True, temps(ply))
            hand.append((int(act[0]), probs[0, :nch[0]].view(np.uint32).tolist(), val[:1].view(np.uint32).item(),
                         cact[0, :nch[0]].tolist()))
            m.updateWithMove(act)
            if ply % 2 == 0:
                m.addDirichletNoise(0.03, 0.25, mask=[1])
        return hand
    finally:
        m.close()


@pytest.mark.gpu
def test_gpu_openings_book_in_selfplay_run(engine):
    """7 games over a book of 3 openings: the records do not depend on the number of slots, game i begins with
    opening i % 3 (plies without children), and games 0 and 1 equal the same games played by hand from
    new_games_moves under the driver's rules -- with the temperature of the REAL ply: game 1's first searched move
    is ply 3, where the schedule has dropped to 0, and a schedule that counted searched moves would record another
    policy there (128 simulations, so that the visit counts differ and the temperature shows)."""
    sims = 128
    recs = selfplay(engine, 3, BOOK, sims=sims)
    assert flat(recs) == flat(selfplay(engine, 2, BOOK, sims=sims))
    for i, r in enumerate(recs):
        op = BOOK[i % 3]
        assert [m.action for m in r.moves[:len(op)]] == op and n_opening(r) == len(op), i
        assert all(m.value == 0.0 and m.thinking_time_ms == 0 and not m.child_actions for m in r.moves[:len(op)])
        assert len(r.moves) == MAXM, i                            # max_moves counts real plies (Black's fifth stone is ply 9)
        assert len(r.moves[len(op)].child_actions) == 81 - len(op)
    real = lambda ply: 1.0 if ply < DROP else 0.0                 # noqa: E731
    for gid in (0, 1):
        op = BOOK[gid]
        assert flat(recs)[gid][2][len(op):] == hand_game(engine, op, gid, sims, real), gid
    counted_from_the_opening = lambda ply: 1.0 if ply - len(BOOK[1]) < DROP else 0.0        # noqa: E731
    wrong = hand_game(engine, BOOK[1], 1, sims, counted_from_the_opening)
    assert wrong[0][1] != flat(recs)[1][2][len(BOOK[1])][1]      # the first searched move's policy tells the two apart


@pytest.mark.gpu
@pytest.mark.parametrize("game", ["renju", "go"])
@pytest.mark.parametrize("book", [None, [[40, 41], [30]]], ids=["no-book", "book"])
def test_gpu_openings_random_plies(engine, game, book):
    """Six random plies after the book's: the records' opening plies are the host restatement's (numpy Philox, the
    host state's legal moves), the records do not depend on the number of slots, another seed gives other openings."""
    import az_amd
    from test_openings_cpu import host_opening
    H = pytest.importorskip("_alphazero_cpp")
    kw = dict(game=az_amd.AZ_GAME_GO) if game == "go" else dict(gomoku_renju=True)
    seed, r, total = 0x1234567887654321, 6, 5
    recs = selfplay(engine, 3, book, r, seed, total=total, max_moves=10, **kw)
    assert flat(recs) == flat(selfplay(engine, 2, book, r, seed, total=total, max_moves=10, **kw))
    for i, rec in enumerate(recs):
        state = H.GoState(9) if game == "go" else H.GomokuState.withRules(9, True, False)
        want = host_opening(state, book[i % len(book)] if book else [], r, seed, i)
        assert [m.action for m in rec.moves[:n_opening(rec)]] == want, i
        assert len(want) == (len(book[i % len(book)]) if book else 0) + r        # nothing ends a 9x9 game this early
    other = selfplay(engine, 3, book, r, seed + 1, total=total, max_moves=10, **kw)
    assert [[m.action for m in x.moves[:n_opening(x)]] for x in other] != \
           [[m.action for m in x.moves[:n_opening(x)]] for x in recs]


@pytest.mark.gpu
def test_gpu_openings_replay_rows(engine):
    """With a replay buffer attached nothing is staged for an opening ply: a game's rows number its searched moves,
    the smallest ply is the opening's length, and that row's planes are the host state's after the opening."""
    import az_amd
    H = pytest.importorskip("_alphazero_cpp")
    rb = az_amd.ReplayBuffer(engine, az_amd.GAME_GOMOKU, 9, capacity=256)
    try:
        recs = selfplay(engine, 3, BOOK, total=5, replay=rb)
        info = rb.info()
        assert info["committed"] == sum(len(r.moves) - n_opening(r) for r in recs) and info["dropped"] == 0
        rows = rb.gather(np.arange(info["committed"]))
        for i, r in enumerate(recs):
            mine = np.flatnonzero(rows["game_id"] == i)
            op = BOOK[i % 3]
            assert mine.size == len(r.moves) - len(op), i
            assert sorted(rows["ply"][mine].tolist()) == list(range(len(op), len(r.moves))), i
            s = H.GomokuState(9)
            for a in op:
                s.makeMove(a)
            first = mine[np.argmin(rows["ply"][mine])]
            want = np.asarray(s.getEnhancedTensorRepresentation(), np.float32).reshape(11, 9, 9)
            assert np.array_equal(rows["states"][first], want), i
    finally:
        rb.close()


@pytest.mark.gpu
def test_gpu_openings_dataset_keeps_opening_plies_as_empty_targets(engine):
    """What az_dataset_extract makes of a move without children, as the opening plies of a record are: the move is
    replayed on the board and yields its examples like any other -- the planes of the position before it, the
    game's value -- with policy length 0 and an all-zero policy row.  (A trainer that wants searched positions
    only drops the examples whose policy length is 0; the replay buffer never holds them.)"""
    import az_amd
    recs = selfplay(engine, 2, BOOK, total=2, max_moves=6)
    ds = az_amd.Dataset(engine, az_amd.GAME_GOMOKU, 9)
    full = az_amd.Dataset(engine, az_amd.GAME_GOMOKU, 9)
    try:
        for r in recs:
            ds.addGameRecord(r)
            # the same games with a made-up uniform policy on the opening plies
            g = az_amd.GameRecord(r.board_size, [az_amd.MoveData(m.action, m.policy or [0.5, 0.5], m.value) for m in r.moves],
                                  r.result, r.game_id)
            full.addGameRecord(g)
        n = ds.extractExamples(includeAugmentations=True, shuffle=False)
        assert n == full.extractExamples(includeAugmentations=True, shuffle=False) == 8 * sum(len(r.moves) for r in recs)
        st, po, pl, va = ds.gather(np.arange(n))
        fst, fpo, fpl, fva = full.gather(np.arange(n))
        assert np.array_equal(st, fst) and np.array_equal(va, fva)
        e = 0
        for i, r in enumerate(recs):
            for ply, m in enumerate(r.moves):
                opening = ply < len(BOOK[i % 3])
                for s in range(8):
                    assert pl[e] == (0 if opening else len(m.policy)), (i, ply, s)
                    if opening:
                        assert not po[e].any() and fpl[e] == 2
                    else:
                        assert np.array_equal(po[e], fpo[e])
                    e += 1
    finally:
        ds.close()
        full.close()


@pytest.mark.gpu
def test_gpu_openings_arena(engine):
    """swap_colors with a 2-opening book: ids 0 and 1 share opening 0, ids 2 and 3 opening 1, the colours alternate,
    the opening plies' movers follow the colour, the summary counts 4 games and the searched moves only."""
    import az_amd
    from test_gpu_arena import make_net
    nets = [make_net(engine, False, 9, 32, 2, az_amd.AZ_PREC_F32, 2, 9 + p) for p in (0, 1)]
    book = [[40, 41, 31], [20, 60]]
    ar = az_amd.Arena(engine, nets[0], nets[1], 2, board_size=9, num_simulations=SIMS, swap_colors=True, tt_log2=8)
    try:
        ar.setOpenings(book, random_plies=2, seed=7)
        recs = ar.run(4, max_moves=8)
        summ = ar.summary()
    finally:
        ar.close()
        for n in nets:
            n.close()
    assert summ["games"] == 4
    heads = []
    for gid, r in enumerate(recs):
        op = book[(gid // 2) % 2]
        n = n_opening(r)
        assert n == len(op) + 2 and [m.action for m in r.moves[:len(op)]] == op, gid
        assert r.a_is_player1 == (gid % 2 == 0)
        # Black (even plies) is the starter: net A in the even games, net B in the odd ones
        assert r.movers[:n] == [(ply % 2) ^ (0 if r.a_is_player1 else 1) for ply in range(n)], gid
        assert r.movers[n] == (n % 2) ^ (0 if r.a_is_player1 else 1)
        heads.append([m.action for m in r.moves[:n]])
    assert heads[0] == heads[1] and heads[2] == heads[3] and heads[0] != heads[2]       # the pair shares its random plies
    assert summ["moves"] == sum(len(r.moves) - n_opening(r) for r in recs)
