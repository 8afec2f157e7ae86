"""CPU checks of tests/replay_util.py: the slot schedule of az_selfplay_run on hand-worked examples."""
import pytest

from replay_util import slot_schedule


def test_slot_schedule_hand_worked():
    # 3 slots, 4 games of 1, 4, 2 and 1 moves:
    #   step 0: slots play games 0, 1, 2; game 0 ends, slot 0 takes id 3
    #   step 1: games 3, 1, 2; games 3 and 2 end, no id is left: slots 0 and 2 go idle
    #   steps 2, 3: only slot 1 moves, game 1 ends after its 4th move
    games, steps = slot_schedule(3, [1, 4, 2, 1])
    assert games == [[0, 3], [1], [2]]
    assert steps == [(0, 1, 2), (3, 1, 2), (None, 1, None), (None, 1, None)]


def test_slot_schedule_same_step_restarts_take_ids_in_slot_order():
    # games 0 and 2 both end in step 0: slot 0 takes id 3, slot 2 id 4; game 4 ends in step 1 and
    # slot 2 takes id 5 while slots 0 and 1 still play
    games, steps = slot_schedule(3, [1, 3, 1, 3, 1, 2])
    assert games == [[0, 3], [1], [2, 4, 5]]
    assert steps == [(0, 1, 2), (3, 1, 4), (3, 1, 5), (3, None, 5)]
    # every game is played exactly once, every move of it in consecutive steps of one slot
    for g, n in enumerate([1, 3, 1, 3, 1, 2]):
        assert sum(row.count(g) for row in steps) == n


def test_slot_schedule_more_slots_than_games():
    games, steps = slot_schedule(4, [2, 1])
    assert games == [[0], [1], [], []]
    assert steps == [(0, 1, None, None), (0, None, None, None)]


def test_slot_schedule_rejects_empty_games():
    with pytest.raises(AssertionError):
        slot_schedule(2, [3, 0])


def _logged_games(bs, sims, games):
    """Play `games` [(id, n_moves)] on the oracle with a network-style evaluator (zero logits and a
    position-dependent value: the oracle's softmax gives exactly 1 / A) and log what a device would."""
    import numpy as np
    import az_oracle as O
    A = bs * bs
    log = []

    def net(game, x):
        v = np.float32(np.tanh(0.1 * float(x[0].sum() - x[1].sum()) + 0.01 * float((x[0] * np.arange(A).reshape(bs, bs)).sum() % 7)))
        log.append((np.full(A, np.float32(1.0) / np.float32(A), np.float32), v, x.copy()))
        return np.zeros(A, np.float32), float(v)

    refs = [O.play(bs=bs, sims=sims, max_moves=n, eval_kind=O.EVAL_NET, evaluator=net, noise_seed=42 + g)[0]
            for g, n in games]
    pol, val, planes = (np.array([e[i] for e in log], np.float32) for i in range(3))
    return refs, pol, val, planes


def test_replay_eval_log_replays_a_sequence_of_games():
    from replay_util import replay_eval_log
    games = [(0, 3), (5, 2), (6, 0)]        # the last one cut before its first move: its first root only
    refs, pol, val, planes = _logged_games(5, 24, games)
    again = replay_eval_log(pol, val, planes, games, bs=5, sims=24)
    assert [r["moves"] for r in again] == [r["moves"] for r in refs]
    assert [len(r["moves"]) for r in again] == [3, 2, 0]


def test_replay_eval_log_fails_on_wrong_planes_order_or_count():
    import numpy as np
    from replay_util import replay_eval_log
    games = [(1, 2), (4, 1)]
    refs, pol, val, planes = _logged_games(5, 16, games)
    bad = planes.copy()
    bad[len(bad) // 2, 0, 0, 0] += 1.0
    with pytest.raises(AssertionError, match="feature planes differ"):
        replay_eval_log(pol, val, bad, games, bs=5, sims=16)
    with pytest.raises(AssertionError, match="feature planes differ"):        # another game's noise stream
        replay_eval_log(pol, val, planes, [(1, 2), (3, 1)][::-1], bs=5, sims=16)
    with pytest.raises(AssertionError, match="the log holds"):
        replay_eval_log(pol[:-1], val[:-1], planes[:-1], games, bs=5, sims=16)
    with pytest.raises(AssertionError, match="logged evaluations"):
        replay_eval_log(np.concatenate([pol, pol[-1:]]), np.concatenate([val, val[-1:]]),
                        np.concatenate([planes, planes[-1:]]), games, bs=5, sims=16)
