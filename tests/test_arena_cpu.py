"""CPU parts of the evaluation match: the Elo arithmetic (alphazero::evaluation::EloRating and az_amd.EloRating,
both over az_elo_update) against ratings recorded from the reference's python/alphazero/utils/elo.py
(tests/golden/elo_sequences.json, written by tests/golden/gen_elo_golden.py), and the evaluate binary's
argument checks, which run before anything touches a GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "alphazero-multi-game_amd", "build", "evaluate")
GOLDEN = os.path.join(ROOT, "tests", "golden", "elo_sequences.json")
# one ulp at 1500 is 2.3e-13 and a sequence has at most 64 updates: the slack covers another libm pow only
TOL = 1e-9


@pytest.fixture(scope="module")
def sequences():
    with open(GOLDEN) as f:
        seqs = json.load(f)
    assert len(seqs) >= 5 and max(len(s["scores"]) for s in seqs.values()) == 64
    return seqs


def trackers():
    import _alphazero_cpp as A
    import az_amd
    return {"cpp": lambda: A.EloRating(1500.0, 32.0), "az_amd": lambda: az_amd.EloRating(1500.0, 32.0)}


@pytest.mark.parametrize("impl", ["cpp", "az_amd"])
def test_elo_matches_reference_sequences(sequences, impl):
    worst = 0.0
    for name, s in sequences.items():
        tr = trackers()[impl]()
        assert tr.getRating("a") == 1500.0 and tr.getRating("nobody") == 1500.0
        for i, score in enumerate(s["scores"]):
            new_a = tr.addGameResult("a", "b", score)
            ra, rb = float.fromhex(s["rating_a"][i]), float.fromhex(s["rating_b"][i])
            ea, eb = abs(tr.getRating("a") - ra), abs(tr.getRating("b") - rb)
            worst = max(worst, ea, eb)
            assert new_a == tr.getRating("a")
            assert ea <= TOL and eb <= TOL, (name, i, ea, eb)
    print(f"EloRating [{impl}]: max |rating - reference| = {worst:.3e}")


def test_elo_expected_score_and_symmetry():
    import _alphazero_cpp as A
    assert A.EloRating.expectedScore(1500.0, 1500.0) == 0.5
    assert abs(A.EloRating.expectedScore(1900.0, 1500.0) - 10.0 / 11.0) <= 1e-15
    tr = A.EloRating()
    tr.addGameResult("x", "y", 1.0)
    assert (tr.getRating("x"), tr.getRating("y")) == (1516.0, 1484.0)


def run_bin(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=60)


def test_evaluate_help_lists_the_reference_flags():
    r = run_bin("--help")
    assert r.returncode == 0
    for flag in ("--model-a", "--model-b", "--game", "--size", "--games", "--simulations", "--threads", "--output-dir",
                 "--temperature", "--swap", "--seed", "--tables", "--precision"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args,word", [
    (("--model-a", "a.azw", "--model-b", "b.azw", "--variant"), "--variant"),
    (("--model-a", "a.azw", "--model-b", "b.azw", "--game", "chess"), "chess"),
    (("--model-a", "a.azw", "--model-b", "b.azw", "--time-control", "1"), "--time-control"),
])
def test_evaluate_refuses_what_the_arena_does_not_play(args, word, tmp_path):
    r = subprocess.run([BIN, *args, "--output-dir", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert r.stderr.startswith("evaluate: ") and word in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()
