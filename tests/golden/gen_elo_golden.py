"""Generates tests/golden/elo_sequences.json from the REFERENCE EloRating (python/alphazero/utils/elo.py,
loaded as it stands; its plotting imports are stubbed when matplotlib is missing -- add_game_result does
not touch them).

Per sequence: the scores of player A in game order (1 / 0.5 / 0) and the two ratings after every game,
from EloRating(1500, 32).add_game_result("a", "b", score), as python/scripts/evaluate.py:333,:412-416
calls it.  Ratings are stored through float.hex, so the fixture holds the doubles exactly.

Run where the reference is checked out:  python tests/golden/gen_elo_golden.py <reference root>
"""
import importlib.util
import json
import os
import random
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))


def load_elo(ref):
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    spec = importlib.util.spec_from_file_location("ref_elo", os.path.join(ref, "python", "alphazero", "utils", "elo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    elo = load_elo(ref)
    rng = random.Random(20240607)
    seqs = {
        "a_wins_64": [1.0] * 64,
        "b_wins_64": [0.0] * 64,
        "draws_16": [0.5] * 16,
        "alternate_40": [1.0, 0.0] * 20,
        "single_draw": [0.5],
        "mixed_64": [rng.choice([1.0, 0.5, 0.0]) for _ in range(64)],
        "mostly_a_48": [rng.choice([1.0, 1.0, 1.0, 0.5, 0.0]) for _ in range(48)],
    }
    out = {}
    for name, scores in seqs.items():
        tr = elo.EloRating(initial_rating=1500.0, k_factor=32.0)
        ra, rb = [], []
        for s in scores:
            tr.add_game_result("a", "b", s)
            ra.append(float(tr.get_rating("a")).hex())
            rb.append(float(tr.get_rating("b")).hex())
        out[name] = {"scores": scores, "rating_a": ra, "rating_b": rb}
    with open(os.path.join(HERE, "elo_sequences.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", len(out), "sequences")


if __name__ == "__main__":
    main()
