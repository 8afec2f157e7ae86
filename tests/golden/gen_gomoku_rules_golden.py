#!/usr/bin/env python3
"""Regenerates the Gomoku rule-variant fixtures (Renju, Omok) from the patched REFERENCE build:

    python3 tests/golden/gen_gomoku_rules_golden.py [REFERENCE_ROOT]

Repeats oracle/build_ref.sh's recipe (patches P1, P2, P5; no arithmetic change) in a temp directory,
adds P11, links tests/golden/gomoku_rules_harness.cpp against it there, and writes only the harness'
JSON output: ref_gomoku_rules_games.json.gz and ref_gomoku_rules_positions.json.gz.  The binary and
the temp copy are deleted; nothing of the reference enters the repository.

P11: GomokuRules installs a temporary board accessor (the board plus the candidate stone) by
assigning a lambda to its own is_bit_set member -- a lambda that calls that member, i.e. itself,
without end.  The accessor saved just before the assignment is the one it means to call; P11 makes
the installed lambda capture and call that saved accessor, in the four functions that do this.

The generator asserts the conditions the fixtures exist for (see check()).
"""
import concurrent.futures
import glob
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

OUT = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF", "/root/reference")

PUCT, PBIAS = 1, 2
# (bs, sims, max_moves, evaluator, eval_seed, noise_each_search, cpuct, fpu) as gen_golden.py's cases, then
# (renju, omok), the noise seed, log2 of the table size and (selection, max_search_depth, use_td, td_lambda)
DEFAULT_OPTS = (PUCT, 1000, 0, 0.8)
GAME_CASES = [
    ((9, 100, 80, "hash", 3, 0, 1.5, 0.0), (1, 0), 42, 20, DEFAULT_OPTS),
    ((9, 100, 80, "hash", 3, 0, 1.5, 0.0), (0, 1), 42, 20, DEFAULT_OPTS),
    ((9, 100, 80, "hash", 3, 0, 1.5, 0.0), (1, 1), 42, 20, DEFAULT_OPTS),
    ((7, 60, 49, "hash", 5, 0, 1.5, 0.0), (1, 0), 42, 20, DEFAULT_OPTS),
    ((7, 60, 49, "hash", 5, 0, 1.5, 0.0), (0, 1), 42, 20, DEFAULT_OPTS),
    ((15, 200, 10, "hash", 7, 0, 1.5, 0.0), (1, 0), 42, 20, DEFAULT_OPTS),
    ((9, 100, 52, "hash", 11, 0, 1.5, 0.0), (0, 1), 42, 6, DEFAULT_OPTS),       # 64-entry table: slot collisions
    ((9, 60, 50, "hash", 5, 1, 1.5, 0.25), (1, 0), 42, 20, DEFAULT_OPTS),       # per-search noise + FPU
    ((9, 100, 40, "hash", 9, 0, 1.5, 0.0), (1, 0), 42, 20, (PBIAS, 1000, 1, 0.6)),   # PROGRESSIVE_BIAS + TD under Renju
    # one case played with three noise seeds: the games of a three-game handle with stride 1
    ((9, 100, 30, "hash", 5, 0, 1.5, 0.0), (1, 0), 42, 20, DEFAULT_OPTS),
    ((9, 100, 30, "hash", 5, 0, 1.5, 0.0), (1, 0), 43, 20, DEFAULT_OPTS),
    ((9, 100, 30, "hash", 5, 0, 1.5, 0.0), (1, 0), 44, 20, DEFAULT_OPTS),
]
RULE_SETS = ((1, 0), (0, 1), (1, 1))
# (bs, count, margin): random legal play; a margin keeps the stones in the centre so that lines meet
POSITION_RUNS = ((7, 20, 0), (7, 12, 1), (9, 20, 0), (9, 12, 2), (15, 6, 0), (15, 8, 4))


def cells(bs, *xy):
    return [x * bs + y for x, y in xy]


def interleave(black, white):
    assert len(white) == len(black), "Black is to move in every constructed position"
    return [a for pair in zip(black, white) for a in pair]


def constructed():
    """name -> (bs, (renju, omok), moves, cell, verdict list, expected membership).  White's stones sit apart on the
    last rows unless they are part of the shape."""
    bs = 15
    far = cells(bs, (14, 0), (14, 2), (14, 4), (14, 6), (14, 8), (14, 10), (14, 12), (12, 0), (12, 2))
    row5 = cells(bs, (7, 2), (7, 3), (7, 4), (7, 6), (7, 7))           # BBB.BB: (7, 5) makes six
    cross = cells(bs, (7, 6), (7, 8), (6, 7), (8, 7))                   # (7, 7) makes a three each way
    out = {
        "overline": (bs, (1, 0), interleave(row5, far[:5]), 7 * bs + 5, "renju_overline", True),
        "overline-omok": (bs, (0, 1), interleave(row5, far[:5]), 7 * bs + 5, "omok_overline", True),
        "two-fours": (bs, (1, 0), interleave(cells(bs, (7, 4), (7, 5), (7, 6), (4, 7), (5, 7), (6, 7)), far[:6]),
                      7 * bs + 7, "renju_double_four", True),
        # the board holds the first shape {2,3,4,6} and {3,4,6,7}, which shares three of its stones: one four, so a
        # cell elsewhere is allowed although two distinct shapes stand on the board
        "unified-fours-elsewhere": (bs, (1, 0), interleave(row5, far[:5]), 12 * bs + 12, "renju_double_four", False),
        "two-connected-threes": (bs, (0, 1), interleave(cross, far[:4]), 7 * bs + 7, "omok_double_three", True),
        "two-unconnected-threes": (bs, (0, 1), interleave(cells(bs, (2, 2), (2, 3), (2, 4), (10, 9), (10, 11)), far[:5]),
                                   10 * bs + 10, "omok_double_three", False),
        # .B.B. in the row ((7, 5) and the cell) is no three: the slice holds two stones, not three
        "gap-triple": (bs, (0, 1), interleave(cells(bs, (7, 5), (6, 7), (8, 7)), far[:3]), 7 * bs + 7, "omok_double_three",
                       False),
        # a white stone just beyond the row's slice (7, 5)..(7, 9) does not close the three
        "white-beyond-end": (bs, (0, 1), interleave(cross, cells(bs, (7, 4)) + far[:3]), 7 * bs + 7, "omok_double_three",
                             True),
    }
    return out


def build(tmp):
    """oracle/build_ref.sh's recipe: copy the hot-path translation units, patch, compile, link."""
    for d in ("src/mcts", "src/nn", "src/games/gomoku", "src/games/go", "src/core"):
        os.makedirs(os.path.join(tmp, d))
    shutil.copytree(os.path.join(REF, "include"), os.path.join(tmp, "include"))
    for d, names in (("src/mcts", ("parallel_mcts", "mcts_node", "transposition_table", "thread_pool")),
                     ("src/nn", ("batch_queue", "random_policy_network")),
                     ("src/games/gomoku", ("gomoku_state", "gomoku_rules")),
                     ("src/games/go", ("go_state", "go_rules")), ("src/core", ("zobrist_hash",))):
        for n in names:
            shutil.copy(os.path.join(REF, d, n + ".cpp"), os.path.join(tmp, d, n + ".cpp"))
    subprocess.run(["chmod", "-R", "u+w", tmp], check=True)

    def patch(rel, old, new, count=1, regex=False):
        p = os.path.join(tmp, rel)
        s = open(p).read()
        s, n = (re.subn(old, new, s) if regex else (s.replace(old, new), s.count(old)))
        assert n == count, (rel, old, n)
        open(p, "w").write(s)

    patch("src/mcts/parallel_mcts.cpp", "[this, i, &completedSimulations]", "[this, i, numThreads, &completedSimulations]")  # P1
    patch("src/games/gomoku/gomoku_state.cpp", "zobrist_(core::GameType::GOMOKU, board_size, 2)", "zobrist_(board_size, 2, 2, 12345u)")  # P2
    patch("src/games/go/go_state.cpp", "zobrist_(core::GameType::GO, board_size, 2)", "zobrist_(board_size, 2, 2, 12345u)")  # P6 (links only)
    patch("include/alphazero/mcts/mcts_node.h", "std::mutex expansionMutex;", "std::recursive_mutex expansionMutex;")  # P5
    patch("src/mcts/parallel_mcts.cpp", r"std::lock_guard<std::mutex> lock\((rootNode_|node)->expansionMutex\)",
          r"std::lock_guard<std::recursive_mutex> lock(\1->expansionMutex)", count=6, regex=True)
    # P11: four asserted replacements, one per function -- the installed accessor calls the saved one
    rules = os.path.join(tmp, "src/games/gomoku/gomoku_rules.cpp")
    s = open(rules).read()
    install = "const_cast<GomokuRules*>(this)->is_bit_set = is_bit_set_temp;"
    fixed = ("const_cast<GomokuRules*>(this)->is_bit_set = [original_is_bit_set, %s](int p_idx, int a) "
             "{ return (a == %s && p_idx == 0) || original_is_bit_set(p_idx, a); };")
    starts = [s.index("GomokuRules::" + f + "(") for f in ("renju_double_four_or_more", "omok_check_double_three_strict",
                                                          "is_allowed_double_three", "is_double_three_allowed_recursive")]
    assert starts == sorted(starts) and s.count(install) == 4
    for at, stone in reversed(list(zip(starts, ("action", "action", "action", "placement")))):
        i = s.index(install, at)
        saved = s.index("auto original_is_bit_set = is_bit_set;", at)
        assert saved < i and s.index("\n}\n", at) > i, "the install follows the save inside this function"
        s = s[:i] + fixed % (stone, stone) + s[i + len(install):]
    assert s.count(install) == 0
    open(rules, "w").write(s)
    flags = ["-std=c++17", "-O2", "-pthread", "-DLIBTORCH_OFF", "-I" + os.path.join(tmp, "include")]
    procs, objs = [], []
    for f in glob.glob(os.path.join(tmp, "src", "*", "*.cpp")) + glob.glob(os.path.join(tmp, "src", "games", "*", "*.cpp")):
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        objs.append(o)
        procs.append(subprocess.Popen(["g++"] + flags + ["-w", "-c", f, "-o", o]))
    h = os.path.join(tmp, "gomoku_rules_harness.o")
    procs.append(subprocess.Popen(["g++"] + flags + ["-c", os.path.join(OUT, "gomoku_rules_harness.cpp"), "-o", h]))
    for p in procs:
        assert p.wait() == 0
    exe = os.path.join(tmp, "gomoku_rules_harness")
    subprocess.run(["g++", "-pthread", h] + objs + ["-o", exe], check=True)
    return exe


VERDICTS = ("renju_overline", "renju_double_four", "renju_double_three_refused", "omok_overline", "omok_double_three")


def all_positions(pos):
    return [p for k in sorted(pos) for p in pos[k]]


def check(games, pos):
    """What the fixtures exist for; tests/test_gomoku_rules_host.py repeats it on the committed files."""
    for rules in ((1, 0), (0, 1)):
        assert any(g["rules"] == list(rules) and any(m["ply"] % 2 == 0 and len(m["children"]) < g["case"][0] ** 2 - m["ply"]
                                                      for m in g["moves"]) for g in games), ("no forbidden root", rules)
    assert any(g["terminal"] and g["result"] != 0 for g in games)
    assert any(g["tt_log2"] == 6 for g in games) and any(g["case"][0] == 15 for g in games)
    assert any(g["opts"] != list(DEFAULT_OPTS) for g in games)
    for p in all_positions(pos):
        assert p["renju_double_three_refused"] == [], "is_allowed_double_three is true for every empty cell"
        assert p["renju_overline"] == p["omok_overline"]
    st = pos["stalemate"]
    assert st
    for p in st:
        assert p["terminal"] and p["result"] == 1 and len(p["moves"]) < p["bs"] ** 2 and p["player"] == 1 and p["legal"] == []
    built = constructed()
    assert len(pos["constructed"]) == len(built)
    for p, (name, (bs, rules, moves, cell, verdict, want)) in zip(pos["constructed"], sorted(built.items())):
        assert p["name"] == name and p["moves"] == moves and p["player"] == 1 and not p["terminal"]
        assert (cell in p[verdict]) == want, (name, verdict, p[verdict])
        forbidden = cell in (p["renju_overline"] + p["renju_double_four"] if rules[0] else p["omok_overline"] + p["omok_double_three"])
        assert forbidden == want and (cell in p["legal"]) == (not want), name
    # the rules bite in random play too, under every rule set, and both on a board with and without standing shapes
    for rules in RULE_SETS:
        assert any(p["renju"] == rules[0] and p["omok"] == rules[1] and p["player"] == 1 and not p["terminal"] and
                   len(p["legal"]) < p["bs"] ** 2 - len(p["moves"]) for p in all_positions(pos)), rules


def main():
    tmp = tempfile.mkdtemp(prefix="az_gomokurules.")
    try:
        exe = build(tmp)

        def run(*args):
            r = subprocess.run([exe] + [str(x) for x in args], capture_output=True, text=True, timeout=3000)
            if r.returncode != 0:
                sys.exit(f"harness failed: {args}: {r.stderr}")
            return json.loads(r.stdout)

        def game(spec):
            case, rules, nseed, ttl, opts = spec
            bs, sims, mm, ev, es, nes, cp, fpu = case
            d = run("game", bs, sims, mm, nes, cp, fpu, *rules, nseed, 1 << ttl, *opts)
            d.update(case=list(case), rules=list(rules), noise_seed=nseed, tt_log2=ttl, opts=list(opts))
            print("game", case, rules, nseed, ttl, opts, "moves", len(d["moves"]), "terminal", d["terminal"], "result",
                  d["result"], flush=True)
            return d

        with concurrent.futures.ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as ex:
            game_jobs = [ex.submit(game, spec) for spec in GAME_CASES]
            pos = {}
            seed = 100
            for renju, omok in RULE_SETS:
                for bs, n, margin in POSITION_RUNS:
                    seed += 1
                    pos[f"{bs}-{renju}-{omok}-m{margin}"] = run("positions", bs, n, seed, renju, omok, margin)["positions"]
            pos["stalemate"] = [run("stalemate", 7, 1, 0, 1, 4000)["position"], run("stalemate", 7, 0, 1, 1, 4000)["position"],
                                run("stalemate", 6, 1, 0, 1, 20000)["position"]]
            pos["constructed"] = []
            for name, (bs, rules, moves, cell, verdict, want) in sorted(constructed().items()):
                p = run("replay", bs, *rules, *moves)
                p["name"] = name
                pos["constructed"].append(p)
            games = [j.result() for j in game_jobs]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    check(games, pos)
    with gzip.GzipFile(os.path.join(OUT, "ref_gomoku_rules_games.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(games, separators=(",", ":")).encode())
    with gzip.GzipFile(os.path.join(OUT, "ref_gomoku_rules_positions.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(pos, separators=(",", ":")).encode())
    print("wrote", OUT)


if __name__ == "__main__":
    main()
