#!/usr/bin/env python3
"""Regenerates the Go rule-option fixtures (komi, Chinese / Japanese scoring, superko / simple ko)
from the patched REFERENCE build:

    python3 tests/golden/gen_go_rules_golden.py [REFERENCE_ROOT]

Repeats oracle/build_ref.sh's recipe (patches P1, P5, P6; no arithmetic change) in a temp directory,
links tests/golden/go_rules_harness.cpp against it there, and writes only the harness' JSON output:
ref_go_rules_games.json.gz and ref_go_rules_positions.json.gz.  The binary and the temp copy are
deleted; nothing of the reference enters the repository.

The generator asserts the conditions the fixtures exist for (see check()).
"""
import glob
import gzip
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

OUT = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("REF", "/root/reference")

# (bs, sims, max_moves, evaluator, eval_seed, noise_each_search, cpuct, fpu) as gen_golden.py's
# GO_GAME_CASES, then (komi, chinese, superko), the noise seed and log2 of the table size
GAME_CASES = [
    ((9, 100, 80, "hash", 3, 0, 1.5, 0.0), (0.5, 1, 1), 42, 20),
    ((9, 100, 80, "hash", 3, 0, 1.5, 0.0), (7.0, 0, 1), 42, 20),
    ((9, 100, 80, "hash", 3, 0, 1.5, 0.0), (-40.5, 1, 1), 42, 20),   # extreme komi: terminal leaves flip
    ((9, 150, 40, "hash", 11, 0, 1.5, 0.0), (7.5, 1, 0), 42, 20),
    ((9, 60, 30, "hash", 5, 1, 1.5, 0.25), (5.5, 0, 0), 42, 20),     # per-search noise + FPU
    ((9, 30, 1000, "hash", 7, 0, 1.5, 0.0), (0.0, 1, 1), 42, 20),    # pass / pass on the empty board: DRAW
    ((9, 150, 40, "hash", 11, 0, 1.5, 0.0), (7.0, 0, 0), 42, 6),     # 64-entry table: slot collisions
    ((13, 300, 8, "hash", 7, 0, 1.5, 0.0), (6.5, 1, 0), 42, 20),
    # one case played with three noise seeds: the games of a three-game handle with stride 1
    ((9, 100, 80, "hash", 5, 0, 1.5, 0.0), (6.5, 0, 0), 42, 20),
    ((9, 100, 80, "hash", 5, 0, 1.5, 0.0), (6.5, 0, 0), 43, 20),
    ((9, 100, 80, "hash", 5, 0, 1.5, 0.0), (6.5, 0, 0), 44, 20),
]
# scoring x ko: (chinese, superko) -> (seed 9x9, seed 13x13)
POSITION_SEEDS = {(1, 1): (11, 21), (1, 0): (12, 22), (0, 1): (13, 23), (0, 0): (14, 24)}
KO_LIST = [3, 9, 11, 10, 1, -1, 0, 2]   # send two, return one: point 1 repeats a position


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


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
    patch("src/games/gomoku/gomoku_state.cpp", "zobrist_(core::GameType::GOMOKU, board_size, 2)", "zobrist_(board_size, 2, 2, 12345u)")  # P2 (links only)
    patch("src/games/go/go_state.cpp", "zobrist_(core::GameType::GO, board_size, 2)", "zobrist_(board_size, 2, 2, 12345u)")  # P6
    patch("include/alphazero/mcts/mcts_node.h", "std::mutex expansionMutex;", "std::recursive_mutex expansionMutex;")  # P5
    patch("src/mcts/parallel_mcts.cpp", r"std::lock_guard<std::mutex> lock\((rootNode_|node)->expansionMutex\)",
          r"std::lock_guard<std::recursive_mutex> lock(\1->expansionMutex)", count=6, regex=True)
    flags = ["-std=c++17", "-O2", "-pthread", "-DLIBTORCH_OFF", "-I" + os.path.join(tmp, "include")]
    procs, objs = [], []
    for f in glob.glob(os.path.join(tmp, "src", "*", "*.cpp")) + glob.glob(os.path.join(tmp, "src", "games", "*", "*.cpp")):
        o = os.path.join(tmp, os.path.basename(f)[:-4] + ".o")
        objs.append(o)
        procs.append(subprocess.Popen(["g++"] + flags + ["-w", "-c", f, "-o", o]))
    h = os.path.join(tmp, "go_rules_harness.o")
    procs.append(subprocess.Popen(["g++"] + flags + ["-c", os.path.join(OUT, "go_rules_harness.cpp"), "-o", h]))
    for p in procs:
        assert p.wait() == 0
    exe = os.path.join(tmp, "go_rules_harness")
    subprocess.run(["g++", "-pthread", h] + objs + ["-o", exe], check=True)
    return exe


def own_captures_result(p):
    """The result the own-captures prisoner formula would give (not the reference's crediting)."""
    b, w = f32(p["score"][0]), f32(p["score"][1])
    c1, c2 = p["captured"]
    b, w = b - c2 + c1, w - c1 + c2
    return 2 if b > w else 3 if w > b else 1   # GameResult: ONGOING 0, DRAW 1, WIN_PLAYER1 2, WIN_PLAYER2 3


def check(games, pos):
    with gzip.open(os.path.join(OUT, "ref_go_games.json.gz"), "rt") as f:
        default = json.load(f)
    a, b = pos["ko"]
    assert a["superko"] == 1 and b["superko"] == 0
    assert set(b["legal"]) - set(a["legal"]) == {1} and not set(a["legal"]) - set(b["legal"]), "constructed ko position"
    assert [x for x in b["legal"] if x != 1] == a["legal"]
    assert any(p["terminal"] and not p["chinese"] and p["captured"][0] != p["captured"][1] and
               p["result"] != own_captures_result(p) for k in pos if k != "ko" for p in pos[k]), "prisoner crediting"
    d3 = [g for g in default if g["case"][4] == 3][0]
    assert any(g["case"][4] == 3 and [m["action"] for m in g["moves"]] != [m["action"] for m in d3["moves"]]
               for g in games), "the rules never reached the search"
    for chinese in (0, 1):
        assert any(g["rules"][1] == chinese and g["terminal"] and g["result"] != 0 for g in games), chinese
    k0 = [g for g in games if g["rules"][0] == 0.0][0]
    assert k0["terminal"] and k0["result"] == 1 and [m["action"] for m in k0["moves"]] == [-1, -1], "komi 0 is a DRAW"


def main():
    tmp = tempfile.mkdtemp(prefix="az_gorules.")
    try:
        exe = build(tmp)

        def run(*args):
            r = subprocess.run([exe] + [str(x) for x in args], capture_output=True, text=True, timeout=1800)
            if r.returncode != 0:
                sys.exit(f"harness failed: {args}: {r.stderr}")
            return json.loads(r.stdout)

        games = []
        for case, rules, nseed, ttl in GAME_CASES:
            bs, sims, mm, ev, es, nes, cp, fpu = case
            d = run("game", bs, sims, mm, nes, cp, fpu, *rules, nseed, 1 << ttl)
            d.update(case=list(case), rules=list(rules), noise_seed=nseed, tt_log2=ttl)
            games.append(d)
            print("game", case, rules, nseed, ttl, "moves", len(d["moves"]), "terminal", d["terminal"], "result", d["result"])
        pos = {}
        for (chinese, superko), (s9, s13) in POSITION_SEEDS.items():
            for bs, n, seed in ((9, 32, s9), (13, 8, s13)):
                pos[f"{bs}-{chinese}-{superko}"] = run("positions", bs, n, seed, chinese, superko)["positions"]
        pos["ko"] = [run("replay", 9, 7.5, 1, sk, *KO_LIST) for sk in (1, 0)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    check(games, pos)
    with gzip.GzipFile(os.path.join(OUT, "ref_go_rules_games.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(games, separators=(",", ":")).encode())
    with gzip.GzipFile(os.path.join(OUT, "ref_go_rules_positions.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(pos, separators=(",", ":")).encode())
    print("wrote", OUT)


if __name__ == "__main__":
    main()
