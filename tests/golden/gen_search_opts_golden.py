#!/usr/bin/env python3
"""Regenerates the search-option fixtures (selection strategy, depth cap, TD(lambda) backup,
progressive widening) from the patched REFERENCE build:

    python3 tests/golden/gen_search_opts_golden.py [REFERENCE_ROOT]

Repeats oracle/build_ref.sh's recipe (patches P1, P2, P5, P6; no arithmetic change) in a temp directory,
links tests/golden/search_opts_harness.cpp against it there, and writes only the harness' JSON output:
ref_search_opts_games.json.gz and ref_search_opts_widening.json.  The binary and the temp copy are
deleted; nothing of the reference enters the repository.

The generator asserts the conditions the fixtures exist for (see check()).
"""
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

UCB, PUCT, PBIAS, RAVE = 0, 1, 2, 3
DEFAULTS = dict(selection=PUCT, max_search_depth=1000, use_td=0, td_lambda=0.8, use_widening=0, widening_min_visits=10,
                widening_base=2.0, widening_exponent=0.5)
ORDER = ("selection", "max_search_depth", "use_td", "td_lambda", "use_widening", "widening_min_visits", "widening_base",
         "widening_exponent")
TD = dict(use_td=1)
WID = dict(use_widening=1)


def case(name, go, bs, sims, mm, opts, ev="hash", es=7, nes=0, cp=1.5, fpu=0.0, vl=3, seed=42, switch_ply=-1, switch=None):
    """`case` is gen_golden.py's tuple (bs, sims, max_moves, evaluator, eval_seed, noise_each_search, cpuct, fpu)."""
    return dict(name=name, go=go, case=[bs, sims, mm, ev, es, nes, cp, fpu], virtual_loss=vl, noise_seed=seed,
                opts=dict(DEFAULTS, **opts), switch_ply=switch_ply, switch=dict(DEFAULTS, **(switch or {})))


GAME_CASES = [
    case("td0.8", 0, 9, 100, 40, dict(TD, td_lambda=0.8)),
    case("td0.5-fpu-noise", 0, 9, 100, 30, dict(TD, td_lambda=0.5), nes=1, fpu=0.25),
    case("td0.3-5x5", 0, 5, 300, 25, dict(TD, td_lambda=0.3)),                      # transposition hits
    case("depth1-5x5", 0, 5, 300, 25, dict(max_search_depth=1)),
    case("depth2", 0, 9, 150, 81, dict(max_search_depth=2)),
    case("pbias", 0, 9, 100, 25, dict(selection=PBIAS)),
    case("pbias-go", 1, 9, 100, 25, dict(selection=PBIAS)),
    case("ucb", 0, 9, 60, 20, dict(selection=UCB)),       # COINCIDE: no root child is visited twice
    case("ucb-100", 0, 9, 100, 20, dict(selection=UCB)),
    case("widening", 0, 9, 100, 25, WID),
    case("widening-go", 1, 9, 100, 25, WID),
    case("widening-min1-vl1", 0, 9, 100, 25, dict(WID, widening_min_visits=1, widening_base=1.0), vl=1),
    case("widening-pbias-td-random", 0, 9, 100, 20, dict(WID, selection=PBIAS, use_td=1), ev="random", es=5),
    case("widening-13x13", 0, 13, 300, 6, WID),                                     # > 64 children decremented per node
    # one case played with three noise seeds: the games of a three-game handle with stride 1
    case("td-seed43", 0, 9, 150, 25, dict(TD, td_lambda=0.6), seed=43),
    case("td-seed44", 0, 9, 150, 25, dict(TD, td_lambda=0.6), seed=44),
    case("td-seed42", 0, 9, 150, 25, dict(TD, td_lambda=0.6), seed=42),
    # 6 plies of PUCT, then PROGRESSIVE_BIAS + TD on the kept tree (the reference's setters)
    case("switch", 0, 9, 100, 16, {}, switch_ply=6, switch=dict(selection=PBIAS, use_td=1)),
]
# 60 simulations on roots of more than 60 children: every simulation opens an unvisited child (FLT_MAX under
# both strategies), so this UCB case plays the PUCT game; ucb-100 is the UCB case that differs
COINCIDE = ("ucb",)
WIDENING_PARAMS = [(2.0, 0.5), (1.0, 0.5), (3.0, 0.8), (0.5, 1.0)]
WIDENING_CHILDREN = (82, 362)
WIDENING_RANGE = (-4, 4096)


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
    h = os.path.join(tmp, "search_opts_harness.o")
    procs.append(subprocess.Popen(["g++"] + flags + ["-c", os.path.join(OUT, "search_opts_harness.cpp"), "-o", h]))
    for p in procs:
        assert p.wait() == 0
    exe = os.path.join(tmp, "search_opts_harness")
    subprocess.run(["g++", "-pthread", h] + objs + ["-o", exe], check=True)
    return exe


def actions(g):
    return [m["action"] for m in g["moves"]]


def check(games, plain):
    """What the fixtures exist for; tests/test_search_opts_host.py asserts the same on the files."""
    for g in games:
        assert (actions(g) == plain[g["name"]]) == (g["name"] in COINCIDE), (g["name"], "the game without its options")
        if g["opts"]["use_widening"]:
            assert g["min_child_n"] < 0, (g["name"], "no root child with a negative visit count")
    seeds = [g for g in games if g["name"].startswith("td-seed")]
    assert sorted(g["noise_seed"] for g in seeds) == [42, 43, 44] and len({tuple(actions(g)) for g in seeds}) == 3
    assert any(len(m["children"]) > 64 and sum(c[1] < 0 for c in m["children"]) > 64
               for g in games if g["case"][0] == 13 for m in g["moves"]), "13x13: more than 64 decremented children"
    assert any(g["moves"][-1]["tt_hits"] > 0 for g in games if g["opts"]["use_td"] and g["case"][0] == 5), "TD with TT hits"


def main():
    tmp = tempfile.mkdtemp(prefix="az_searchopts.")
    try:
        exe = build(tmp)

        def run(*args):
            r = subprocess.run([exe] + [str(x) for x in args], capture_output=True, text=True, timeout=1800)
            if r.returncode != 0:
                sys.exit(f"harness failed: {args}: {r.stderr}")
            return json.loads(r.stdout)

        def game(c, opts, switch_ply, switch):
            bs, sims, mm, ev, es, nes, cp, fpu = c["case"]
            return run("game", c["go"], bs, sims, mm, ev, es, nes, cp, fpu, c["virtual_loss"], c["noise_seed"],
                       *[opts[k] for k in ORDER], switch_ply, *[switch[k] for k in ORDER])

        games, plain = [], {}
        for c in GAME_CASES:
            d = game(c, c["opts"], c["switch_ply"], c["switch"])
            d.update(c)
            # the same game without the options: only its actions are kept, for check() and the CPU test
            plain[c["name"]] = actions(game(c, DEFAULTS, -1, DEFAULTS))
            d["plain_actions"] = plain[c["name"]]
            games.append(d)
            print("game", c["name"], "moves", len(d["moves"]), "evals", d["moves"][-1]["evals"], "min child N", d["min_child_n"])
        wid = []
        for base, exponent in WIDENING_PARAMS:
            for children in WIDENING_CHILDREN:
                w = run("widening", base, exponent, children, *WIDENING_RANGE)
                w.update(base=base, exponent=exponent)
                wid.append(w)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    check(games, plain)
    with gzip.GzipFile(os.path.join(OUT, "ref_search_opts_games.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(games, separators=(",", ":")).encode())
    with open(os.path.join(OUT, "ref_search_opts_widening.json"), "w") as f:
        json.dump(wid, f, separators=(",", ":"))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
