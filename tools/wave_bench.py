#!/usr/bin/env python3
"""Leaf-parallel search (az_search_set_leaves) against the plain search at small and large batches.

For every configuration and K in --leaves: one self-play handle of G games with the 20-block x 256-filter fp16
net, one warm-up move, then --moves timed moves of --sims simulations (az_selfplay_step, finished games
restart, so every game plays in every step):

  sims_per_s      G x sims x moves / seconds
  evals_per_s     network evaluations the completions consumed (the `evals` counters) / seconds
  discarded       1 - consumed / forwarded.  With every game playing and K dividing sims every simulation
                  step runs the identity batch, so the net forwards G x K leaves per wave = G x sims per move
                  at every K; what the completions do not consume (terminal leaves, TT hits, a wave-mate's
                  expansion or store) is dropped.

Configurations: Gomoku 15x15 at G = 1, 16, 256 and Go 19x19 at G = 128.  Every (configuration, K) runs in a
child process of its own under `timeout`; a child that fails or overruns is recorded and nothing more is started.
Writes profiles/r09_wave_bench.json (--out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-multi-game_amd"))

CONFIGS = [("gomoku", 15, 1), ("gomoku", 15, 16), ("gomoku", 15, 256), ("go", 19, 128)]


def one(a):
    import az_amd
    go = a.game == "go"
    G, K, bs = a.games, a.k, a.board
    eng = az_amd.Engine(0)
    if go:
        desc = az_amd.NetDesc(bs, 8, a.channels, a.blocks, bs * bs + 1, 32, 8, 256, 1, 0, az_amd.AZ_PREC_FP16, G * K)
    else:
        desc = az_amd.gomoku_net_desc(board_size=bs, channels=a.channels, blocks=a.blocks, precision=az_amd.AZ_PREC_FP16,
                                      max_batch=G * K)
    net = az_amd.HipNeuralNetwork(eng, desc)
    net.init_random(1234)
    m = az_amd.ParallelMCTS(eng, net=net, n_games=G, board_size=bs, num_simulations=a.sims, evaluator=az_amd.AZ_EVAL_NET,
                            noise_seed=42, noise_seed_stride=1, game=az_amd.AZ_GAME_GO if go else az_amd.AZ_GAME_GOMOKU,
                            leaves=K)
    try:
        m.newGames()
        m.addDirichletNoise(0.03, 0.25)
        m.selfplayStep()                                     # warm-up
        ev0 = [m.counters(g)["evals"] for g in range(G)]
        t0 = time.perf_counter()
        moves = 0
        for _ in range(a.moves):
            mv, _ = m.selfplayStep()
            moves += mv
        dt = time.perf_counter() - t0
        ev1 = [m.counters(g)["evals"] for g in range(G)]
    finally:
        m.close()
        net.close()
        eng.close()
    restarted = any(b < a_ for a_, b in zip(ev0, ev1))       # a new game resets its slot's counter
    consumed = None if restarted else sum(b - a_ for a_, b in zip(ev0, ev1))
    forwarded = G * a.sims * a.moves if a.sims % K == 0 else None
    print(json.dumps({"game": a.game, "board": bs, "games": G, "leaves": K, "sims": a.sims, "moves": moves,
                      "seconds": dt, "sims_per_s": G * a.sims * a.moves / dt,
                      "evals_per_s": None if consumed is None else consumed / dt,
                      "discarded": None if consumed is None or forwarded is None else 1.0 - consumed / forwarded}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", default="1,2,4,8,16")
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--moves", type=int, default=3)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds per (configuration, K) child")
    ap.add_argument("--configs", default="", help="subset, e.g. gomoku:15:1,go:19:128 (default: all four)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_wave_bench.json"))
    ap.add_argument("--one", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--game", default="gomoku", help=argparse.SUPPRESS)
    ap.add_argument("--board", type=int, default=15, help=argparse.SUPPRESS)
    ap.add_argument("--games", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, default=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a)
    configs = CONFIGS
    if a.configs:
        configs = [(g, int(b), int(n)) for g, b, n in (c.split(":") for c in a.configs.split(","))]
    ks = [int(k) for k in a.leaves.split(",")]
    rows, stopped = [], None
    for game, board, G in configs:
        for K in ks:
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--one",
                   "--game", game, "--board", str(board), "--games", str(G), "--k", str(K), "--sims", str(a.sims),
                   "--moves", str(a.moves), "--channels", str(a.channels), "--blocks", str(a.blocks)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode == 0:
                row = json.loads(r.stdout.strip().splitlines()[-1])
                rows.append(row)
                print(f"{game} {board}x{board} G={G} K={K}: {row['sims_per_s']:.0f} sims/s, "
                      f"{row['evals_per_s'] or 0:.0f} evals/s, discarded {row['discarded']}", file=sys.stderr, flush=True)
            else:
                rows.append({"game": game, "board": board, "games": G, "leaves": K, "failed": r.returncode,
                             "stderr": r.stderr[-400:]})
                print(f"{game} G={G} K={K}: exit {r.returncode}\n{r.stderr[-400:]}", file=sys.stderr, flush=True)
                stopped = f"{game} G={G} K={K}: exit {r.returncode}"   # whatever ended it: start nothing more
                break
            with open(a.out, "w") as f:                       # kept current: a later stop loses nothing
                json.dump({"net": f"{a.blocks}b x {a.channels}f fp16", "sims": a.sims, "timed_moves": a.moves,
                           "stopped": stopped, "rows": rows}, f, indent=1)
        if stopped:
            break
    with open(a.out, "w") as f:
        json.dump({"net": f"{a.blocks}b x {a.channels}f fp16", "sims": a.sims, "timed_moves": a.moves, "stopped": stopped,
                   "rows": rows}, f, indent=1)
    by = {(r["game"], r["games"], r["leaves"]): r for r in rows if "sims_per_s" in r}
    if ("gomoku", 1, 8) in by and ("gomoku", 1, 1) in by:
        ratio = by[("gomoku", 1, 8)]["sims_per_s"] / by[("gomoku", 1, 1)]["sims_per_s"]
        print(f"G = 1: K = 8 / K = 1 = {ratio:.2f}x simulations/s", file=sys.stderr)
        if ratio <= 1.0:
            return 3
    return 2 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
