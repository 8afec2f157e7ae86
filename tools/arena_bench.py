#!/usr/bin/env python3
"""The evaluation match on one handle against the same match composed from two single-net handles.

  arena        az_amd.Arena: one search handle of 2 x tables slots with per-slot nets; every simulation step
               partitions its leaf batch by net (k_scan_nets) and runs one forward per net
  composition  two ParallelMCTS handles of `tables` slots, one per net, driven through the masked entry
               points (search(mask), select, updateWithMove on both): the path the API had before the arena

Both play the same plies (colours swapped every game, so each net moves on half of the tables in every ply;
no noise, the deterministic selection rule) in one process on one device, alternating in rounds after one
warm-up ply each.  Per round and mode: positions/s, evaluations/s of each net and milliseconds per lock-step
simulation step (wall time of a ply over its simulations).  Net: 15x15, --blocks x --channels, fp16 trunk,
counter-based random init (two seeds)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-multi-game_amd"))
import az_amd  # noqa: E402


def evals(m, slots):
    return sum(m.counters(g)["evals"] for g in slots)


class Composition:
    def __init__(self, eng, nets, T, bs, sims, tt_log2):
        self.T = T
        self.hs = [az_amd.ParallelMCTS(eng, n_games=T, board_size=bs, num_simulations=sims, evaluator=az_amd.AZ_EVAL_NET,
                                       net=nets[p], noise_seed=42, noise_seed_stride=1, tt_log2=tt_log2) for p in (0, 1)]
        for p in (0, 1):
            self.hs[p].newGames(np.arange(T), ids=2 * np.arange(T) + p)
        self.ply = 0

    def step(self):
        T = self.T
        a_moves = (np.arange(T) % 2 == 0) == (self.ply % 2 == 0)       # swapped colours: game id = table
        acts = np.zeros(T, np.int32)
        for p, mask in ((0, a_moves), (1, ~a_moves)):
            self.hs[p].search(mask=mask.astype(np.uint8))
            act = self.hs[p].select(True, 0.1)[0]
            acts[mask] = act[mask]
        for h in self.hs:
            h.updateWithMove(acts)
        self.ply += 1
        return T

    def evals(self):
        return [evals(h, range(self.T)) for h in self.hs]

    def close(self):
        for h in self.hs:
            h.close()


class OneHandle:
    def __init__(self, eng, nets, T, bs, sims, tt_log2):
        self.T = T
        self.ar = az_amd.Arena(eng, nets[0], nets[1], T, board_size=bs, num_simulations=sims, swap_colors=True,
                               temperature=0.1, tt_log2=tt_log2)

    def step(self):
        return self.ar.step()

    def evals(self):
        return [evals(self.ar.search, range(p, 2 * self.T, 2)) for p in (0, 1)]

    def close(self):
        self.ar.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=512)
    ap.add_argument("--board", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=20)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--sims", type=int, default=64)
    ap.add_argument("--plies", type=int, default=3, help="timed plies per round and mode")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tt-log2", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    eng = az_amd.Engine(0)
    nets = []
    for seed in (9, 10):
        n = az_amd.HipNeuralNetwork(eng, az_amd.gomoku_net_desc(a.board, a.channels, a.blocks, az_amd.AZ_PREC_FP16,
                                                                 max_batch=a.tables))
        n.init_random(seed)
        nets.append(n)
    modes = {"arena": OneHandle(eng, nets, a.tables, a.board, a.sims, a.tt_log2),
             "composition": Composition(eng, nets, a.tables, a.board, a.sims, a.tt_log2)}
    lines = [f"arena_bench: {eng.device_name}, {a.board}x{a.board}, {a.blocks}b x {a.channels}f fp16 ({nets[0].trunk_kernel()}), "
             f"{a.tables} tables, {a.sims} sims, {a.plies} timed plies per round after 1 warm-up ply",
             "mode         round  positions/s  evals/s A  evals/s B  ms/sim-step"]
    for m in modes.values():
        m.step()
    rate = {k: [] for k in modes}
    for r in range(a.rounds):
        for name, m in modes.items():
            e0 = m.evals()
            t0 = time.perf_counter()
            moves = sum(m.step() for _ in range(a.plies))
            dt = time.perf_counter() - t0
            e1 = m.evals()
            rate[name].append(moves / dt)
            lines.append(f"{name:12s} {r:5d}  {moves / dt:11.1f}  {(e1[0] - e0[0]) / dt:9.0f}  {(e1[1] - e0[1]) / dt:9.0f}  "
                         f"{dt / (a.plies * a.sims) * 1e3:11.3f}")
    best = {k: max(v) for k, v in rate.items()}
    lines.append(f"best round: arena {best['arena']:.1f} positions/s, composition {best['composition']:.1f} positions/s, "
                 f"arena / composition = {best['arena'] / best['composition']:.3f}")
    for m in modes.values():
        m.close()
    for n in nets:
        n.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
