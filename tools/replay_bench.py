#!/usr/bin/env python3
"""Cost of the replay buffer (az_replay_*) on the C3 game shape: 15x15 Gomoku, 2048 game slots.

The stage / commit / gather kernels read roots and ring rows only, so their cost does not depend on the evaluator:
the games here run on the hash evaluator (no network), which keeps a run to seconds.  Prints
  - the GPU time of k_replay_stage per self-play step and of the k_replay_commit that commits all 2048 games (cut at
    --plies), by HIP events around the launches (az_diag_replay_profile),
  - the wall time of the same run with and without a buffer attached,
  - k_replay_gather at n = 4096 samples with symmetries, into torch device tensors: GPU time, positions/s and bytes
    written per second against the algorithmic 4 (C A + NA + 2) bytes per sample.
Usage: python tools/replay_bench.py [--games 2048] [--sims 200] [--plies 12] [--n 4096] [--reps 20]"""
import argparse
import ctypes
import os
import sys
import time

import torch  # before libaz_hip.so: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-multi-game_amd"))
import az_amd  # noqa: E402
from az_amd import _lib  # noqa: E402


def profile(rb, enable):
    f = _lib.lib().az_diag_replay_profile
    f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int64)]
    ms, n = (ctypes.c_double * 3)(), (ctypes.c_int64 * 3)()
    _lib.check(f(rb.h, int(enable), ms, n))
    return list(ms), list(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--sims", type=int, default=200)
    ap.add_argument("--plies", type=int, default=12)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    bs, G = 15, a.games
    eng = az_amd.Engine(0)
    print(f"device {eng.device_name}; {G} games of {bs}x{bs}, hash evaluator, {a.sims} simulations, cut at {a.plies} plies")

    def run(attach, prof=False):
        mgr = az_amd.SelfPlayManager(eng, numGames=G, numSimulations=a.sims, board_size=bs, evaluator=az_amd.AZ_EVAL_HASH,
                                     noise_seed_stride=1, tt_log2=16)
        rb = az_amd.ReplayBuffer(eng, az_amd.GAME_GOMOKU, bs, G * a.plies, a.plies) if attach else None
        if rb is not None:
            mgr.mcts.attachReplay(rb)
            if prof:
                profile(rb, 1)
        t0 = time.perf_counter()
        mgr.generateGames(totalGames=G, max_moves=a.plies)
        dt = time.perf_counter() - t0
        mgr.mcts.close()
        return dt, rb

    run(False)                                                   # warm-up
    walls = {k: [] for k in ("off", "on")}
    for _ in range(3):
        walls["off"].append(run(False)[0])
        dt, rb = run(True)
        walls["on"].append(dt)
        rb.close()
    for k, v in walls.items():
        print(f"wall, buffer {k:3s}: " + " ".join(f"{1e3 * x:8.1f}" for x in v) + f" ms per run of {a.plies} steps | "
              f"median {1e3 * sorted(v)[1] / a.plies:.3f} ms per step")
    _dt, rb = run(True, prof=True)
    ms, n = profile(rb, 0)
    info = rb.info()
    print(f"k_replay_stage : {n[0]} launches, {1e3 * ms[0] / max(1, n[0]):.1f} us per launch ({G} roots each)")
    print(f"k_replay_commit: {n[1]} launch(es), {1e3 * ms[1] / max(1, n[1]):.1f} us ({info['committed']} positions of "
          f"{info['games']} games)")
    C, A, NA = 11, bs * bs, bs * bs
    dev = torch.device("cuda:0")
    st = torch.empty((a.n, C, bs, bs), dtype=torch.float32, device=dev)
    po = torch.empty((a.n, NA), dtype=torch.float32, device=dev)
    z = torch.empty(a.n, dtype=torch.float32, device=dev)
    q = torch.empty(a.n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rb.seed(1)
    for _ in range(3):
        rb.sample_into(st, po, z, q, augment=True)
    profile(rb, 1)
    t0 = time.perf_counter()
    for _ in range(a.reps):
        rb.sample_into(st, po, z, q, augment=True)
    wall = (time.perf_counter() - t0) / a.reps
    ms, n = profile(rb, 0)
    k_ms = ms[2] / max(1, n[2])
    nbytes = 4 * (C * A + NA + 2) * a.n
    print(f"k_replay_gather: n = {a.n}, {n[2]} launches, {1e3 * k_ms:.1f} us per launch = {a.n / (1e-3 * k_ms):.3e} positions/s, "
          f"{nbytes} algorithmic bytes written = {nbytes / (1e-3 * k_ms) / 1e9:.1f} GB/s")
    print(f"sample_into    : {1e3 * wall:.3f} ms wall per call (plan, upload, gather, synchronise; events on) = "
          f"{a.n / wall:.3e} positions/s")
    rb.close()
    eng.close()


if __name__ == "__main__":
    main()
