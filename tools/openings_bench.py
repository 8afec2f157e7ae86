#!/usr/bin/env python3
"""What starting games from an opening costs: one az_search_new_games_moves (k_open_games: every slot's sequence in
one launch, judged by a dry pass first) against the same state reached by az_search_new_games_ids and one
az_search_apply per ply (a k_apply, a k_compact of every tree and a stream synchronisation per ply).

Shapes: the C3 handle (2048 slots, Gomoku 15x15, 800 simulations) and Go 19x19 on 2048 slots, 8-ply openings that
differ from slot to slot.  Every call returns after the engine's stream is idle, so the wall time of a call is the
time the device and the host spent on it together.  The engine's stream is private to the library and
non-blocking, so no event of the caller's brackets its work: a device-only time is not reported.  Medians of --reps
calls after one warm-up.  Prints a table; the last line is a JSON summary."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-multi-game_amd"))

import numpy as np   # noqa: E402

import az_amd        # noqa: E402


def openings(bs, slots, plies, rng):
    """`plies` distinct cells per slot, away from each other so that nothing is captured and no five can form."""
    cells = np.array([r * bs + c for r in range(0, bs, 2) for c in range(0, bs, 3)], np.int32)
    return [rng.permutation(cells)[:plies].tolist() for _ in range(slots)]


def measure(fn, reps):
    fn()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(wall)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, default=2048)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    eng = az_amd.Engine(0)
    rng = np.random.default_rng(0)
    rows = []
    for name, bs, game in (("gomoku 15x15", 15, az_amd.AZ_GAME_GOMOKU), ("go 19x19", 19, az_amd.AZ_GAME_GO)):
        m = az_amd.ParallelMCTS(eng, n_games=args.slots, board_size=bs, num_simulations=args.sims,
                                evaluator=az_amd.AZ_EVAL_HASH, game=game)
        try:
            seqs = openings(bs, args.slots, args.plies, rng)
            ids = np.arange(args.slots, dtype=np.int32)
            # the C calls on arrays packed beforehand: no Python list handling inside the timed region
            L, check = az_amd.lib(), az_amd.check
            mv = np.ascontiguousarray(seqs, np.int32)
            nm = np.full(args.slots, args.plies, np.int32)
            cols = [np.ascontiguousarray(mv[:, ply]) for ply in range(args.plies)]
            term, res = np.zeros(args.slots, np.int32), np.zeros(args.slots, np.int32)
            ip = ctypes.POINTER(ctypes.c_int)

            def composed():
                check(L.az_search_new_games_ids(m.h, ids.ctypes.data, ids.ctypes.data, args.slots))
                for col in cols:
                    check(L.az_search_apply(m.h, col.ctypes.data_as(ip), term.ctypes.data_as(ip), res.ctypes.data_as(ip)))

            def opened():
                check(L.az_search_new_games_moves(m.h, ids.ctypes.data, ids.ctypes.data, args.slots, mv.ctypes.data,
                                                  nm.ctypes.data, args.plies))

            one = measure(opened, args.reps)
            per = measure(composed, args.reps)
            fresh = measure(lambda: m.newGames(ids=ids), args.reps)
        finally:
            m.close()
        row = dict(shape=name, slots=args.slots, plies=args.plies, new_games_moves_wall_ms=one, ids_plus_applies_wall_ms=per,
                   new_games_ids_wall_ms=fresh, ratio_wall=per / one)
        rows.append(row)
        print(f"{name}, {args.slots} slots, {args.plies}-ply openings (wall, median of {args.reps}):")
        print(f"  az_search_new_games_moves          {one:9.3f} ms")
        print(f"  new_games_ids + {args.plies} az_search_apply   {per:9.3f} ms")
        print(f"  az_search_new_games_ids alone      {fresh:9.3f} ms")
        print(f"  ratio (applies / one call)         {row['ratio_wall']:9.2f} x")
    eng.close()
    print(json.dumps({"openings_bench": rows}))


if __name__ == "__main__":
    main()
