"""tests/wave_model.py -- TEST INFRASTRUCTURE ONLY.

ctypes wrapper of tests/wave_model.cpp: the leaf-parallel (K leaves per wave) schedule derived from
the CPU restatement oracle/az_oracle.cpp, which the .cpp includes unchanged.  Built lazily with g++
into tests/_build/ (git-ignored), as oracle/az_oracle.py builds liboracle.so; the flags are the
oracle Makefile's less -Wall (the including unit leaves oracle helpers unused).
"""
import ctypes
import json
import os
import subprocess

import numpy as np

import az_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "wave_model.cpp")
ORACLE_SRC = os.path.join(os.path.dirname(HERE), "oracle", "az_oracle.cpp")
LIB_PATH = os.path.join(HERE, "_build", "libwave_model.so")

STAT_KEYS = ("same_leaf", "wave_tt_hits", "expanded_miss", "short_waves")


def build():
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    tmp = LIB_PATH + ".%d.tmp" % os.getpid()
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
                    "-w", "-shared", SRC, "-o", tmp], check=True)
    os.replace(tmp, LIB_PATH)


_lib = None


def lib():
    global _lib
    if _lib is None:
        stale = not os.path.exists(LIB_PATH) or \
            os.path.getmtime(LIB_PATH) < max(os.path.getmtime(SRC), os.path.getmtime(ORACLE_SRC))
        if stale:
            build()
        L = ctypes.CDLL(LIB_PATH)
        L.wave_model_play.restype = ctypes.c_void_p
        L.wave_model_play.argtypes = [ctypes.POINTER(O.OracleCfg), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                      O.EVAL_CB, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
        L.az_oracle_free.argtypes = [ctypes.c_void_p]
        _lib = L
    return _lib


def play_raw(leaves=1, seed_stride=0, evaluator=None, **kw):
    """(games JSON, stats JSON) as the library wrote them.  leaves: K, or a per-ply list of K (the last
    entry holds for every later ply); the other arguments are az_oracle.play's."""
    cfg = O.make_cfg(**kw)
    ks = [int(leaves)] if np.isscalar(leaves) else [int(k) for k in leaves]
    assert ks and all(k >= 1 for k in ks)

    def _cb(user, game, planes, n_planes, A, pol, val):
        try:
            bs = int(round((A - (1 if cfg.game == O.GAME_GO else 0)) ** 0.5))
            x = np.ctypeslib.as_array(planes, shape=(n_planes, bs, bs)).copy()
            p, v = evaluator(game, x)
            p = np.asarray(p, dtype=np.float32).reshape(-1)
            ctypes.memmove(pol, p.ctypes.data, 4 * A)
            val[0] = float(v)
            return 0
        except O.StopPlay:
            return 2
        except Exception as e:  # surfaced as an abort in the model
            print("wave model evaluator failed:", repr(e))
            return 1

    cb = O.EVAL_CB(_cb)
    arr = (ctypes.c_int * len(ks))(*ks)
    stats = ctypes.c_void_p(None)
    L = lib()
    ptr = L.wave_model_play(ctypes.byref(cfg), seed_stride, arr, len(ks), cb, None, ctypes.byref(stats))
    if not ptr:
        raise ValueError("wave_model_play: unsupported configuration")
    try:
        s = ctypes.string_at(ptr).decode()
        t = ctypes.string_at(stats.value).decode() if stats.value else "null"
    finally:
        L.az_oracle_free(ptr)
        if stats.value:
            L.az_oracle_free(stats.value)
    return s, t


def play(leaves=1, seed_stride=0, evaluator=None, **kw):
    """az_oracle.play's per-game dicts under the wave schedule, each with a "wave" dict of the game's
    counters: same_leaf (a descent ending on the leaf of an earlier descent of its wave), wave_tt_hits
    (a TT hit on an entry stored earlier in the same wave), expanded_miss (the getValue() branch taken
    because a wave-mate expanded the node) and short_waves."""
    s, t = play_raw(leaves, seed_stride, evaluator, **kw)
    games = json.loads(s)
    if games is None:
        return None
    for g, st in zip(games, json.loads(t)):
        g["wave"] = st
    return games
