"""The model-parity cases of the leaf-parallel search, shared by tests/test_wave_model_cpu.py (the model's
counters show each case meets the event it is there for) and tests/test_gpu_wave.py (the device against the
model).  Each case: the wave_model.play / az_oracle.play settings, K, and the event counters that must be > 0."""
import az_oracle as O

# id: (K, play settings, events)
CASES = {
    "a-6x6-hash-k4":      (4, dict(seed_stride=1, bs=6, sims=96, max_moves=10, n_games=3, eval_kind=O.EVAL_HASH), ()),
    # 50 = 6 x 8 + 2: every search ends on a short wave
    "b-7x7-random-k8":    (8, dict(seed_stride=1, bs=7, sims=50, max_moves=8, n_games=2, eval_kind=O.EVAL_RANDOM, eval_seed=5),
                           ("short_waves",)),
    # a 16-cell board: every wave past the opening has more descents than children; played to the draw
    "c-4x4-hash-k16":     (16, dict(seed_stride=1, bs=4, sims=64, n_games=2, eval_kind=O.EVAL_HASH),
                           ("same_leaf", "wave_tt_hits")),
    # a 16-slot table.  On 6x6 with K = 8 no two descents of a wave share a leaf in the first 8 moves at any
    # simulation count or seed tried (120 .. 4000 sims, seeds 42 .. 47: same_leaf = 0), so the store a wave-mate
    # is refused never matters there; the case stays for the replacement rule under a wave, and the 4x4 case
    # below is the small-table case that reaches the getValue() branch
    "d-6x6-tt4-k8":       (8, dict(bs=6, sims=120, max_moves=8, tt_log2=4, eval_kind=O.EVAL_HASH), ()),
    "d2-4x4-tt4-k16":     (16, dict(bs=4, sims=64, tt_log2=4, eval_kind=O.EVAL_HASH), ("same_leaf", "expanded_miss")),
    # 40 = 32 + 8
    "e-9x9-uniform-k32":  (32, dict(bs=9, sims=40, max_moves=4, eval_kind=O.EVAL_UNIFORM), ("short_waves",)),
    # 40 simulations over 82 children: both sides pass at once (as at K = 1); f2 plays stones
    "f-go9-hash-k4":      (4, dict(seed_stride=1, bs=9, sims=40, max_moves=10, n_games=2, eval_kind=O.EVAL_HASH, game=O.GAME_GO), ()),
    "f2-go9-hash-k4-120": (4, dict(seed_stride=1, bs=9, sims=120, max_moves=6, n_games=2, eval_kind=O.EVAL_HASH, game=O.GAME_GO), ()),
}
