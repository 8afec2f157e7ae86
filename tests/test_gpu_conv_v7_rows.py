"""conv3x3_v7's row-streamed main loop (csrc/conv_v7.hip: the SLIM 15x15 tile, every wave owns all 15
fragments of the board x 32 channels, tap weights in registers, one barrier per chunk) against the
per-tap loop it replaces as the default (conv flag 0x2000) and against conv3x3_v6 (flag 0x100).  All
three give every accumulator the same nine products per chunk in the same order, so the whole
network must be BITWISE equal, under both poisons and clean, in both 16-bit modes."""
import numpy as np
import pytest

V7 = 0xa04          # the library default 0x204 | 0x800: conv3x3_v7 takes 15x15 below 1024 boards too
PER_TAP = 0x2000    # conv3x3_v7's per-tap main loop
V6 = 0x100          # conv3x3_v6


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


def _flags(f):
    from az_amd import _lib
    _lib.lib().az_diag_set_conv_flags(int(f))


def _poison(byte):
    from az_amd import _lib
    _lib.lib().az_diag_set_poison(int(byte))


CASES = [  # channels, blocks, capacity, boards forwarded, flags selecting conv3x3_v7
    (128, 1, 1, 1, V7),            # one channel half, 4 chunks, one board
    (256, 2, 9, 9, V7),            # a second XCD group of tiles, mostly empty
    (256, 2, 37, 37, V7),          # ragged batch
    (256, 1, 1100, 1100, 0x204),   # several rounds of two blocks per CU (the drain hazard); v7 by default
    (384, 1, 3, 3, V7),            # 12 chunks
    (256, 1, 16, 5, V7),           # 5 of 16 boards: the device-side board limit, blocks that return at once
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_gpu_v7_rows_bitwise_equals_per_tap_and_v6(engine, case, mode):
    import az_amd
    import net_oracle
    ch, blocks, cap, B, fl = case
    prec = az_amd.AZ_PREC_FP16 if mode == "fp16" else az_amd.AZ_PREC_BF16
    desc = az_amd.NetDesc(15, 11, ch, blocks, 225, 32, 8, 256, 1, 0, prec, cap)
    net = az_amd.HipNeuralNetwork(engine, desc)
    _flags(fl)
    try:
        assert net.trunk_kernel() == f"conv3x3_v7<{2 if mode == 'fp16' else 1}, 15, SLIM>", net.trunk_kernel()
    finally:
        _flags(0x204)
    net.load_weights(net_oracle.init_blob(desc, seed=41))
    x = (np.random.default_rng(ch + B).random((B, 11, 15, 15)) < 0.25).astype(np.float32)
    outs = {}
    try:
        for name, f in (("v6", fl | V6), ("per-tap", fl | PER_TAP), ("rows", fl)):
            for byte in (0xff, 0x55, -1):
                _flags(f)
                _poison(byte)
                outs[f"{name}/{byte & 0xff:02x}" if byte >= 0 else f"{name}/clean"] = net.forward(x)
    finally:
        _poison(-1)
        _flags(0x204)                     # the library default
    l6, v6 = outs["v6/ff"]
    for name, (lo, v) in outs.items():
        bad = np.where((lo != l6).any(axis=1) | (v != v6))[0]
        print(f"{case} {mode} {name}: max|. - v6| logits {np.abs(lo - l6).max():.3e} value {np.abs(v - v6).max():.3e}, "
              f"boards differing {bad.tolist()[:16]} of {B}")
    assert np.abs(l6).max() > 0
    for name, (lo, v) in outs.items():
        assert np.isfinite(lo).all() and np.isfinite(v).all(), name
        assert np.array_equal(lo, l6) and np.array_equal(v, v6), name
    net.close()
