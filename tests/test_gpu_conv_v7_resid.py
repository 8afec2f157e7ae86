"""conv3x3_v7's row-streamed tile tail (csrc/conv_v7.hip): the last chunk is peeled, a 2nd conv's
residual tile arrives during the main loop (its 16-bit plane by LDS-DMA into the block's LDS, its int8
remainder in one burst of loads) and the join reads it from there.  Against the tile tail it replaces
(conv flag 0x4000: the last chunk reloads itself, the join reads global memory), the per-tap loop
(0x2000) and conv3x3_v6 (0x100).  The values joined and the arithmetic are the same in all four, so
the whole network must be BITWISE equal, under both poisons and clean, in both 16-bit modes.  The
boards differ from one another, so a stale or misplaced residual image shows."""
import numpy as np
import pytest

V7 = 0xa04          # the library default 0x204 | 0x800: conv3x3_v7 takes 15x15 below 1024 boards too
OLD_TAIL = 0x4000   # the row-streamed loop with the unpeeled tile tail
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


CASES = [  # channels, blocks, capacity, boards forwarded, NetDesc residual flag
    (128, 1, 1, 1, 1),        # four chunks, the fewest a trunk has: the staging schedule compressed
    (256, 2, 9, 9, 1),        # eight chunks, two channel halves, a second XCD group mostly empty, conv2 -> next residual
    (384, 1, 3, 3, 1),        # twelve chunks: more chunks than staged rows
    (256, 1, 16, 5, 1),       # the device-side board limit: blocks that return before issuing any DMA
    (256, 1, 520, 520, 1),    # 1040 blocks, over two rounds of two per CU: LDS a previous block's images just left
    (128, 1, 3, 3, 0),        # no residual: Rhi null on the second conv too, nothing may be prefetched
]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_gpu_v7_resid_prefetch_bitwise_equals_old_tail_per_tap_and_v6(engine, case, mode):
    import az_amd
    import net_oracle
    ch, blocks, cap, B, residual = case
    prec = az_amd.AZ_PREC_FP16 if mode == "fp16" else az_amd.AZ_PREC_BF16
    desc = az_amd.NetDesc(15, 11, ch, blocks, 225, 32, 8, 256, residual, 0, prec, cap)
    net = az_amd.HipNeuralNetwork(engine, desc)
    _flags(V7)
    try:
        assert net.trunk_kernel() == f"conv3x3_v7<{2 if mode == 'fp16' else 1}, 15, SLIM>", net.trunk_kernel()
    finally:
        _flags(0x204)
    net.load_weights(net_oracle.init_blob(desc, seed=43))
    x = (np.random.default_rng(7 * ch + B).random((B, 11, 15, 15)) < 0.25).astype(np.float32)
    assert len({x[b].tobytes() for b in range(B)}) == B       # every board its own input
    outs = {}
    try:
        for name, f in (("v6", V7 | V6), ("per-tap", V7 | PER_TAP), ("old-tail", V7 | OLD_TAIL), ("new", V7)):
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
