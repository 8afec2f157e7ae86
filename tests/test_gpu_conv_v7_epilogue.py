"""conv3x3_v7's row-streamed path has an epilogue of its own (csrc/conv_v7.hip, epilogue_rows): the
residual / remainder-plane tests are compile-time facts, the stores go through one buffer resource per
output plane based at the wave's tile, and the dead 16th grid column is one execution mask.  Conv flag
0x8000 keeps the shared tile epilogue.  Values, arithmetic and stored bytes are the same, so whole
nets must be BITWISE equal under the lean epilogue (0xa04), the shared one (| 0x8000), the unpeeled
tile tail (| 0x4000), the per-tap loop (| 0x2000) and conv3x3_v6 (| 0x100), under both poisons and
clean, in both 16-bit modes.  Every board has its own input.

Which case reaches which compiled copy of the lean epilogue (net_forward launches three combinations
of residual tile x remainder plane; a residual without a remainder plane is launched by nobody):
  * (no residual, no remainder): the first conv of every block, every case;
  * (residual, remainder): the second conv of every block of the cases with residual = 1; in the
    256-channel, 2-block case its output is the next block's residual, so a misplaced 16-bit or int8
    store shows one block later;
  * (no residual, remainder): the second conv of the residual = 0 case.
The range-guard tests below reach the same three by putting the overflow into the first conv, the
second conv of a residual net and the second conv of a net without residual."""
import numpy as np
import pytest

V7 = 0xa04            # the library default 0x204 | 0x800: conv3x3_v7 takes 15x15 below 1024 boards too
OLD_EPILOGUE = 0x8000  # the row-streamed loop ends in the shared tile epilogue
OLD_TAIL = 0x4000     # the row-streamed loop with the unpeeled tile tail
PER_TAP = 0x2000      # conv3x3_v7's per-tap main loop
V6 = 0x100            # conv3x3_v6


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
    (128, 1, 1, 1, 1),        # four chunks, one channel half (n0 == 0 only)
    (256, 2, 3, 3, 1),        # two channel halves; conv2's output is the next block's residual
    (384, 1, 2, 2, 1),        # three channel halves, twelve chunks
    (256, 1, 16, 5, 1),       # blocks past the device-side board limit
    (128, 1, 3, 3, 0),        # no residual: Rhi null on both convs, the remainder plane still written
]
ARMS = (("v6", V7 | V6), ("per-tap", V7 | PER_TAP), ("old-tail", V7 | OLD_TAIL), ("shared", V7 | OLD_EPILOGUE), ("lean", V7))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_gpu_v7_lean_epilogue_bitwise_equals_every_other_arm(engine, case, mode):
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
    net.load_weights(net_oracle.init_blob(desc, seed=47))
    x = (np.random.default_rng(11 * ch + B).random((B, 11, 15, 15)) < 0.25).astype(np.float32)
    assert len({x[b].tobytes() for b in range(B)}) == B       # every board its own input
    outs = {}
    try:
        for name, f in ARMS:
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


def _guard_net(desc, conv, tap_kx):
    """A 128-channel, 1-block net whose trunk is transparent but for one weight: the input conv copies
    256 x input plane 0 into channel 0 (centre tap), every BN is the identity (up to eps), and trunk
    conv `conv` (0: the block's first, 1: its second; the other one passes channel 0 through its centre
    tap) multiplies channel 0 by 512 into output channel 5 through tap (ky 1, kx tap_kx) alone.  An
    input of 1 at pixel (y, x) so gives 131072 > 65504 at output pixel (y, x + 1 - tap_kx) and nothing
    of note anywhere else."""
    import net_oracle
    blob = net_oracle.init_blob(desc, seed=5)
    off = 0
    for name, shape, kind, _ in net_oracle.param_shapes(desc):
        n = int(np.prod(shape))
        v = blob[off:off + n].reshape(shape)
        trunk = name.startswith(("input_", "blocks."))
        if trunk and kind == 0:
            v[...] = 0.0
            if name == "input_conv.weight":
                v[0, 0, 1, 1] = 256.0
            elif name == f"blocks.0.{3 * conv}.weight":
                v[5, 0, 1, tap_kx] = 512.0
            else:
                v[0, 0, 1, 1] = 1.0
        elif trunk:
            v[...] = 1.0 if kind in (2, 5) else 0.0      # BN weight and variance 1, bias and mean 0
        off += n
    return blob


GUARD = [  # overflowing trunk conv (0 first, 1 second), NetDesc residual flag: one per compiled copy of the lean epilogue
    (0, 1),     # (no residual, no remainder)
    (1, 1),     # (residual, remainder)
    (1, 0),     # (no residual, remainder)
]


@pytest.mark.gpu
@pytest.mark.parametrize("conv,residual", GUARD)
def test_gpu_v7_lean_epilogue_fp16_range_guard(engine, conv, residual):
    """The fp16 range guard under the lean epilogue and the shared one (0x8000) alike, on the smallest
    net of test_gpu_trained_scale.py::test_gpu_fp16_overflow_fails_loudly's kind (conv3x3_v7 at 15x15):
      * one live pixel of one board of three overflows (input at (7, 13), tap kx 0 -> output (7, 14),
        the last live column): the forward fails with AZ_ERR_RANGE;
      * the large value can arise only in the dead 16th grid column: input at (7, 14) with tap kx 0
        lands at x = 15, input at (7, 0) with tap kx 2 at x = -1, the same grid column of the row
        above.  No live output exceeds 256, and the forward must run, in both arms alike."""
    import az_amd
    from az_amd import _lib
    desc = az_amd.NetDesc(15, 11, 128, 1, 225, 32, 8, 256, residual, 0, az_amd.AZ_PREC_FP16, 3)
    inputs = {  # name -> (tap kx, input pixel (y, x) of board 1, overflow expected)
        "live": (0, (7, 13), True),
        "dead-left": (0, (7, 14), False),
        "dead-right": (2, (7, 0), False),
    }
    seen = {}
    try:
        for name, (kx, (y, xx), ovf) in inputs.items():
            net = az_amd.HipNeuralNetwork(engine, desc)
            net.load_weights(_guard_net(desc, conv, kx))
            x = np.zeros((3, 11, 15, 15), np.float32)
            x[1, 0, y, xx] = 1.0
            for arm, f in (("shared", V7 | OLD_EPILOGUE), ("lean", V7)):
                _flags(f)
                assert net.trunk_kernel() == "conv3x3_v7<2, 15, SLIM>", net.trunk_kernel()
                try:
                    lo, v = net.forward(x)
                    assert np.isfinite(lo).all() and np.isfinite(v).all()
                    seen[name, arm] = "ran"
                except az_amd.AzError as e:
                    assert e.code == _lib.AZ_ERR_RANGE and "fp16 activation overflow" in str(e), e
                    seen[name, arm] = "range"
            net.close()
            print(f"conv {conv} residual {residual} {name}: lean {seen[name, 'lean']}, shared {seen[name, 'shared']}")
            assert seen[name, "lean"] == seen[name, "shared"], name      # the two arms behave alike
            assert seen[name, "lean"] == ("range" if ovf else "ran"), name
    finally:
        _flags(0x204)
