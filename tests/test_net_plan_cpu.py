"""The forward's route table on the CPU (csrc/net_plan.h compiled for the host).

net_plan(shape, precision, conv flags, LDS limit) is the one place that decides how a network runs:
the input stage, the trunk kernel family, the tail, the head FC variant and the refusals of
az_net_create* / az_net_set_precision; net_packs(shape) names the weight sets a load builds.  Here
the header is compiled with g++ and read through ctypes: a named table of the shapes the suite and
the benchmark run (expected values from the dispatch as it was before the table existed, confirmed on
the device by tests/test_gpu_net_plan.py), the refusals against test_gpu_net_lifecycle.py's ACCEPTED
table, and an exhaustive grid for the invariants -- above all the lifecycle contract: every weight set
a plan reads is one the load packs, for every precision the shape accepts."""
import itertools
import subprocess

import numpy as np
import pytest

from net_plan_host import (BF16, BF16X3, F16X3, F32, FIELDS, FLAGS, FP16, HEADS, IN, LDS, PACK_IN16, PACK_IN32, PACK_SM,
                           PACK_TRUNK16, PRECS, SRC, TRUNK, PlanLib, desc)

COL = {n: i for i, n in enumerate(FIELDS)}
SMALL_MAX_BLOCKS = 15            # AZ_SMALLNET_MAX_BLOCKS


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return PlanLib(tmp_path_factory.mktemp("netplan"))


def route(plans, d, rw, prec, flags=FLAGS, lds=LDS):
    """'refused', or 'input/TRUNK' with the g8 input layer in brackets."""
    r = plans.many([d], [rw], [prec], flags, lds)[0]
    if r[COL["status"]]:
        return "refused"
    i = IN[r[COL["input"]]]
    if i == "g8":
        i += "(in32)" if r[COL["in32"]] else "(in)"
    return f"{i}/{TRUNK[r[COL['trunk']]]}"


# (board, planes, channels, blocks, conv_bias): f32, bf16x3, bf16, fp16, f16x3
TABLE = {
    "small":   ((15, 11, 64, 2, 0), ["gemm/GEMM_F32", "small/SMALL", "gemm/NHWC16", "small/SMALL", "small/SMALL"]),
    "g8-15":   ((15, 11, 128, 1, 0), ["gemm/GEMM_F32", "gemm/G8X3", "g8(in)/G8", "g8(in)/G8", "gemm/G8X3"]),
    "g8-9":    ((9, 11, 128, 1, 0), ["gemm/GEMM_F32", "gemm/G8X3", "g8(in32)/G8", "g8(in32)/G8", "gemm/G8X3"]),
    "nhwc":    ((15, 11, 32, 1, 0), ["gemm/GEMM_F32", "gemm/NHWC16", "gemm/NHWC16", "refused", "refused"]),
    "f32only": ((8, 11, 16, 1, 1), ["gemm/GEMM_F32", "refused", "refused", "refused", "refused"]),
}


@pytest.mark.parametrize("name", TABLE)
@pytest.mark.parametrize("cap", [4, 512])
def test_named_table(plans, name, cap):
    (board, planes, ch, blocks, bias), want = TABLE[name]
    d = desc(board, planes, ch, blocks, cap, conv_bias=bias)
    assert [route(plans, d, 0, p) for p in [F32, BF16X3, BF16, FP16, F16X3]] == want
    rows = plans.many([d] * 5, [0] * 5, PRECS)
    for p, r in zip(PRECS, rows):
        if r[COL["status"]]:
            continue
        # the tail is fused on every g8 row with heads 32 / pool 8, nowhere else
        assert bool(r[COL["tail_fused"]]) == (TRUNK[r[COL["trunk"]]] in ("G8", "G8X3")), (name, p)
        heads = "f32" if cap < 512 or p in (F32, BF16X3) else "x3-fp16" if p == F16X3 else "x3-bf16"
        assert HEADS[r[COL["heads"]]] == heads, (name, p, cap)
        assert not r[COL["no_forward"]]


def test_benchmark_configs(plans):
    assert route(plans, desc(15, 11, 256, 20, 2048), 0, FP16) == "g8(in)/G8"            # C3
    assert route(plans, desc(19, 8, 256, 20, 2048), 0, FP16) == "g8(in32)/G8"           # C4
    c5 = desc(8, 111, 256, 20, 2048)
    assert plans.lib.np_cin_pad(np.array(c5, np.int32).ctypes.data, 0) == 128
    assert route(plans, c5, 0, FP16) == "g8(in)/G8"                                     # C5


def test_randwire(plans):
    def rw(prec, cap):
        return route(plans, desc(15, 11, 64, 2, cap), 1, prec)
    assert rw(F32, 4) == "gemm/RW_F32"
    assert rw(FP16, 4) == "gemm/RW_V4_FP16"
    assert rw(BF16X3, 128) == "gemm/RW_V4_X3" and rw(BF16X3, 127) == "gemm/RW_F32"
    assert rw(BF16, 128) == "refused" and rw(F16X3, 128) == "refused"
    # off 15x15, or with channels % 64 != 0: fp32 only
    for d in (desc(9, 11, 64, 2, 128), desc(15, 11, 32, 2, 128)):
        assert [route(plans, d, 1, p) for p in PRECS] == ["gemm/RW_F32"] + ["refused"] * 4


def test_flags_change_only_tail_and_heads(plans):
    shapes = [desc(*TABLE[n][0][:4], cap, conv_bias=TABLE[n][0][4]) for n in TABLE for cap in (4, 512)]
    shapes += [desc(19, 8, 256, 20, 2048), desc(15, 11, 64, 2, 512)]
    rows = [(d, rw, p) for d in shapes for rw in (0, 1) for p in PRECS]
    args = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    base = plans.many(*args)
    keep_tail = plans.many(*args, flags=FLAGS | 0x400000)
    keep_f32 = plans.many(*args, flags=FLAGS | 0x08000000)
    other = [COL[c] for c in FIELDS if c not in ("tail_fused", "head_conv_fused", "heads")]
    assert np.array_equal(base[:, other], keep_tail[:, other]) and np.array_equal(base[:, other], keep_f32[:, other])
    assert np.array_equal(base[:, COL["heads"]], keep_tail[:, COL["heads"]])
    assert not keep_tail[:, COL["tail_fused"]].any() and base[:, COL["tail_fused"]].any()
    assert np.array_equal(base[:, [COL["tail_fused"], COL["head_conv_fused"]]],
                          keep_f32[:, [COL["tail_fused"], COL["head_conv_fused"]]])
    x3 = np.isin(base[:, COL["heads"]], [HEADS.index("x3-bf16"), HEADS.index("x3-fp16")])
    assert x3.any() and (keep_f32[x3, COL["heads"]] == HEADS.index("f32")).all()
    assert np.array_equal(base[~x3, COL["heads"]], keep_f32[~x3, COL["heads"]])
    # a 64 KB part cannot hold the fused tail's LDS at 19x19
    c4 = desc(19, 8, 256, 20, 2048)
    assert plans.many([c4], [0], [FP16])[0][COL["tail_fused"]] == 1
    assert plans.many([c4], [0], [FP16], lds=64 * 1024)[0][COL["tail_fused"]] == 0


def test_refusals_are_the_lifecycle_suites_accepted_table(plans):
    import test_gpu_net_lifecycle as lc
    for name, (bs, ci, ch, blocks, B, bias) in lc.SHAPES.items():
        d = desc(bs, ci, ch, blocks, B, conv_bias=bias)
        accepted = []
        for p in lc.PRECS:
            st, line = plans.line(d, 0, p)
            if st == 0:
                accepted.append(p)
            else:
                assert st == -1 and line.startswith("refused: ") and len(line) > len("refused: ") + 20, (name, p, line)
        assert accepted == lc.ACCEPTED[name], name
    st, line = plans.line(desc(15, 11, 64, 2, 4), 0, 7)
    assert st == -1 and line == "refused: bad precision 7"


# ---- the exhaustive grid
BOARDS = [6, 7, 8, 9, 13, 15, 19]
PLANES = [3, 11, 16, 17, 111]
CHANNELS = [16, 32, 48, 64, 128, 192, 256]
BLOCKS = [0, 1, 20, SMALL_MAX_BLOCKS + 1]
HEAD_CH = [16, 32]
POOLS = [1, 8]
CAPS = [1, 127, 128, 511, 512, 1023, 1024, 2048]


@pytest.fixture(scope="module")
def grid(plans):
    shapes = np.array([desc(b, pl, c, k, cap, head_channels=hc, pool=po) + [rw]
                       for b, pl, c, k, hc, po, cap, rw in itertools.product(BOARDS, PLANES, CHANNELS, BLOCKS, HEAD_CH, POOLS,
                                                                             CAPS, [0, 1])], np.int32)
    n = len(shapes)
    descs = np.repeat(shapes[:, :12], len(PRECS), axis=0)
    rw = np.repeat(shapes[:, 12], len(PRECS))
    prec = np.tile(np.array(PRECS, np.int32), n)
    return descs, rw, prec, plans.many(descs, rw, prec)


def test_grid_every_set_a_plan_reads_is_packed(grid):
    """The lifecycle contract as an invariant: whatever precision a shape accepts, the weight sets its
    plan reads are among those the load packs for the shape (which never depend on the precision)."""
    descs, rw, prec, out = grid
    ok = out[:, COL["status"]] == 0
    packs, inp, trunk = out[:, COL["packs"]], out[:, COL["input"]], out[:, COL["trunk"]]
    reads = np.zeros(len(out), np.int32)
    reads |= np.where(trunk == TRUNK.index("SMALL"), PACK_SM, 0)
    reads |= np.where((inp == IN.index("g8")) & (out[:, COL["in32"]] == 1), PACK_IN32, 0)
    reads |= np.where((inp == IN.index("g8")) & (out[:, COL["in32"]] == 0), PACK_IN16, 0)
    t16 = [TRUNK.index(t) for t in ("G8", "G8X3", "NHWC16", "RW_V4_FP16", "RW_V4_X3")]
    reads |= np.where(np.isin(trunk, t16), PACK_TRUNK16, 0)
    bad = ok & ((reads & ~packs) != 0)
    assert not bad.any(), (descs[bad][:5], prec[bad][:5], reads[bad][:5], packs[bad][:5])
    assert ok.sum() > 100000 and (reads[ok] != 0).sum() > 10000
    # the packs are the shape's: the same on all five precision rows of a shape
    assert (packs.reshape(-1, len(PRECS)) == packs.reshape(-1, len(PRECS))[:, :1]).all()
    # small and g8 inputs come with their trunks, and the other way round
    assert ((inp == IN.index("small")) == (trunk == TRUNK.index("SMALL"))).all()
    assert (inp[rw == 1] == IN.index("gemm")).all() and (trunk[rw == 1] >= TRUNK.index("RW_F32")).all()
    assert (trunk[rw == 0] < TRUNK.index("RW_F32")).all()


def test_grid_g8_trunk_always_has_a_g8_input_conv(grid):
    """A g8 net never needs the f32 input conv followed by a conversion to g8 (the forward has no such
    branch): with channels % 128 == 0 cin_pad is 16 or a multiple of 32; 16 is served by the net's own
    input layer at 15x15 and by the zero-padded one on the other boards, a multiple of 32 by its own."""
    descs, rw, prec, out = grid
    g8 = out[:, COL["trunk"]] == TRUNK.index("G8")
    assert g8.sum() > 1000
    lone = g8 & (out[:, COL["input"]] != IN.index("g8"))
    assert not lone.any(), descs[lone][:5]
    assert (out[~g8, COL["input"]] != IN.index("g8")).all()


def test_grid_plan_is_a_function_of_its_arguments(plans, grid):
    descs, rw, prec, out = grid
    sel = np.random.default_rng(0).permutation(len(out))[:50000]
    again = plans.many(descs[sel], rw[sel], prec[sel])          # another order, other neighbours, a fresh buffer
    assert np.array_equal(again, out[sel])
    assert (out != -77).all()
    # a refusal always carries a message, an accepted plan none
    assert ((out[:, COL["status"]] != 0) == (out[:, COL["msg_len"]] > 0)).all()
    assert np.isin(out[:, COL["status"]], [0, -1]).all()


def test_grid_entry_point_disagreements(grid):
    """The create-time check and the forward disagree in one corner of the grid, kept as it was: a plain
    net without blocks is created at AZ_PREC_F16X3 on any shape with channels % 32 == 0, and its
    forward is refused unless the shape has the fp16-piece kernels anyway."""
    descs, rw, prec, out = grid
    nf = (out[:, COL["no_forward"]] == 1) & (out[:, COL["status"]] == 0)
    assert nf.any()
    assert (prec[nf] == F16X3).all() and (descs[nf][:, 3] == 0).all() and (rw[nf] == 0).all()


def test_standalone_program(tmp_path):
    """The -DNET_PLAN_MAIN program (the one a sanitizer build runs) builds and passes."""
    exe = str(tmp_path / "net_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DNET_PLAN_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("net_plan ok"), (r.stdout, r.stderr)
