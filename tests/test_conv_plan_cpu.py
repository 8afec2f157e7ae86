"""Every trunk conv launch on the CPU (csrc/conv_plan.h compiled for the host).

conv_plan_g8 / conv_plan_nhwc16 / conv_plan_x3 (shape, mode, conv flags) decide the kernel, geometry,
tile rows, ring, variant and grid of one launch; the launchers execute that plan and az_net_trunk_kernel
prints conv_plan_name of the same plan.  Here the header is compiled with g++ and read through ctypes
(tests/native/conv_plan_host.cpp): against the labels the launchers' own name functions gave at the
last commit that had them (tests/golden/conv_plan_names.txt.gz, gen_conv_plan_golden.py), and for the
invariants of the launch arithmetic over the same grid.  That the label is the kernel that runs, and
that the grid is right, is for the bitwise GPU suites (test_gpu_conv_v7*.py, test_gpu_poison.py,
test_gpu_net.py::test_gpu_trunk_kernel_name)."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "conv_plan_host.cpp")
GOLDEN = os.path.join(HERE, "golden", "conv_plan_names.txt.gz")
G8, NHWC16, X3 = 0, 1, 2
IN = ["family", "flags", "H", "C", "N", "B", "mode", "opt"]
OUT = ["kernel", "mode", "pt", "board", "geo", "tm", "ring", "bm", "bn", "bnt", "sched", "boards", "nt", "var", "stagger",
       "rows", "cols", "grid", "block", "name_status"]
I = {n: i for i, n in enumerate(IN)}
O = {n: i for i, n in enumerate(OUT)}
KERNEL = ["none", "bf16", "v3", "v4", "v5", "v6", "v7", "v7x3", "v9x3"]
K = {n: i for i, n in enumerate(KERNEL)}
PAD, SLIM, DENSE = 0, 1, 2
CF, CLO, CQ, RQ, RHI, RLO, NO_RELU, SHORT_TAIL = 1, 2, 4, 8, 16, 32, 64, 128
# the literal values of the conv flag bits (az_diag_set_conv_flags; the external interface), in the
# order of conv_plan.h's table, then the default set
FLAG_VALUES = [0x4, 0x8, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000, 0x70000, 0x80000, 0x400000, 0x08000000,
               0x10000000, 0x20000000, 0x40000000, 0x204]
REMOVED_BITS = 0x100000 | 0x4000000     # two options nothing set, removed with this table: they select nothing


class Lib:
    def __init__(self, outdir):
        out = os.path.join(str(outdir), "libconvplan.so")
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", out], check=True)
        self.lib = ctypes.CDLL(out)
        self.lib.cp_plan_many.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        self.lib.cp_flags.argtypes = [ctypes.c_void_p]

    def many(self, rows):
        """([n][len(OUT)] int32, the n labels) for rows [n][len(IN)]."""
        rows = np.ascontiguousarray(rows, np.int32)
        n = len(rows)
        assert rows.shape == (n, len(IN))
        out = np.full((n, len(OUT)), -77, np.int32)
        names = np.zeros((n, 64), np.uint8)
        self.lib.cp_plan_many(rows.ctypes.data, n, out.ctypes.data, names.ctypes.data)
        return out, [bytes(r).split(b"\0", 1)[0].decode() for r in names]

    def one(self, family, flags, H, C, N, B, mode, opt=0):
        out, names = self.many([[family, flags, H, C, N, B, mode, opt]])
        return dict(zip(OUT, out[0].tolist())), names[0]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return Lib(tmp_path_factory.mktemp("convplan"))


@pytest.fixture(scope="module")
def grid(lib):
    """The fixture's rows, one per recorded label: (rows [n][len(IN)], recorded labels, plans, labels)."""
    rows, want = [], []
    with gzip.open(GOLDEN, "rt") as f:
        for line in f:
            key, *labels = line.rstrip("\n").split("|")
            fl, H, C, N, B = (int(x, 0) for x in key.split())
            cols = [(G8, 1), (G8, 2), (NHWC16, 0), (NHWC16, 1), (NHWC16, 2), (X3, 1), (X3, 2)]
            assert len(labels) == len(cols)
            for (family, mode), label in zip(cols, labels):
                if label != "-":
                    rows.append([family, fl, H, C, N, B, mode, 0])
                    want.append(label)
    rows = np.array(rows, np.int32)
    out, names = lib.many(rows)
    return rows, want, out, names


def test_labels_are_the_recorded_ones(grid):
    rows, want, out, names = grid
    assert len(want) == 116250 + 24 and len(set(want)) > 60
    bad = [i for i, (a, b) in enumerate(zip(names, want)) if a != b]
    assert not bad, [(rows[i].tolist(), names[i], want[i]) for i in bad[:5]]
    # an unsupported shape is "none" exactly where it was, and "none" is CONV_NONE with no label
    none = np.array([w == "none" for w in want])
    assert none.sum() > 10000
    assert np.array_equal(out[:, O["kernel"]] == K["none"], none) and np.array_equal(out[:, O["name_status"]] != 0, none)
    assert (out != -77).all()
    # every kernel, geometry, tile and ring the launchers instantiate appears
    assert set(out[:, O["kernel"]].tolist()) == set(range(len(KERNEL)))
    v7 = out[out[:, O["kernel"]] == K["v7"]]
    assert {(g, t, r) for g, t, r in v7[:, [O["geo"], O["tm"], O["ring"]]].tolist()} == {
        (PAD, 256, 4), (SLIM, 256, 4), (DENSE, 256, 4), (DENSE, 192, 4), (DENSE, 128, 4), (DENSE, 128, 3), (DENSE, 64, 4),
        (DENSE, 64, 3)}
    assert set(out[out[:, O["kernel"]] == K["v9x3"], O["var"]].tolist()) == {0, 1, 2, 3}


def test_benchmark_labels(lib):
    assert lib.one(G8, 0x204, 15, 256, 256, 2048, 2)[1] == "conv3x3_v7<2, 15, SLIM>"            # C3
    assert lib.one(G8, 0x204, 15, 16, 256, 2048, 2)[1] == "conv3x3_v5<2, 8>"                    # its input conv
    assert lib.one(G8, 0x204, 15, 256, 256, 256, 2)[1] == "conv3x3_v6<2, 15>"
    assert lib.one(G8, 0x204, 19, 256, 256, 2048, 2)[1] == "conv3x3_v6<2, 19, DENSE>"           # C4
    assert lib.one(G8, 0x204, 19, 256, 256, 256, 2)[1] == "conv3x3_v7<2, 19, DENSE, 128, 3>"    # its 8-GPU shard
    assert lib.one(X3, 0x204, 15, 256, 256, 2048, 2)[1] == "conv3x3_v9x3<15, SLIM, f16>"
    assert lib.one(X3, 0x204, 15, 128, 128, 2048, 1)[1] == "conv3x3_v7x3<15, SLIM>"
    p, name = lib.one(NHWC16, 0x204, 15, 64, 64, 256, 0)                                        # C2 bf16x3: one board per block
    assert name == "conv3x3_v4<0, 64>" and (p["boards"], p["nt"], p["sched"], p["grid"]) == (1, 512, 1, 256)
    p, name = lib.one(NHWC16, 0x204, 15, 64, 64, 512, 0)
    assert name == "conv3x3_v4<0, 64>" and (p["boards"], p["nt"], p["sched"], p["grid"]) == (1, 512, 1, 512)
    p, name = lib.one(NHWC16, 0x204, 15, 64, 64, 513, 0)
    assert name == "conv3x3_v4<0, 64>" and (p["boards"], p["nt"], p["sched"], p["grid"]) == (2, 512, 0, 257)


def test_grids_and_variants_the_labels_do_not_carry(lib):
    """Worked by hand from the launchers' arithmetic as it was: tiles rounded up to whole groups of 8,
    times the 128-channel halves (v5 / v6 / v7 / v7x3); v9x3 one block per tile and 256 channels."""
    def grid(*a):
        return lib.one(*a)[0]["grid"]
    assert grid(G8, 0x200, 15, 256, 128, 16, 2) == 8 and grid(G8, 0x200, 15, 256, 256, 17, 2) == 32      # v5: pairs of boards
    assert grid(G8, 0x204, 15, 256, 128, 16, 2) == 8 and grid(G8, 0x204, 15, 256, 256, 17, 2) == 32      # v6, padded 15x15
    assert grid(G8, 0x204, 19, 256, 256, 2048, 2) == 2896           # v6 DENSE: 739328 pixels / 512 = 1444 -> 1448 tiles
    assert grid(G8, 0x204, 15, 256, 256, 2048, 2) == 4096           # v7 SLIM: a board per tile
    assert grid(G8, 0x204, 19, 256, 256, 256, 2) == 1456            # v7 DENSE 128-row: 92416 / 128 = 722 -> 728
    assert grid(G8, 0xa0c, 15, 256, 256, 37, 2) == 272              # v7 DENSE 64-row at 15x15: 8325 / 64 = 131 -> 136
    assert grid(X3, 0x10000204, 9, 256, 256, 100, 1) == 64          # v7x3 DENSE: 8100 / 256 = 32 tiles
    assert grid(X3, 0x204, 9, 256, 256, 100, 1) == 32 and grid(X3, 0x204, 15, 256, 256, 100, 2) == 100   # v9x3
    assert grid(NHWC16, 0x204, 15, 64, 128, 5, 2) == 3 and grid(NHWC16, 0x204, 9, 64, 256, 100, 1) == 64  # v4, v3 128 x 256
    assert grid(NHWC16, 0x204, 9, 64, 64, 100, 0) == 32 and grid(NHWC16, 0x204, 9, 16, 192, 100, 0) == 128  # v3 256 x 64, bf16
    for fl, var in ((0x204, 3), (0x20000204, 2), (0x40000204, 1), (0x60000204, 0)):
        assert lib.one(X3, fl, 15, 256, 256, 64, 1)[0]["var"] == var and lib.one(X3, fl, 15, 256, 256, 64, 2)[0]["var"] == 3


def test_what_a_layer_carries_decides_too(lib):
    """The optional outputs and residuals of a launch: conv3x3_v7 wants a ReLU and no fp32 / lo output,
    conv3x3_v6 / v5 a ReLU (v6) and the tail behind all of the activations; the x3 kernels a whole residual."""
    def g8(opt, B=2048, H=15):
        return lib.one(G8, 0x204, H, 256, 256, B, 2, opt)[1]
    assert g8(0) == g8(CQ | RQ | RHI) == "conv3x3_v7<2, 15, SLIM>"
    assert g8(CF) == g8(CLO) == "conv3x3_v6<2, 15>"
    assert g8(NO_RELU) == g8(SHORT_TAIL, B=256) == g8(CF | SHORT_TAIL) == "none"
    assert g8(NO_RELU, H=19) == "none"
    assert lib.one(G8, 0x200, 15, 256, 256, 2048, 2, NO_RELU)[1] == "conv3x3_v5<2, 8>"
    def x3(opt):
        return lib.one(X3, 0x204, 15, 256, 256, 64, 1, opt)[1]
    assert x3(0) == x3(RHI | RLO) == x3(CLO) == "conv3x3_v9x3<15, SLIM>"
    assert {x3(o) for o in (CF, CQ, RQ, RHI, RLO, NO_RELU, SHORT_TAIL)} == {"none"}
    # a mode a family has no kernel for is refused, not rounded to a neighbour
    assert lib.one(G8, 0x204, 15, 256, 256, 2048, 0)[1] == "none" and lib.one(NHWC16, 0x204, 15, 64, 64, 4, 3)[1] == "none"
    assert lib.one(NHWC16, 0x204, 9, 64, 64, 4, 2)[1] == "none"             # fp16 operands: conv3x3_v4 only


def test_launch_invariants(grid):
    rows, want, out, names = grid
    ok = out[:, O["kernel"]] != K["none"]
    r, o = rows[ok].astype(np.int64), out[ok].astype(np.int64)
    col = lambda n: o[:, O[n]]
    M = r[:, I["B"]] * r[:, I["H"]] ** 2
    kern = col("kernel")
    # the grid covers M: whole columns of blocks, each block one tile of rows
    assert (col("cols") >= 1).all() and (col("grid") % col("cols") == 0).all()
    assert (col("grid") // col("cols") * col("rows") >= M).all()
    assert (col("grid") >= 1).all() and np.isin(col("block"), [256, 512]).all()
    # the XCD-aware mapping of v5 / v6 / v7 / v7x3: whole groups of 8 tiles per 128-channel half
    xcd = np.isin(kern, [K["v5"], K["v6"], K["v7"], K["v7x3"]])
    assert xcd.sum() > 10000 and (col("grid")[xcd] % (8 * (r[xcd, I["N"]] // 128)) == 0).all()
    # tiles and rings the kernels have
    t7 = np.isin(kern, [K["v7"], K["v7x3"], K["v9x3"]])
    assert np.isin(col("tm")[t7], [64, 128, 192, 256]).all()
    v7 = kern == K["v7"]
    assert np.isin(col("ring")[v7], [3, 4]).all()
    assert (col("tm")[v7 & (col("ring") == 3)] <= 128).all() and (col("ring")[v7 & (col("tm") == 192)] == 4).all()
    assert (col("tm")[t7 & (col("geo") != DENSE)] == 256).all() and (col("tm")[t7 & ~v7] == 256).all()
    assert (col("board") == r[:, I["H"]])[np.isin(kern, [K["v6"], K["v7"], K["v7x3"], K["v9x3"]])].all()
    # 15x15 alone has the padded and SLIM tiles; the x3 kernels one tile per board
    assert (r[np.isin(kern, [K["v5"], K["v4"]]), I["H"]] == 15).all()
    assert (r[(col("geo") != DENSE) & (t7 | (kern == K["v6"])), I["H"]] == 15).all()
    x3 = np.isin(kern, [K["v7x3"], K["v9x3"]])
    assert (col("geo")[x3] == np.where(r[x3, I["H"]] == 15, SLIM, DENSE)).all()
    # the stagger: v9x3 launches of at least 1024 blocks, and all of those
    st = col("stagger") == 1
    assert st.any() and np.array_equal(st, (kern == K["v9x3"]) & (col("grid") >= 1024))
    # fp16 pieces run v9x3's default variant only
    assert (col("var")[(kern == K["v9x3"]) & (col("pt") == 2)] == 3).all()


def test_plan_is_a_function_of_its_arguments(lib, grid):
    rows, want, out, names = grid
    sel = np.random.default_rng(0).permutation(len(rows))[:30000]
    again, names2 = lib.many(rows[sel])                 # another order, other neighbours, fresh buffers
    assert np.array_equal(again, out[sel]) and names2 == [names[i] for i in sel]


def test_flag_constants_and_removed_bits(lib, grid):
    f = np.zeros(32, np.int32)
    n = lib.lib.cp_flags(f.ctypes.data)
    assert f[:n].tolist() == FLAG_VALUES
    bits = FLAG_VALUES[:-1]
    assert sum(bits) == np.bitwise_or.reduce(bits) and not sum(bits) & REMOVED_BITS      # disjoint, and none of the removed
    rows, want, out, names = grid
    sel = np.random.default_rng(1).permutation(len(rows))[:30000]
    more = rows[sel].copy()
    more[:, I["flags"]] |= REMOVED_BITS
    again, names2 = lib.many(more)
    assert np.array_equal(again, out[sel]) and names2 == [names[i] for i in sel]


def test_standalone_program(tmp_path):
    """The -DCONV_PLAN_MAIN program (the one a sanitizer build runs) builds and passes."""
    exe = str(tmp_path / "conv_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-DCONV_PLAN_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("conv_plan ok"), (r.stdout, r.stderr)
