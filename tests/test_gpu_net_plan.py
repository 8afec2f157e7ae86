"""The route the library takes is the one csrc/net_plan.h gives on the CPU (tests/test_net_plan_cpu.py).

Create-only: HipNeuralNetwork.plan() (az_diag_net_plan) needs neither a load nor a forward.  For the
lifecycle suite's five shape classes at every precision they accept, and at the capacity thresholds
(rand-wire node convs 127 / 128 boards, split-operand FC heads 511 / 512), the library's line equals the
host-compiled header's for the same description, and its trunk family is the one trunk_kernel() names."""
import pytest

from net_plan_host import BF16, BF16X3, F16X3, F32, FP16, PlanLib
from test_gpu_net_lifecycle import ACCEPTED, PNAME, PRECS, SHAPES

# trunk_kernel() prefix -> the plan's trunk families
FAMILY = [("k_smallnet", {"small"}), ("conv3x3_v7x3", {"g8x3"}), ("conv3x3_v9x3", {"g8x3"}),
          ("conv3x3_v5", {"g8"}), ("conv3x3_v6", {"g8"}), ("conv3x3_v7<", {"g8"}),
          ("conv3x3_v4", {"nhwc16", "rw_v4_fp16", "rw_v4_x3"}), ("conv3x3_v3", {"nhwc16"}), ("conv3x3_bf16", {"nhwc16"}),
          ("gemm_f32", {"gemm_f32", "rw_f32"})]

# (shape class or "rw", precision, capacity): every accepted state at the class's small batch, then the thresholds
CASES = [(s, p, SHAPES[s][4]) for s in SHAPES for p in ACCEPTED[s]]
CASES += [("rw", BF16X3, 127), ("rw", BF16X3, 128), ("rw", FP16, 4), ("rw", F32, 4)]
CASES += [(s, p, cap) for s, p in (("small", FP16), ("small", F16X3), ("small", BF16X3), ("g8-9", FP16), ("g8-9", F16X3),
                                   ("g8-15", BF16)) for cap in (511, 512)]


@pytest.fixture(scope="module")
def engine():
    import az_amd
    return az_amd.Engine(0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    return PlanLib(tmp_path_factory.mktemp("netplan"))


def _create(engine, shape, prec, cap):
    import az_amd
    if shape == "rw":
        d = az_amd.randwire_net_desc(board_size=15, channels=64, blocks=1, max_batch=cap)
        d.precision = prec
        return az_amd.HipNeuralNetwork(engine, d, randwire=True)
    bs, ci, ch, blocks, _, bias = SHAPES[shape]
    return az_amd.HipNeuralNetwork(engine, az_amd.NetDesc(bs, ci, ch, blocks, bs * bs, 32, 8, 256, 1, bias, prec, cap))


def _fields(line):
    return dict(kv.split("=") for kv in line.split())


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{PNAME[c[1]]}-{c[2]}")
def test_gpu_plan_is_the_headers_and_names_the_trunk_family(engine, plans, case):
    shape, prec, cap = case
    net = _create(engine, shape, prec, cap)
    try:
        line, kernel = net.plan(), net.trunk_kernel()
        st, want = plans.line(net.desc, shape == "rw", prec)
    finally:
        net.close()
    print(f"{shape} {PNAME[prec]} cap {cap}: {line}; trunk kernel {kernel}")
    assert st == 0 and line == want
    families = [fam for prefix, fam in FAMILY if kernel.startswith(prefix)]
    assert len(families) == 1 and _fields(line)["trunk"] in families[0], (line, kernel)
    f = _fields(line)
    if shape == "rw":
        assert f["trunk"] == {F32: "rw_f32", FP16: "rw_v4_fp16", BF16X3: "rw_v4_x3" if cap >= 128 else "rw_f32"}[prec]
    heads = "f32" if cap < 512 or prec in (F32, BF16X3) else "x3-fp16" if prec == F16X3 else "x3-bf16"
    assert f["heads"] == heads


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [s for s in SHAPES if len(ACCEPTED[s]) > 2])
def test_gpu_plan_after_set_precision_is_the_fresh_nets(engine, shape):
    acc = ACCEPTED[shape]
    fresh = {}
    for p in acc:
        net = _create(engine, shape, p, SHAPES[shape][4])
        fresh[p] = (net.plan(), net.trunk_kernel())
        net.close()
    assert len(set(fresh.values())) > 1
    for i, p in enumerate(acc):
        net = _create(engine, shape, p, SHAPES[shape][4])
        try:
            for q in (acc[(i + 1) % len(acc)], acc[(i + 2) % len(acc)], p):      # two other precisions and back
                net.set_precision(q)
                assert (net.plan(), net.trunk_kernel()) == fresh[q], (shape, p, q)
            for q in PRECS:
                if q not in acc:                                                # a refused switch changes nothing
                    with pytest.raises(Exception):
                        net.set_precision(q)
                    assert (net.plan(), net.trunk_kernel()) == fresh[p]
        finally:
            net.close()
