#!/usr/bin/env python3
"""Phase timeline of conv3x3_v7's row-streamed launches (diagnostic build: make EXTRA=-DAZ_V7_STAMPS
OUT=build_stamps7, loaded with AZ_DIAG_HIP_LIB).  Wave 0 of every block stamps s_memrealtime (100 MHz)
at its start, after the prologue barrier, at the main loop's end, when the first residual operands
are in registers, after the last store issues and after all stores complete; HW_ID / XCC_ID name the
CU.  For one 1st conv and one 2nd conv of the C3 trunk, under each --flags set, prints per block the
main-loop and epilogue times, how the epilogue starts of a round (the r-th pair of blocks of every CU)
spread over the chip, how many epilogues run at once, and the phase between the two blocks that
share a CU."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alphazero-multi-game_amd"))
import az_amd  # noqa: E402
from az_amd import _lib  # noqa: E402

NST = 6


def report(tag, t, hw):
    t0 = t[:, 0].min()
    ph = np.diff(t, axis=1) / 100.0                      # prologue, main, residual wait, join + stores, drain (us)
    epi = (t[:, 5] - t[:, 2]) / 100.0
    cu = (hw[:, 1].astype(np.int64) << 16) | ((hw[:, 0] >> 8) & 0xFF)
    ucu = np.unique(cu)
    rnd = np.zeros(len(t), np.int64)
    phase, resident = [], []
    for c in ucu:
        idx = np.where(cu == c)[0]
        o = idx[np.argsort(t[idx, 0])]
        rnd[o] = np.arange(len(o)) // 2
        for a, b in zip(o[0::2], o[1::2]):               # the two blocks of a round on this CU
            phase.append(abs(int(t[a, 2]) - int(t[b, 2])) / 100.0)
            resident.append(t[b, 0] < t[a, 5])           # the second started before the first ended
    ev = np.concatenate([np.stack([t[:, 2], np.ones(len(t), np.int64)], 1), np.stack([t[:, 5], -np.ones(len(t), np.int64)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
    conc = np.cumsum(ev[:, 1])
    dt = np.diff(ev[:, 0])
    span = (t[:, 5].max() - t0) / 100.0
    print(f"{tag}: span {span:.1f} us, {len(t)} blocks on {len(ucu)} CUs; per block (us): prologue {ph[:, 0].mean():.2f}, "
          f"main loop {ph[:, 1].mean():.2f} (min {ph[:, 1].min():.1f} median {np.median(ph[:, 1]):.1f} max {ph[:, 1].max():.1f}), "
          f"residual wait {ph[:, 2].mean():.2f}, join + stores {ph[:, 3].mean():.2f}, drain {ph[:, 4].mean():.2f}; "
          f"epilogue {epi.mean():.2f} (median {np.median(epi):.2f}, p90 {np.percentile(epi, 90):.2f})")
    print(f"   epilogues at once: time-average {(conc[:-1] * dt).sum() / max(dt.sum(), 1):.0f}, peak {conc.max()}; "
          f"co-resident pairs {np.mean(resident):.3f} of {len(resident)}; phase between the two blocks of a CU "
          f"(|difference of loop ends|): median {np.median(phase):.1f} us, p10 {np.percentile(phase, 10):.1f}, "
          f"p90 {np.percentile(phase, 90):.1f}")
    for r in range(int(rnd.max()) + 1):
        s = (t[rnd == r, 2] - t0) / 100.0
        e = epi[rnd == r]
        print(f"   round {r}: {len(s)} blocks, epilogue starts at {np.median(s):.1f} us (p10 {np.percentile(s, 10):.1f}, p90 "
              f"{np.percentile(s, 90):.1f}, std {s.std():.1f}), epilogue {e.mean():.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--precision", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--block", type=int, default=10, help="residual block whose two convs are stamped")
    ap.add_argument("--flags", default="0x204", help="comma list of conv flag sets (0x4204: the unpeeled tile tail)")
    a = ap.parse_args()
    L = _lib.lib()
    f = L.az_diag_v7_stamps
    f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    if f(-1, None, None, 0) != 0:
        raise SystemExit("not a stamp build (make EXTRA=-DAZ_V7_STAMPS OUT=build_stamps7; AZ_DIAG_HIP_LIB)")
    eng = az_amd.Engine(0)
    prec = {"fp16": az_amd.AZ_PREC_FP16, "bf16": az_amd.AZ_PREC_BF16}[a.precision]
    net = az_amd.HipNeuralNetwork(eng, az_amd.NetDesc(15, 11, 256, 20, 225, 32, 8, 256, 1, 0, prec, a.batch))
    net.init_random(1234)
    x = (np.random.default_rng(0).random((a.batch, 11, 15, 15)) < 0.2).astype(np.float32)
    net.forward(x)
    grid = (a.batch + 7) // 8 * 8 * 2
    st = np.zeros((grid, NST), np.uint64)
    hw = np.zeros((grid, 2), np.uint32)
    for fl in [int(s, 0) for s in a.flags.split(",")]:
        L.az_diag_set_conv_flags(fl)
        net.forward(x)
        for name, launch in (("conv1", 2 * a.block), ("conv2", 2 * a.block + 1)):
            for rep in range(2):
                f(launch, None, None, 0)
                net.forward(x)
                assert f(-2, st.ctypes.data, hw.ctypes.data, grid) == 0
                t = st.astype(np.int64)
                live = t[:, 0] > 0
                assert live.sum() == a.batch * 2 and (t[live] > 0).all(), "missing stamps"
                report(f"flags {fl:#x} {name} (launch {launch}) rep {rep}", t[live], hw[live])
    f(-1, None, None, 0)


if __name__ == "__main__":
    main()
