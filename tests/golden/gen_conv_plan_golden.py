#!/usr/bin/env python3
"""Records the trunk conv labels of commit a13e64c, the last one whose launchers named their own
kernels (az_conv_g8_name / az_conv_bf16_name / az_conv_x3_name in conv_bf16.hip / conv_v7.hip), into
conv_plan_names.txt.gz -- the table tests/test_conv_plan_cpu.py holds csrc/conv_plan.h to:

    python3 tests/golden/gen_conv_plan_golden.py PARENT

PARENT: a checkout of a13e64c with alphazero-multi-game_amd/build/libaz_hip.so built.  The three name
functions are pure host code, so the program below, compiled against that checkout's csrc/net.h and
linked against its library, runs without a GPU.  It cannot be rebuilt from a later commit: those
functions are gone, which is the point of the fixture.

One line per (flags, board, C, N, boards):

    flags H C N B|g8 bf16|g8 fp16|nhwc16 bf16x3|nhwc16 bf16|nhwc16 fp16|x3 bf16 pieces|x3 fp16 pieces

"none": the family refuses the shape.  "-": not recorded -- a13e64c named a conv3x3_v4 kernel for
fp16 operands on any shape, though the forward only ever sends it the shapes conv3x3_v4 supports.
The axes are those of tests/test_conv_plan_cpu.py (FLAG_SETS: the default and every set a test or a
tool passes; batches on both sides of every threshold in the launchers), then EXTRA: batches around
the block-count thresholds of the tile choice that the common batch list does not straddle.
"""
import gzip
import os
import subprocess
import sys
import tempfile

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_plan_names.txt.gz")
FLAG_SETS = [0x204, 0x304, 0xa04, 0xe04, 0xa0c, 0x804, 0x10804, 0x20804, 0x30804, 0x40804, 0xa0804, 0xb0804, 0x20a0c,
             0x2204, 0x4204, 0x1204, 0x10000204, 0x904, 0x20000204, 0x40000204, 0x60000204, 0x200, 0x20c, 0x30204, 0xb0204]
BOARDS = [8, 9, 13, 15, 19]
CS = [16, 32, 64, 128, 256]
NS = [64, 128, 256]
BATCHES = [1, 64, 128, 256, 400, 512, 768, 1023, 1024, 2048]
# 128-row tiles from 512 blocks on, 64-row tiles below: 13x13 with one 128-channel half (382 boards),
# 8x8 with two (497 boards)
EXTRA = [(0x204, 13, 128, 128, b) for b in (381, 382)] + [(0x204, 8, 256, 256, b) for b in (496, 497)]

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "net.h"
extern "C" int az_diag_set_conv_flags(int);
int main(int argc, char** argv) {
    const int fl = (int)strtol(argv[1], nullptr, 0), H = atoi(argv[2]), one = argc > 3;
    az_diag_set_conv_flags(fl);
    for (int C : {%(cs)s}) for (int N : {%(ns)s}) for (int B : {%(bs)s}) {
        if (one) { C = atoi(argv[3]); N = atoi(argv[4]); B = atoi(argv[5]); }
        ConvBf16Args a{};
        a.H = a.W = H; a.C = C; a.N = N; a.M = B * H * H; a.rows_per_sample = H * H; a.relu = 1;
        a.a_tail = (size_t)a.M * C * 2;
        char s[7][96];
        for (int m = 1; m <= 2; ++m) if (az_conv_g8_name(a, m, s[m - 1], 96)) snprintf(s[m - 1], 96, "none");
        for (int m = 0; m <= 2; ++m) az_conv_bf16_name(a, m, s[2 + m], 96);
        if (!(H == 15 && C %% 16 == 0 && N %% 64 == 0)) snprintf(s[4], 96, "-");      // az_conv_v4_supported
        for (int pt = 1; pt <= 2; ++pt) { a.pt = pt; if (az_conv_x3_name(a, s[4 + pt], 96)) snprintf(s[4 + pt], 96, "none"); }
        printf("%%#x %%d %%d %%d %%d|%%s|%%s|%%s|%%s|%%s|%%s|%%s\n", fl, H, C, N, B, s[0], s[1], s[2], s[3], s[4], s[5], s[6]);
        if (one) return 0;
    }
    return 0;
}
"""


def main():
    parent = os.path.abspath(sys.argv[1])
    pkg = os.path.join(parent, "alphazero-multi-game_amd")
    head = subprocess.run(["git", "-C", parent, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    assert head == "a13e64c", f"{parent} is at {head!r}, not a13e64c"
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "names.cpp"), os.path.join(tmp, "names")
        with open(src, "w") as f:
            f.write(SRC % {"cs": ", ".join(map(str, CS)), "ns": ", ".join(map(str, NS)), "bs": ", ".join(map(str, BATCHES))})
        subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(pkg, "csrc"),
                        src, "-L" + os.path.join(pkg, "build"), "-laz_hip", "-Wl,-rpath," + os.path.join(pkg, "build"), "-o", exe],
                       check=True)
        for fl in FLAG_SETS:
            for h in BOARDS:
                lines += subprocess.run([exe, hex(fl), str(h)], capture_output=True, text=True, check=True).stdout.splitlines()
        for row in EXTRA:
            lines += subprocess.run([exe, hex(row[0])] + [str(x) for x in row[1:]], capture_output=True, text=True,
                                    check=True).stdout.splitlines()
    assert len(lines) == len(FLAG_SETS) * len(BOARDS) * len(CS) * len(NS) * len(BATCHES) + len(EXTRA)
    with gzip.GzipFile(OUT, "wb", mtime=0) as f:
        f.write(("\n".join(lines) + "\n").encode())
    print(f"{len(lines)} rows -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
