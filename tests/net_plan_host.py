"""csrc/net_plan.h compiled for the host (tests/native/net_plan_host.cpp) behind ctypes: the plan of a
network description without a GPU.  Shared by test_net_plan_cpu.py and test_gpu_net_plan.py."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "net_plan_host.cpp")
F32, BF16X3, BF16, FP16, F16X3 = 0, 1, 2, 3, 4
PRECS = [F32, BF16X3, BF16, FP16, F16X3]
FLAGS = 0x204                    # the library's default conv flags
LDS = 160 * 1024                 # gfx950's LDS per workgroup
IN = ["gemm", "small", "g8"]
TRUNK = ["GEMM_F32", "SMALL", "G8", "G8X3", "NHWC16", "RW_F32", "RW_V4_FP16", "RW_V4_X3"]
HEADS = ["generic", "f32", "x3-bf16", "x3-fp16"]
FIELDS = ["input", "in32", "trunk", "tail_fused", "head_conv_fused", "heads", "status", "no_forward", "msg_len", "packs"]
PACK_SM, PACK_IN16, PACK_IN32, PACK_TRUNK16 = 1, 2, 4, 8


def desc(board, planes, channels, blocks, max_batch, head_channels=32, pool=8, conv_bias=0, precision=0):
    """The twelve ints of az_net_desc (az_amd.NetDesc's field order)."""
    return [board, planes, channels, blocks, board * board, head_channels, pool, 256, 1, conv_bias, precision, max_batch]


class PlanLib:
    def __init__(self, outdir, extra=()):
        out = os.path.join(str(outdir), "libnetplan.so")
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", *extra, SRC, "-o", out], check=True)
        self.lib = ctypes.CDLL(out)
        self.lib.np_plan_line.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                                          ctypes.c_char_p, ctypes.c_int]
        self.lib.np_plan_many.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_void_p]
        self.lib.np_cin_pad.argtypes = [ctypes.c_void_p, ctypes.c_int]

    def line(self, d, rw, precision, flags=FLAGS, lds=LDS):
        """(status, the line az_diag_net_plan writes) for description d (twelve ints, or an az_amd.NetDesc)."""
        if not isinstance(d, (list, tuple)):
            d = [getattr(d, n) for n, _ in d._fields_]
        a = np.array(d, np.int32)
        buf = ctypes.create_string_buffer(320)
        st = self.lib.np_plan_line(a.ctypes.data, int(rw), precision, flags, lds, buf, 320)
        return st, buf.value.decode()

    def many(self, descs, rw, precision, flags=FLAGS, lds=LDS):
        """[n][len(FIELDS)] int32 for n descriptions ([n][12]), rw [n] and precision [n]."""
        descs = np.ascontiguousarray(descs, np.int32)
        rw = np.ascontiguousarray(rw, np.int32)
        precision = np.ascontiguousarray(precision, np.int32)
        n = len(rw)
        assert descs.shape == (n, 12) and precision.shape == (n,)
        out = np.full((n, len(FIELDS)), -77, np.int32)
        self.lib.np_plan_many(descs.ctypes.data, rw.ctypes.data, precision.ctypes.data, n, flags, lds, out.ctypes.data)
        return out
