#!/usr/bin/env python3
"""Static figures of the trunk convs' epilogues from gfx950 assembly (no GPU): compile
csrc/conv_v7.hip with the Makefile's NETFLAGS plus `-S --cuda-device-only`, then

    python3 tools/v7_epilogue_isa.py conv_v7.s [more.s ...]

Per file: code length, VGPRs, scratch and LDS of every conv3x3_v7* / v9x3 kernel, and for the two
row-streamed kernels (conv3x3_v7<2 / 1, 15, SLIM, 256, 4>) and conv3x3_v9x3<15, SLIM, 3, 2> every run of
output stores -- one run per compiled copy of an epilogue -- with the instruction count from its
first to its last store and, inside that span, the branches, kernarg / scalar loads, 64-bit vector
multiplies and adds, exec-mask saves, constant moves and LDS reads.  Global-store runs are the shared
tile epilogue (per-tap loop: one copy per row half; row-streamed loop: the 0x4000 tail reading global
memory, then the copy reading the residual from LDS); buffer-store runs are the row-streamed path's
lean epilogue, one per (residual, remainder) combination."""
import re
import sys

ROWS = ["_Z10conv3x3_v7ILi2ELi15ELi1ELi256ELi4EEv12ConvBf16Args", "_Z10conv3x3_v7ILi1ELi15ELi1ELi256ELi4EEv12ConvBf16Args",
        "_Z12conv3x3_v9x3ILi15ELi1ELi3ELi2EEv12ConvBf16Args"]
COUNT = [("branches", r"s_cbranch|s_branch"), ("s_load", r"s_load|s_buffer_load"), ("v_mad_64", r"v_mad_u64_u32|v_mad_i64_i32"),
         ("v_lshl_add_u64", r"v_lshl_add_u64"), ("v_lshlrev_b64", r"v_lshlrev_b64"), ("saveexec", r"s_(and|or)_saveexec"),
         ("s_mov", r"s_movk_i32|s_mov_b32"), ("v_mov", r"v_mov_b32"), ("ds_read", r"ds_read"), ("scratch", r"scratch_")]


def kernels(path):
    """{name: ([instruction, ...], {figure: value})} of every kernel in an assembly file"""
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.strip()
        if line.startswith(".Lfunc_end"):
            out[name] = (body, {})
            name = None
            continue
        if s and not s.startswith((";", ".", "//")) and not s.endswith(":"):
            body.append(s)
    last = None
    for line in open(path):                                  # the figures follow each kernel as comments
        m = re.match(r"(_Z\w+):", line)
        if m:
            last = m.group(1)
        m = re.match(r"; (codeLenInByte|NumVgprs|ScratchSize|LDSByteSize)\s*[:=]\s*(\d+)", line)
        if m and last in out:
            out[last][1].setdefault(m.group(1), int(m.group(2)))
    return out


def store_runs(ins):
    """runs of output stores: [(family, [instruction index, ...])]"""
    runs, prev_off = [], -1
    for k, text in enumerate(ins):
        m = re.match(r"(buffer|global)_store_dword(x2)?\b", text)
        if not m:
            continue
        fam = m.group(1)
        off = re.search(r"offset:(0x[0-9a-f]+|\d+)", text)
        off = int(off.group(1), 0) if off else 0
        new = not runs or runs[-1][0] != fam or k - runs[-1][1][-1] > 200
        if fam == "buffer" and m.group(2):                   # a lean copy starts over at fragment row 0
            new = new or off < prev_off
            prev_off = off
        if new:
            runs.append((fam, []))
        runs[-1][1].append(k)
    return runs


def main():
    for path in sys.argv[1:]:
        ks = kernels(path)
        print(f"== {path}")
        for name in sorted(ks):
            if re.match(r"_Z\d+conv3x3_v(7|9x3)", name):
                f = ks[name][1]
                print(f"{name}: code {f.get('codeLenInByte')} B, VGPRs {f.get('NumVgprs')}, scratch {f.get('ScratchSize')} B, "
                      f"LDS {f.get('LDSByteSize')} B, instructions {len(ks[name][0])}")
        for name in ROWS:
            if name not in ks:
                continue
            ins = ks[name][0]
            print(f"-- {name}: store runs")
            for fam, idx in store_runs(ins):
                lo, hi = idx[0], idx[-1]
                figs = ", ".join(f"{n} {sum(1 for k in range(lo, hi + 1) if re.match(p, ins[k]))}" for n, p in COUNT)
                print(f"   {fam} stores {len(idx)}: instructions {hi - lo + 1} (at {lo}..{hi}); {figs}")


if __name__ == "__main__":
    main()
