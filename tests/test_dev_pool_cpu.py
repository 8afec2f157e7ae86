"""Device memory ownership on the CPU (csrc/dev_pool.h).

DevPool is the one place of the host runtime that calls hipMalloc / hipFree: every handle allocates
from pools it holds by value, and two process-wide counters (az_diag_device_mem) say what is alive.
tests/native/dev_pool_host.cpp is a stand-alone program that defines the HIP allocation calls itself
(malloc-backed) and checks the pool's bookkeeping: order and recorded bytes, release, clear, moves,
the failure injection of az_diag_fail_alloc at every position of a sequence, counters back at zero.
The source scan below is the invariant that makes the counters mean something: no other file of the
runtime allocates or frees device or pinned memory itself (tests/test_gpu_device_mem.py then holds
every handle's lifecycle and failure paths to the counters on the device)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-multi-game_amd")
SRC = os.path.join(ROOT, "tests", "native", "dev_pool_host.cpp")


def test_dev_pool_program(tmp_path):
    exe = str(tmp_path / "dev_pool_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "dev_pool ok", r.stdout + r.stderr


CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\(")


def test_only_dev_pool_and_pinned_allocate():
    """Outside dev_pool.h and the Pinned template no source of the runtime calls hipMalloc, hipFree,
    hipHostMalloc or hipHostFree."""
    found, pinned, pool = [], 0, 0
    for top in ("csrc", "cpp"):
        for d, _, files in os.walk(os.path.join(PKG, top)):
            for f in sorted(files):
                path = os.path.join(d, f)
                text = open(path, errors="replace").read()
                if f == "engine_internal.h":
                    a = text.index("struct Pinned {")
                    b = text.index("};", a)
                    pinned = len(CALLS.findall(text[a:b]))
                    text = text[:a] + text[b:]
                if f == "dev_pool.h":
                    pool = len(CALLS.findall(text))
                    continue
                for i, line in enumerate(text.splitlines(), 1):
                    if CALLS.search(line):
                        found.append(f"{os.path.relpath(path, ROOT)}:{i}: {line.strip()}")
    assert not found, "\n".join(found)
    assert pool >= 2 and pinned >= 2          # the scan did look at the two places that may
