"""The Renju / Omok predicates on the CPU (csrc/gomoku_rules.h compiled for the host).

The header is the one statement of the rules: the device kernels build the forbidden mask of a
Black-to-move leaf from it and the host GomokuState answers from it.  Here it is compiled with g++
(-Wall -Werror) into a stand-alone program (tests/native/gomoku_rules_host.cpp), once plain and
once with -fsanitize=address,undefined, and fed every position of
tests/golden/ref_gomoku_rules_positions.json.gz (the patched REFERENCE GomokuState / GomokuRules,
written by tests/golden/gen_gomoku_rules_golden.py): the per-cell verdicts, the forbidden mask and
the legal count must equal the reference's exactly."""
import gzip
import json
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
with gzip.open(os.path.join(GOLD, "ref_gomoku_rules_positions.json.gz"), "rt") as _f:
    POSITIONS = json.load(_f)
ALL = [(f"{k}[{i}]", p) for k in sorted(POSITIONS) for i, p in enumerate(POSITIONS[k])]


def _build(tmp_path_factory, name, extra):
    exe = str(tmp_path_factory.mktemp(name) / "gomoku_rules_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + extra +
                   [os.path.join(HERE, "native", "gomoku_rules_host.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _build(tmp_path_factory, "gomokurules", [])


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    return _build(tmp_path_factory, "gomokurules_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, positions):
    text = "".join(f"{p['bs']} {p['renju']} {p['omok']} {len(p['moves'])} {' '.join(map(str, p['moves']))}\n" for _, p in positions)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(positions)
    out = []
    for line in lines:
        over, four, three, legal, mask = line.split(";")
        cells = [[int(x) for x in f.split(",")] if f else [] for f in (over, four, three)]
        out.append(cells + [int(legal), [int(w, 16) for w in mask.split(",")]])
    return out


def _check(exe):
    assert len(ALL) > 100
    for (name, p), (over, four, three, legal, mask) in zip(ALL, _run(exe, ALL)):
        assert over == p["renju_overline"] == p["omok_overline"], (name, "overline")
        assert four == p["renju_double_four"], (name, "double four")
        assert three == p["omok_double_three"], (name, "double three")
        assert p["renju_double_three_refused"] == [], name       # why the header has no Renju double-three test
        A = p["bs"] ** 2
        forbidden = sorted(a for a in range(A) if mask[a >> 6] >> (a & 63) & 1)
        if p["player"] == 1:
            want = sorted(set(over + four) if p["renju"] else set(over + three))
        else:
            want = []                                            # White is never restricted
        assert forbidden == want, (name, "mask")
        assert legal == A - len(p["moves"]) - len(want), (name, "legal count")
        if not p["terminal"]:
            assert legal == len(p["legal"]) and not set(p["legal"]) & set(forbidden), (name, "legal list")
        elif p["result"] == 1 and len(p["moves"]) < A:
            assert legal == 0 and p["player"] == 1, (name, "stalemate")


def test_rule_predicates_match_reference_positions(plain):
    _check(plain)


def test_rule_predicates_under_address_and_undefined_sanitizers(sanitized):
    _check(sanitized)
