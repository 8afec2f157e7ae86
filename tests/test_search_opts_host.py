"""Search options on the host (selection strategy, depth cap, TD(lambda) backup, progressive widening):
  (1) az_amd._lib.SearchOpts mirrors az_search_opts byte for byte (the options are a struct of their own:
      az_search_cfg keeps its layout, which tests/test_go_rules_host.py pins);
  (2) az_search_widening_table (host only) equals the patched REFERENCE's getProgressiveWideningCount
      entry for entry (tests/golden/ref_search_opts_widening.json) and refuses what the engine refuses;
  (3) the golden games cover what they exist for (tests/golden/gen_search_opts_golden.py asserts the
      same on the reference's output);
  (4) the RunMetadata key set is unchanged."""
import ctypes
import gzip
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
with gzip.open(os.path.join(GOLD, "ref_search_opts_games.json.gz"), "rt") as _f:
    GAMES = json.load(_f)
with open(os.path.join(GOLD, "ref_search_opts_widening.json")) as _f:
    WIDENING = json.load(_f)
OPT_FIELDS = ["selection", "max_search_depth", "use_td", "td_lambda", "use_widening", "widening_min_visits",
              "widening_base", "widening_exponent"]


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def actions(g):
    return [m["action"] for m in g["moves"]]


def test_search_opts_ctypes_mirror_matches_the_header(tmp_path):
    import az_amd._lib as L
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "az_engine.h"', 'int main(void) {']
    for cname, cls in (("az_search_cfg", L.SearchCfg), ("az_search_opts", L.SearchOpts)):
        lines.append(f'    printf("%zu\\n", sizeof({cname}));')
        lines += [f'    printf("%zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname}*)0)->{n}));' for n, _ in cls._fields_]
    lines.append('    printf("%d %d %d %d\\n", AZ_SEL_UCB, AZ_SEL_PUCT, AZ_SEL_PROGRESSIVE_BIAS, AZ_SEL_RAVE);')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split("\n")
    for cls in (L.SearchCfg, L.SearchOpts):
        names = [n for n, _ in cls._fields_]
        assert int(out[0]) == ctypes.sizeof(cls)
        for n, line in zip(names, out[1:]):
            f = getattr(cls, n)
            assert [int(x) for x in line.split()] == [f.offset, f.size], n
        assert getattr(cls, names[-1]).offset + getattr(cls, names[-1]).size == ctypes.sizeof(cls)
        out = out[1 + len(names):]
    assert [int(x) for x in out[0].split()] == [L.AZ_SEL_UCB, L.AZ_SEL_PUCT, L.AZ_SEL_PROGRESSIVE_BIAS, L.AZ_SEL_RAVE] == \
        [0, 1, 2, 3]
    assert [n for n, _ in L.SearchOpts._fields_] == OPT_FIELDS
    # the configuration itself is as it was: it ends with the Go rules
    assert [n for n, _ in L.SearchCfg._fields_][-1] == "go_superko"


def test_az_amd_search_option_fields():
    import az_amd

    def fields(**kw):
        o = az_amd._search_opts_struct(kw)
        return tuple(getattr(o, n) for n in OPT_FIELDS)

    assert fields() == (1, 1000, 0, np.float32(0.8), 0, 10, 2.0, 0.5)          # MCTSConfig's defaults
    assert fields(use_td=True, td_lambda=0.5) == (1, 1000, 1, 0.5, 0, 10, 2.0, 0.5)
    assert fields(selection=az_amd.AZ_SEL_PROGRESSIVE_BIAS, use_widening=True, widening_min_visits=1) == \
        (2, 1000, 0, np.float32(0.8), 1, 1, 2.0, 0.5)
    with pytest.raises(TypeError, match="unknown search options"):
        az_amd._search_opts_struct(dict(widening=True))


@pytest.mark.parametrize("idx", range(len(WIDENING)), ids=[f"{w['base']}-{w['exponent']}-{w['children']}" for w in WIDENING])
def test_widening_table_matches_reference(idx):
    """The table is the reference's count for every N it covers; past a complete table the reference's
    count is "every child", and at N <= 0 it is 1 -- the two rules the device applies without the table."""
    import az_amd
    w = WIDENING[idx]
    base, exponent, children = f32(w["base_bits"]), f32(w["exponent_bits"]), w["children"]
    assert (base, exponent) == (np.float32(w["base"]), np.float32(w["exponent"]))
    tab = az_amd.widening_table(base, exponent, children)
    assert tab.dtype == np.int32 and tab[0] == 1 and tab[-1] == children and (tab[:-1] < children).all()
    assert (np.diff(tab) >= 0).all()
    for n, count in zip(range(w["n0"], w["n0"] + len(w["counts"])), w["counts"]):
        mine = 1 if n <= 0 else int(tab[n]) if n < len(tab) else children
        assert mine == count, (n, mine, count)
    assert w["n0"] < 0 and len(w["counts"]) == 4101


def test_widening_fixture_covers_the_cases():
    assert sorted({(w["base"], w["exponent"]) for w in WIDENING}) == [(0.5, 1.0), (1.0, 0.5), (2.0, 0.5), (3.0, 0.8)]
    assert {w["children"] for w in WIDENING} == {82, 362} and len(WIDENING) == 8
    # tables that end inside the fixture's range and tables that run past it
    assert any(w["counts"][-1] == w["children"] for w in WIDENING) and any(w["counts"][-1] < w["children"] for w in WIDENING)


def test_widening_table_refusals_and_truncation():
    import az_amd
    from az_amd import _lib
    n = ctypes.c_int(-1)
    for base, exponent, na in ((0.0, 0.5, 82), (-1.0, 0.5, 82), (float("nan"), 0.5, 82), (float("inf"), 0.5, 82),
                               (2.0, 0.0, 82), (2.0, -0.5, 82), (2.0, 1.5, 82), (2.0, float("nan"), 82), (2.0, 0.5, 0),
                               (2.0, 0.5, 363)):
        assert _lib.lib().az_search_widening_table(base, exponent, na, None, 0, ctypes.byref(n)) == _lib.AZ_ERR_ARG, \
            (base, exponent, na)
        assert _lib.lib().az_last_error()
    assert n.value == -1
    assert _lib.lib().az_search_widening_table(2.0, 0.5, 82, None, 0, None) == _lib.AZ_ERR_ARG
    # the length alone (cap 0), then a short buffer: only `cap` entries are written
    assert _lib.lib().az_search_widening_table(2.0, 0.5, 82, None, 0, ctypes.byref(n)) == 0 and n.value == 1682   # 2 sqrt(1681) = 82
    buf = np.full(8, -7, np.int32)
    assert _lib.lib().az_search_widening_table(2.0, 0.5, 82, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 4, ctypes.byref(n)) == 0
    assert buf.tolist() == [1, 2, 2, 3, -7, -7, -7, -7] and n.value == 1682
    # a table the limit cuts is incomplete: its last entry is below the action space
    old = _lib.lib().az_diag_set_widening_cap(16)
    try:
        tab = az_amd.widening_table(1.0, 0.5, 82)
        assert len(tab) == 16 and tab[-1] == 3
    finally:
        assert _lib.lib().az_diag_set_widening_cap(old) == 16
    assert old == 1 << 22 and len(az_amd.widening_table(1.0, 0.5, 82)) == 82 * 82 + 1


def test_golden_games_cover_the_options():
    """What the fixtures exist for (the generator asserts the same on the reference's output)."""
    by = {g["name"]: g for g in GAMES}
    assert len(by) == len(GAMES)
    for g in GAMES:
        # every option case differs from the same case without its options, except the 60-simulation UCB
        # case: no simulation revisits a root child, so UCB and PUCT coincide there (ucb-100 differs)
        assert (actions(g) == g["plain_actions"]) == (g["name"] == "ucb"), g["name"]
        if g["opts"]["use_widening"]:
            assert g["min_child_n"] < 0 and min(c[1] for m in g["moves"] for c in m["children"]) == g["min_child_n"], g["name"]
    td = [g for g in GAMES if g["opts"]["use_td"]]
    assert {g["opts"]["td_lambda"] for g in td} >= {0.8, 0.5, 0.3}
    assert any(g["case"][5] == 1 and g["case"][7] == 0.25 for g in td)                       # per-search noise + FPU
    assert any(g["case"][0] == 5 and g["moves"][-1]["tt_hits"] > 0 for g in td)             # TT hits
    assert {(g["case"][0], g["opts"]["max_search_depth"]) for g in GAMES if g["opts"]["max_search_depth"] < 1000} == {(5, 1), (9, 2)}
    assert {(g["go"], g["opts"]["selection"]) for g in GAMES} >= {(0, 2), (1, 2), (0, 0)}
    wid = [g for g in GAMES if g["opts"]["use_widening"]]
    assert {g["go"] for g in wid} == {0, 1}
    assert any((g["opts"]["widening_min_visits"], g["opts"]["widening_base"], g["virtual_loss"]) == (1, 1.0, 1) for g in wid)
    assert any(g["opts"]["selection"] == 2 and g["opts"]["use_td"] and g["case"][3] == "random" for g in wid)
    assert any(g["case"][0] == 13 and any(sum(c[1] < 0 for c in m["children"]) > 64 for m in g["moves"]) for g in wid)
    seeds = [g for g in GAMES if g["name"].startswith("td-seed")]
    assert sorted(g["noise_seed"] for g in seeds) == [42, 43, 44] and len({tuple(actions(g)) for g in seeds}) == 3
    sw = by["switch"]
    assert sw["switch_ply"] == 6 and sw["switch"]["selection"] == 2 and sw["switch"]["use_td"] == 1
    assert actions(sw)[:6] == sw["plain_actions"][:6] and sw["opts"]["selection"] == 1 and not sw["opts"]["use_td"]
    for name in ("ref_search_opts_games.json.gz", "ref_search_opts_widening.json"):
        assert os.path.getsize(os.path.join(GOLD, name)) <= os.path.getsize(os.path.join(GOLD, "ref_go_rules_games.json.gz"))


def test_run_metadata_keys_unchanged():
    """--progressive-widening now reaches the search; the metadata file's keys stay the reference's."""
    az = pytest.importorskip("_alphazero_cpp", reason="build the host module: make -C alphazero-multi-game_amd")
    from test_self_play_main import EXT_KEYS, REF_KEYS
    m = az.RunMetadata()
    m.progressiveWidening = True
    txt = az.runMetadataJson(m)
    assert re.findall(r'^  "([a-z_0-9]+)": ', txt, flags=re.M) == REF_KEYS + EXT_KEYS
    assert json.loads(txt)["progressive_widening"] is True


def test_host_config_carries_the_options():
    """MCTSConfig's option fields keep the reference's defaults and names (the pybind layer needs no new ones)."""
    az = pytest.importorskip("_alphazero_cpp")
    c = az.MCTSConfig()
    assert (c.selectionStrategy, c.maxSearchDepth, c.useTemporalDifference, c.useProgressiveWidening,
            c.minVisitsForWidening) == (az.MCTSNodeSelection.PUCT, 1000, False, False, 10)
    assert (c.tdLambda, c.progressiveWideningBase, c.progressiveWideningExponent) == (np.float32(0.8), 2.0, 0.5)
    assert [int(az.MCTSNodeSelection.UCB), int(az.MCTSNodeSelection.PUCT), int(az.MCTSNodeSelection.PROGRESSIVE_BIAS),
            int(az.MCTSNodeSelection.RAVE)] == [0, 1, 2, 3]
