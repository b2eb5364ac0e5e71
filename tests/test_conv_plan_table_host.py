"""The convolution planners against a recorded table (nothing is launched): tools/conv_plan_table.py walks a fixed list of layer
shapes under every afd_debug_conv_path mode, each applied from the default state, and asks the query entry points (weight
kinds, Winograd workspace of both passes, weight-gradient form and workspace at ksize 1 and 3, the 3x3 weight-gradient plan
with its five info values).  tests/conv_plan_table.json is that sweep, recorded before the switches moved into one struct
behind one table; this test replays it on the built library and compares every value exactly.  Regenerate the file only when
a rule is changed on purpose.

Families that change at least one recorded answer, so that the sweep pins them: 48 / 49, 50-55, 64-70, 73-75, 76 / 77, 78 / 79,
80-82, 84-86, 88 / 89, 96-98 (test_each_planning_family_moves_a_recorded_value).  Launch-only families, which change no recorded
answer for any shape: 0-2, 8-10, 32-34, 59-63, 71 / 72, 92 / 93 and the Winograd grid (100000 + g).  These rest on
tests/test_conv_switches_host.py, which pins the switch each mode sets, and on the GPU tests that run under them."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import conv_plan_table as T  # noqa: E402

PLANNING = ((48, 49), range(50, 56), range(64, 71), (73, 74, 75), (76, 77), (78, 79), (80, 81, 82), (84, 85, 86), (88, 89), (96, 97, 98))
LAUNCH_ONLY = (0, 1, 2, 8, 9, 10, 32, 33, 34, 59, 60, 61, 62, 63, 71, 72, 92, 93, 100000, 100007)


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(ROOT, "tests", "conv_plan_table.json")) as f:
        return json.load(f)


def test_table_is_the_tools_sweep(table):
    assert [tuple(s) for s in table["shapes"]] == T.SHAPES and tuple(table["fields"]) == T.FIELDS
    assert sorted(int(m) for m in table["modes"]) == sorted(T.MODES)
    assert len(table["default"]) == len(T.SHAPES) and all(len(r) == len(T.FIELDS) for r in table["default"])


def test_shapes_cover_the_case_tables():
    import param_grad_cases as P
    import unet64_cases as U
    layers = {tuple(cc.case[1:5]) for cc in U.CONV_CASES}
    layers |= {(ci, co, S, S) for _, _, ci, co, S, _, _ in P.CONV3} | {(ci, co, S, S) for _, _, ci, co, S in P.CONV1}
    layers |= {c.consts["geom"][1:5] for c in P.tied_cases() if c.kind == "conv"}
    assert layers <= set(T.LAYERS)
    assert set(T.BATCHES) == {256, 6, 1}
    L = T.LAYERS
    assert any(l[0] == 3 for l in L) and any(l[0] == 24 for l in L) and any(l[1] == 48 for l in L)
    assert any(l[2] != l[3] for l in L) and any(l[3] == 64 for l in L) and any(l[3] == 2 for l in L)


def test_each_planning_family_moves_a_recorded_value(table):
    for fam in PLANNING:
        assert any(table["modes"][str(m)] for m in fam), f"no mode of {tuple(fam)} changes a recorded answer"
    assert not any(table["modes"][str(m)] for m in LAUNCH_ONLY)
    assert {m for fam in PLANNING for m in fam} | set(LAUNCH_ONLY) == set(T.MODES)


def test_replay(table):
    import afdm
    got = T.sweep(afdm.lib())
    assert got["default"] == table["default"]
    for m in T.MODES:
        assert got["modes"][str(m)] == table["modes"][str(m)], f"mode {m}"
