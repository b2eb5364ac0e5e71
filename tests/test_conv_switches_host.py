"""afd_debug_conv_path, host side (nothing is launched): every accepted mode sets exactly the switches its row of the table
below names, to exactly the values named, and every other integer is refused and changes nothing.  The table is written out
here, not read from the code: it is what callers (tests, tools, bench.py, training.TrainStep) rely on."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the switches, in the order afd_debug_conv_state reports them
TILE, PW, WGRAD_NW, WG_TARGET, WG_WAVES, H2_FEED, WINO, SKW, SK, DIRECT_ARITH, WG_ARITH, DIRECT, WG3, WG1, ENDS, WGWINO, GRID = range(17)
DEFAULT_MODES = (0, 8, 34, 48, 50, 60, 64, 74, 76, 78, 80, 84, 88, 92, 96, 100000)
DEFAULT_STATE = {TILE: 0, PW: 0, WGRAD_NW: 0, WG_TARGET: 256, WG_WAVES: 0, H2_FEED: 1, WINO: 0, SKW: 0, SK: 0, DIRECT_ARITH: 0,
                 WG_ARITH: 0, DIRECT: 0, WG3: 0, WG1: 0, ENDS: 0, WGWINO: 0, GRID: 0}
# mode -> {switch: value}
TABLE = {
    0: {TILE: 0}, 1: {TILE: 1}, 2: {TILE: 2},                                  # tile path
    8: {PW: 0}, 9: {PW: 1}, 10: {PW: 2},                                       # 1x1 streaming
    32: {WGRAD_NW: 4}, 33: {WGRAD_NW: 8}, 34: {WGRAD_NW: 0},                   # fp32 wgrad waves
    48: {WG_TARGET: 256}, 49: {WG_TARGET: 160},                                # wgrad workgroup target
    50: {WG_WAVES: 0}, 51: {WG_WAVES: 1}, 52: {WG_WAVES: 2}, 53: {WG_WAVES: 3}, 54: {WG_WAVES: 4}, 55: {WG_WAVES: 5},   # f16x2 wgrad waves mode
    59: {H2_FEED: 4}, 60: {H2_FEED: 1}, 61: {H2_FEED: 0}, 62: {H2_FEED: 2}, 63: {H2_FEED: 3},                          # h2 operand feed
    64: {WINO: 0}, 65: {WINO: 1}, 66: {WINO: 2}, 67: {WINO: 3}, 68: {WINO: 4}, 69: {WINO: 5}, 70: {WINO: 6},           # Winograd mode
    71: {SKW: 1}, 72: {SKW: 2},                                                # slice-walking split-K
    73: {SK: 2},                                                               # split-K mode
    74: {SKW: 0, SK: 0},                                                       # slice-walking AND split-K
    75: {SK: 1},
    76: {DIRECT_ARITH: 0}, 77: {DIRECT_ARITH: 1},                              # direct-form arithmetic
    78: {WG_ARITH: 0}, 79: {WG_ARITH: 1},                                      # wgrad arithmetic
    80: {DIRECT: 0}, 81: {DIRECT: 1}, 82: {DIRECT: 2},                         # direct bf16x3 mode
    84: {WG3: 0}, 85: {WG3: 1}, 86: {WG3: 2},                                  # bf16x3 3x3 wgrad mode
    88: {WG1: 0}, 89: {WG1: 1},                                                # 1x1 matrix-core wgrad
    92: {ENDS: 0}, 93: {ENDS: 1},                                              # output-layer kernels
    96: {WGWINO: 0}, 97: {WGWINO: 1}, 98: {WGWINO: 2},                         # Winograd wgrad
    100000: {GRID: 0}, 100001: {GRID: 1}, 100007: {GRID: 7}, 199999: {GRID: 99999},   # Winograd grid: 100000 + g
}
REFUSED = tuple(range(3, 8)) + tuple(range(11, 32)) + tuple(range(35, 48)) + (56, 57, 58, 83, 87, 90, 91, 94, 95, 99) + \
          (-1, 99999, 200000, 100, 101, 1000, -74, 2 ** 31 - 1, -2 ** 31)
PREFIX = "afd_debug_conv_path: mode must be"


def _lib():
    import afdm
    return afdm.lib()


def _state(L):
    count = L.afd_debug_conv_state(None, 0)
    v = (ctypes.c_long * count)()
    assert L.afd_debug_conv_state(ctypes.addressof(v), count) == count
    return list(v)


def _reset(L):
    for m in DEFAULT_MODES:
        L.afd_debug_conv_path(m)


def _default():
    return [DEFAULT_STATE[i] for i in range(len(DEFAULT_STATE))]


def test_default_state():
    L = _lib()
    _reset(L)
    assert _state(L) == _default()


def test_table_lists_every_mode_outside_refused():
    assert not set(TABLE) & set(REFUSED)
    assert {m for m in range(-1, 100) if m not in REFUSED} == {m for m in TABLE if m < 100000}


def test_state_read_back_is_bounded():
    L = _lib()
    _reset(L)
    count = L.afd_debug_conv_state(None, 0)
    assert count == len(DEFAULT_STATE)
    v = (ctypes.c_long * (count + 2))(*([-7] * (count + 2)))
    assert L.afd_debug_conv_state(ctypes.addressof(v), 3) == count
    assert list(v) == _default()[:3] + [-7] * (count - 1)
    assert L.afd_debug_conv_state(ctypes.addressof(v), count + 2) == count
    assert list(v) == _default() + [-7, -7]


@pytest.mark.parametrize("mode", sorted(TABLE))
def test_mode_sets_exactly_its_switches(mode):
    L = _lib()
    try:
        _reset(L)
        L.afd_debug_conv_path(mode)
        want = _default()
        for k, v in TABLE[mode].items():
            want[k] = v
        assert _state(L) == want
    finally:
        _reset(L)
    assert _state(L) == _default()


@pytest.mark.parametrize("first, second, want", [(71, 74, {}), (73, 75, {SK: 1}), (79, 52, {WG_ARITH: 1, WG_WAVES: 2}),
                                                   (100007, 100000, {}), (72, 73, {SKW: 2, SK: 2}), (73, 74, {})])
def test_order_dependent_cases(first, second, want):
    L = _lib()
    try:
        _reset(L)
        L.afd_debug_conv_path(first)
        L.afd_debug_conv_path(second)
        exp = _default()
        for k, v in want.items():
            exp[k] = v
        assert _state(L) == exp
    finally:
        _reset(L)


@pytest.mark.parametrize("mode", REFUSED)
def test_other_integers_are_refused(mode):
    from afdm._lib import AfdError
    L = _lib()
    try:
        _reset(L)
        L.afd_debug_conv_path(77)                         # a state that is not the default: a refused mode must not reset it either
        L.afd_debug_conv_path(100005)
        before = _state(L)
        with pytest.raises(AfdError) as e:
            L.afd_debug_conv_path(mode)
        assert PREFIX in str(e.value) and str(e.value).split(": ", 1)[1].startswith(PREFIX)
        assert _state(L) == before
    finally:
        _reset(L)
