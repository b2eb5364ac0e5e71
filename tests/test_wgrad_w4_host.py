"""The plan of the matrix-core 3x3 weight gradient, host side (nothing is launched): for every 3x3 layer shape of the Config-D
step at B = 256 the default rule picks a form that exists, the workspace query covers the slabs the launch will write, and no
layer writes more slabs than the eight-wave plan (afd_debug_conv_path 51: one workgroup per CU everywhere)."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = 256
# (Cin, Cout, S) of the Config-D UNet's 3x3 layers with 32 or more input channels (bench.py CONV3, each shape once)
SHAPES = [(32, 32, 32), (32, 32, 16), (32, 64, 16), (64, 64, 16), (64, 64, 8), (64, 128, 8), (128, 128, 8), (128, 128, 4),
          (128, 256, 4), (256, 256, 4), (256, 128, 4), (256, 256, 8), (256, 128, 8), (128, 64, 8), (128, 128, 16), (128, 64, 16),
          (64, 32, 16), (64, 64, 32), (64, 32, 32)]


def _plan(L, ci, co, S):
    info = (ctypes.c_int * 5)()
    return L.afd_conv_wgrad3_plan(B, ci, co, S, S, ctypes.addressof(info)), tuple(info)


def test_shapes_are_config_d():
    import bench
    assert set(SHAPES) == {s for s in bench.CONV3 if s[0] >= 32}


@pytest.mark.parametrize("mode", (50, 51, 52), ids=("rule", "eight", "four"))
def test_plan_query_and_workspace_agree(mode):
    import afdm
    L = afdm.lib()
    try:
        for ci, co, S in SHAPES:
            L.afd_debug_conv_path(51)
            slabs8, _ = _plan(L, ci, co, S)
            L.afd_debug_conv_path(mode)
            assert L.afd_conv_wgrad_form(B, ci, co, S, S, 3) == 4
            slabs, (tps, nt, bn, bk, nw) = _plan(L, ci, co, S)
            assert nt == {4: B // 8, 8: B // 2}.get(S, B * S * S // 128)
            assert bn in (32, 64) and bk in (32, 64) and co % bn == 0 and ci % bk == 0
            assert nw in (4, 8) and (nw == 8 or mode != 51) and (nw == 4 or mode != 52)
            roles = (bn // 16) * (bk // 32)
            assert roles <= nw and nw % roles == 0, (ci, co, S, bn, bk, nw)          # a kernel of that form exists
            assert tps >= 1 and slabs == -(-nt // tps) and (slabs - 1) * tps < nt     # no empty split
            assert 1 <= slabs <= slabs8, (ci, co, S, slabs, slabs8)                   # never more slab bytes than eight waves
            assert L.afd_conv_wgrad_workspace_bytes(B, ci, co, S, S, 3) >= 4 * slabs * (9 * co * ci + co)
    finally:
        L.afd_debug_conv_path(50)


def test_bf16x3_arithmetic_keeps_eight_waves():
    import afdm
    L = afdm.lib()
    try:
        L.afd_debug_conv_path(79)
        L.afd_debug_conv_path(52)
        for ci, co, S in SHAPES:
            assert _plan(L, ci, co, S)[1][4] == 8
    finally:
        L.afd_debug_conv_path(78)
        L.afd_debug_conv_path(50)
