"""The four-wave workgroups of the f16x2 3x3 weight gradient (csrc/h2_wgrad.hip: wgrad_h2<S, BN, BK, 4>, wgrad_h2_s4<BN, BK, 4>),
forced block by block through afd_debug_conv_path 53 / 54 / 55 (64 x 32, 32 x 64, 32 x 32: output x input channels), beside the
eight-wave form of the same call (51).

Oracle: fp64 conv2d weight gradients on the CPU (tests/h2_cases.py wgrad3_ref).  Gate: the per-32x32-block bound of
tests/test_gpu_h2_scales.py (its TOL and its _gate; h2_cases.per_block) -- a workgroup owns a block of one split's slab, and
every block of 64 x 32 or 32 x 64 is two of those.

Shapes: the smallest at which a form can go wrong.  AFD_WGB_TARGET = 4 (read per call) keeps the launches at a few workgroups,
so that every split walks two or more tiles and the running scales are carried from tile to tile:

  32 x 32, B 2,  64 -> 64    16 tiles; two input-channel blocks of the 64 x 32 form, two output-channel blocks of 32 x 64
  16 x 16, B 4,  64 -> 128 and 128 -> 64    mixed widths, 8 tiles
   8 x 8,  B 5,  64 -> 64    two images per tile: the last tile is half empty
   4 x 4,  B 9, 128 -> 128   wgrad_h2_s4; the last tile holds 1 of 8 images; 32 x 32 runs with two wave groups (NSG = 2)

Inputs: seeded normal values, as they are, with x rising by 2^12 over the tiles, and with dY rising by 2^12 (both running
scales move)."""
import ctypes

import pytest
import torch

import h2_cases as H
import test_gpu_h2_scales as HS

pytestmark = pytest.mark.gpu
RESTORE = HS.RESTORE + (50,)
SHAPES = [(32, 2, 64, 64), (16, 4, 64, 128), (16, 4, 128, 64), (8, 5, 64, 64), (4, 9, 128, 128)]      # (S, B, Cin, Cout)
SETS = ("plain", "x ramp", "dy ramp")
FORMS = ((53, 64, 32), (54, 32, 64), (55, 32, 32))                 # (mode, output channels, input channels per workgroup)
TARGET = 4                                                         # workgroups per launch
_REF = {}


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    yield afdm, ops, gpu
    for m in RESTORE:
        afdm.lib().afd_debug_conv_path(m)


def _inputs(S, B, ci, co, which):
    """-> x, dY, fp64 dW (computed once per case and shared)"""
    key = (S, B, ci, co, which)
    if key not in _REF:
        g = H.gen(1000 * S + 10 * B + ci // 64)
        x, dy = torch.randn(B, ci, S, S, generator=g), torch.randn(B, co, S, S, generator=g)
        nb = H.wg_bands(S)
        if which == "x ramp":
            x = H.stream_ramp(x, "ascending", 0, 12, nb)
        elif which == "dy ramp":
            dy = H.stream_ramp(dy, "ascending", 0, 12, nb)
        _REF[key] = (x, dy, H.wgrad3_ref(x, dy, torch.float64))
    return _REF[key]


def _plan(L, B, ci, co, S):
    info = (ctypes.c_int * 5)()
    slabs = L.afd_conv_wgrad3_plan(B, ci, co, S, S, ctypes.addressof(info))
    return slabs, tuple(info)


@pytest.mark.parametrize("which", SETS, ids=lambda s: s.replace(" ", "_"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_B%d_%dto%d" % (s[0], s[0], s[1], s[2], s[3]))
def test_four_wave_forms(A, monkeypatch, shape, which):
    """Every four-wave block and the eight-wave form against fp64 under the per-block gate; two four-wave calls bit-equal; the
    launch reports the slab count the plan query promised, and the workspace query covers it."""
    afdm, ops, dev = A
    L = afdm.lib()
    S, B, ci, co = shape
    monkeypatch.setenv("AFD_WGB_TARGET", str(TARGET))
    x, dy, dw64 = _inputs(S, B, ci, co, which)
    xd, dyd = x.to(dev), dy.to(dev)
    nt = {4: (B + 7) // 8, 8: (B + 1) // 2}.get(S, B * S * S // 128)
    bad = []
    try:
        for mode, bn, bk in FORMS + ((51, 0, 0),):
            HS._modes(L, (86, 78, mode))
            assert L.afd_conv_wgrad_form(B, ci, co, S, S, 3) == 4
            slabs_q, (tps, ntq, pbn, pbk, nw) = _plan(L, B, ci, co, S)
            if mode == 51:
                assert nw == 8
            else:
                assert (pbn, pbk, nw) == (bn, bk, 4), (mode, pbn, pbk, nw)          # the form under test took the shape
                assert (pbn // 16) * (pbk // 32) <= 4
            assert ntq == nt and slabs_q == -(-nt // tps) and (tps >= 2 or nt < 2), (nt, ntq, tps, slabs_q)
            assert L.afd_conv_wgrad_workspace_bytes(B, ci, co, S, S, 3) >= 4 * slabs_q * 9 * co * ci
            dw, _, slabs = HS._wgrad_call(A, xd, dyd, 3)
            assert slabs == slabs_q, (mode, slabs, slabs_q)
            e = H.per_block(dw, dw64)
            print(f"wgrad w4 {shape} {which}: mode {mode} block {pbn}x{pbk} waves {nw} slabs {slabs} x {tps} tiles, worst block {e[0]:.2e} at {e[1]}")
            fam = "F5 h2 wgrad %s-wave: per 32x32 block" % ("eight" if mode == 51 else "four")
            if not HS._gate(fam, e, (shape, which, mode)):
                bad.append((mode, e))
            if mode != 51:
                dw2, _, _ = HS._wgrad_call(A, xd, dyd, 3)
                assert torch.equal(dw, dw2), mode
    finally:
        HS._modes(L, RESTORE)
    assert not bad, bad
