"""The slice-walking form of the split-K small-map convolution (conv_h2_skw, csrc/h2.hip) against conv_h2_sk and against fp64.

A wave of conv_h2_skw is what a wave of conv_h2_sk is -- one K-slice of one block of 32 output channels, one running scale per
32-pixel slice -- but it walks SW = 1, 2 or 4 consecutive slices and fetches each weight fragment once for all of them.  Per
slice the products, their order and the scales are the same, so the results are required to be the same BITS as conv_h2_sk's
(afd_debug_conv_path 72 = never the new form), and to pass the gates of tests/test_gpu_h2_scales.py on inputs built on the
kernel's scale scopes (tests/h2_cases.py; tests/test_h2_skw_cases_host.py shows fp32 passes them on these shapes).

Shapes (S, Cin, Cout, B), 4 x 4 maps only -- the form does not cover the 8 x 8 maps, so the issue's (8, 128, 32, 5) is absent:
  (4, 256, 64, 13)  7 slices: SW = 4, a ragged second group with a half-empty last slice; forward 8 chunks over 4 K-slices (the
                    weights are reloaded per chunk), dgrad K = 64 in 2 K-slices x 2 pixel groups; two channel blocks
  (4, 128, 96, 9)   5 slices, one chunk per wave forward, three channel blocks; dgrad K = 96: 3 chunks over 2 K-slices
  (4, 64, 64, 9)    KSP = 2 both ways"""
import pytest
import torch

import h2_cases as H
from conftest import note

pytestmark = pytest.mark.gpu
SHAPES = [(4, 256, 64, 13), (4, 128, 96, 9), (4, 64, 64, 9)]
RESTORE = (0, 34, 8, 80, 60, 74, 84, 92, 64, 96, 88, 78)     # as tests/test_gpu_h2_scales.py; 74 also returns 71 / 72 to the rule
SK, WALK, NEVER = 73, 71, 72
_ids = lambda s: "x".join(str(v) for v in s)


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    yield afdm, ops, gpu
    for m in RESTORE:
        afdm.lib().afd_debug_conv_path(m)


def _modes(L, modes):
    for m in modes:
        L.afd_debug_conv_path(m)


def _run(ops, dev, x, w, dy):
    xd = x.to(dev).requires_grad_(True)
    y = ops.conv(xd, w.to(dev))
    (gx,) = torch.autograd.grad(y, xd, dy.to(dev))
    return y.detach().cpu(), gx.cpu()


def _cases(shape):
    for tag, x, w, dy in H.conv_inputs(shape):
        yield tag, x, w, dy, []
    yield from H.conv_zero_inputs(shape)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_skw_bit_identical_and_within_contract(A, shape):
    """Every input of h2_cases.conv_inputs and conv_zero_inputs: y and dx under 73 + 71 are torch.equal to 73 + 72, pass the
    per-image gate against fp64, and are exactly zero on all-zero scopes."""
    afdm, ops, dev = A
    L = afdm.lib()
    S, ci, co, B = shape
    bad = []
    try:
        for tag, x, w, dy, zi in _cases(shape):
            y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
            _modes(L, (82, SK, WALK))
            assert L.afd_conv3x3_weight_kinds(B, ci, co, S, S) == 3
            y, dx = _run(ops, dev, x, w, dy)
            _modes(L, (NEVER,))
            assert L.afd_conv3x3_weight_kinds(B, ci, co, S, S) == 3
            y1, dx1 = _run(ops, dev, x, w, dy)
            ey, ed = H.per_image(y, y64), H.per_image(dx, dx64)
            print(f"h2 skw {shape} {tag}: fwd {ey[0]:.2e} (image {ey[1]}) dgrad {ed[0]:.2e} (image {ed[1]}); "
                  f"equal to conv_h2_sk: y {torch.equal(y, y1)} dx {torch.equal(dx, dx1)}")
            note("F5 h2 skw: fwd per image", ey[0], (shape, tag, ey[1]))
            note("F5 h2 skw: dgrad per image", ed[0], (shape, tag, ed[1]))
            assert torch.isfinite(y).all() and torch.isfinite(dx).all(), tag
            assert not y[zi].any() and not dx[zi].any(), tag
            if not (torch.equal(y, y1) and torch.equal(dx, dx1) and ey[0] <= H.TOL and ed[0] <= H.TOL):
                bad.append((tag, ey, ed, torch.equal(y, y1), torch.equal(dx, dx1)))
    finally:
        _modes(L, RESTORE)
    assert not bad, bad


def _rule_width(B, K, N):
    """h2_skw_width (csrc/h2.hip) restated: slices per wave the default rule gives a 4 x 4 split-K launch (0: conv_h2_sk)"""
    if K < 128:
        return 0
    nslices = (B * 16 + 31) // 32
    for sw in (4, 2, 1):
        if -(-nslices // sw) * (N // 32) >= 512:
            return sw
    return 0


@pytest.mark.parametrize("C,sw,moving", [(256, 2, False), (128, 1, True)], ids=["256to256_SW2", "128to128_SW1"])
def test_skw_full_size_layer_default_rule(A, C, sw, moving):
    """C -> C @ 4 x 4, B = 256, with bias, GELU and residual in the epilogue (forward) and through autograd (dgrad): the default
    rule's result is torch.equal to mode 72's, and to the forced form's (71: SW = 4).  256 -> 256 on randn, where the rule
    walks two slices per wave; 128 -> 128, where it runs the form with one slice per wave (which 71 never picks), on inputs whose
    scales move (chunks nine decades apart, image pairs 2^+-30 apart).

    The library has no query for the slices per wave (and the issue allows no new export), so that the default rule takes
    the new form here is checked as far as it can be from outside: the launch rule restated above gives SW, the call returns
    AFD_OK (a failed opt-in to more than 64 KB of LDS would surface as AFD_ELAUNCH, which ops raises), and the default result
    equals the forced one bit for bit."""
    afdm, ops, dev = A
    L = afdm.lib()
    B, S = 256, 4
    g = H.gen(7 + C)
    x, res = torch.randn(B, C, S, S, generator=g), torch.randn(B, C, S, S, generator=g).to(dev)
    w, bias = (torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5)).to(dev), torch.randn(C, generator=g).to(dev)
    dy = torch.randn(B, C, S, S, generator=g)
    if moving:
        x, dy = H.pair_scale(H.k_ramp(x, "ascending"), H.PAIR_X), H.pair_scale(H.k_ramp(dy, "descending"), H.PAIR_DY)
    x, dy = x.to(dev), dy.to(dev)
    assert _rule_width(B, C, C) == sw

    def run():
        assert L.afd_conv3x3_weight_kinds(B, C, C, S, S) == 3
        y = ops.conv_infer(x, w, bias, res, act=1)
        xd = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(ops.conv(xd, w), xd, dy)
        torch.cuda.synchronize()
        return y.cpu(), gx.cpu()
    try:
        y0, d0 = run()
        _modes(L, (NEVER,))
        y1, d1 = run()
        _modes(L, (WALK,))
        y2, d2 = run()
    finally:
        _modes(L, RESTORE)
    assert torch.isfinite(y0).all() and torch.isfinite(d0).all()
    assert torch.equal(y0, y1) and torch.equal(d0, d1)
    assert torch.equal(y0, y2) and torch.equal(d0, d2)
