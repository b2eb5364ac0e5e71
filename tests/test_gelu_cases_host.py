"""CPU checks of tests/gelu_cases.py: the grid holds what it promises, the delta-tap identity that lets a test place exact
values of u into the fused kernel's table lookup, the fp32 figures behind the gates, and the fp32 restatement of `gelu_piece`
against those gates.  Prints the figures (run with -s)."""
import math

import numpy as np
import pytest
import torch

import gelu_cases as G
from oracle import ref_ops as R


def test_grid_holds_every_special_point_and_fits_every_case():
    u = G.grid()
    assert u.dtype == torch.float32 and u.numel() == G.GRID_N and bool(torch.isfinite(u).all())
    have = set(u.numpy().view(np.uint32).tolist())                       # by bit pattern: +0 and -0 are two points
    want = []
    for k in range(-130, 131):
        v = np.float32(k / 16.0)
        assert float(v) == k / 16.0
        want += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    for v in (6.0, 6.5, 8.0, 50.0, 1e4, 3e38, 1e-30, 1e-45, 0.0):
        want += [np.float32(v), np.float32(-v)]
    want += [np.nextafter(np.float32(s * 6.0), np.float32(d)) for s in (-1, 1) for d in (-np.inf, np.inf)]
    for v in want:
        assert int(np.asarray(v, dtype=np.float32).view(np.uint32)) in have, float(v)
    assert float(np.float32(1e-45)) > 0 and float(np.float32(1e-45)) < G.TINY          # a denormal
    fill = u[(u.abs() <= 8) & (u.abs() > 0)]
    assert fill.numel() > 3000 and float(u.min()) == -float(np.float32(3e38))
    for S, C in G.filt_act_cases():
        n = C * S * S
        un = G.grid(n)
        assert un.numel() == n and set(un.numpy().view(np.uint32).tolist()) >= set(G.special_points().view(np.uint32).tolist())
        ppw = max(64 // S, 1)
        assert (C % ppw == 0) or (C - 1) % ppw == 0
    assert {S for S, _ in G.filt_act_cases()} == {4, 8, 16, 32, 64}
    assert sum(1 for S, C in G.filt_act_cases() if C % max(64 // S, 1)) == 4          # dead-lane variants at S = 4 .. 32


def test_delta_taps_turn_the_filtered_gelu_into_gelu():
    """ku = kd = delta: R.filt_act and the closed form the kernel implements are y = GELU(x) and dx = dy GELU'(x), in fp64."""
    k = G.delta_taps()
    x = G.grid().reshape(1, 16, 16, 16).double().requires_grad_(True)
    y = R.filt_act(x, k, k)
    assert torch.equal(y.detach(), R.gelu_erf(x.detach()))
    assert torch.equal(R.filt_act_n3_closed_form(x.detach(), k, k), R.gelu_erf(x.detach()))
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    (dx,) = torch.autograd.grad(y, x, dy)
    assert float((dx - dy * G.gelu_grad64(x.detach())).abs().max()) < 1e-15
    # the metric's reference (erfc form, accurate in the negative tail) against the oracle's erf form: Phi to 1e-16 absolute
    xs = x.detach()
    assert float(((G.gelu64(xs) - R.gelu_erf(xs)).abs() / xs.abs().clamp_min(G.TINY)).max()) < 2.3e-16
    assert float(G.phi64(torch.tensor([-6.0]))) == pytest.approx(9.8658764503769e-10, rel=1e-12)


def test_fp32_reference_figures_and_the_restated_table_on_the_grid():
    worst = [0.0, 0.0]
    for n in sorted({C * S * S for S, C in G.filt_act_cases()}):
        u = G.grid(n)
        (rf, uf), (rb, ub), left_out = G.reference_figures(*G.torch_f32(u), u)
        assert [abs(v) for v in left_out] in ([], [float(np.float32(3e38))]), left_out
        ry, rdx = G.restated_f32(u)
        (tf, tuf), (tb, tub) = G.fwd_metric(ry, u), G.bwd_metric(rdx, u)
        print(f"grid({n}): fp32 F.gelu fwd {rf:.3e} at u={uf:.6g}, bwd {rb:.3e} at u={ub:.6g}; "
              f"restated table fwd {tf:.3e} at u={tuf:.6g}, bwd {tb:.3e} at u={tub:.6g}")
        assert rf <= G.gate_fwd() / 2 and rb <= G.gate_bwd() / 2
        assert tf < G.gate_fwd() and tb < G.gate_bwd()
        worst = [max(worst[0], rf), max(worst[1], rb)]
    assert worst[0] > 0.98 * G.REF_FWD and worst[1] > 0.98 * G.REF_BWD      # the constants are the measured figures, not padded


def test_restated_table_saturates_and_keeps_its_ends():
    tp, tg = G.piece_tables()
    assert tp.shape == (192, 4) and tp.dtype == np.float32
    u = torch.tensor([-3e38, -1e4, -6.5, -6.0, 6.0, 6.5, 1e4, 3e38])
    y, dx = G.restated_f32(u)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert G.fwd_metric(y, u)[0] < 1e-7 and G.bwd_metric(dx, u)[0] < 1e-7
    # one wrong coefficient in one tail piece is far outside the gate (what the whole-tensor rel-L2 on randn data never saw)
    bad = tp.copy()
    bad[3, 1] += np.float32(1e-5)
    ug = G.grid()
    yb = torch.from_numpy(ug.numpy() * G.piece_f32(ug.numpy(), bad))
    assert G.fwd_metric(yb, ug)[0] > 2 * G.gate_fwd()


@pytest.mark.parametrize("shape", G.GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fp32_reference_figures_of_the_fused_forms(shape):
    x, gamma, beta = G.gn_inputs(shape)
    assert float(x.double().sum()) == 0.0 and float(x.sum()) == 0.0
    u64, y64, d64 = G.gn_compose(x, gamma, beta, torch.float64)
    assert float(u64.min()) < -7 and float(u64.max()) > 7
    assert torch.equal(y64, R.gelu_erf(u64)) and float((d64 - G.gelu_grad64(u64)).abs().max()) < 1e-15
    u32, y32, d32 = G.gn_compose(x, gamma, beta, torch.float32)
    (rf, uf), (rb, ub), left_out = G.reference_figures(y32, d32, u64)
    assert not left_out
    ry, rdx = G.restated_f32(u32)
    (tf, tuf), (tb, tub) = G.fwd_metric(ry, u64), G.bwd_metric(rdx, u64)
    gf, gb = G.gate_gn(shape)
    print(f"{shape}: fp32 groupnorm1 + filt_act fwd {rf:.3e} at u={uf:.6g}, bwd {rb:.3e} at u={ub:.6g}; "
          f"restated table fwd {tf:.3e} at u={tuf:.6g}, bwd {tb:.3e} at u={tub:.6g}; gates {gf:.3e} / {gb:.3e}")
    assert rf <= gf / 2 and rb <= gb / 2
    assert rf > 0.98 * G.REF_GN[shape][0] and rb > 0.98 * G.REF_GN[shape][1]
    assert tf < gf and tb < gb
    # the form the kernel had first (piece and t from one fma, 16 u + 96) misses this backward gate: the rounding of that fma
    _, odx = G.restated_f32(u32, fused_index=True)
    ob, oub = G.bwd_metric(odx, u64)
    print(f"{shape}: restated table bwd with the fused index {ob:.3e} at u={oub:.6g}")
    assert ob > gb
