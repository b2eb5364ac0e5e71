"""Both GELU implementations per element over their whole domain (cases, metric and gates: tests/gelu_cases.py).

csrc/filt.hip reads 192 cubic pieces on [-6, 6) clamped with fmed3 (`gelu_piece`, reached through filt_act_fwd_n3 /
filt_act_bwd_n3 with delta taps, which turn the fused op into y = GELU(x), dx = dy GELU'(x)); csrc/common.h evaluates the
Abramowitz-Stegun erf (`gelu_erf`, `gelu_erf_grad`, reached through ops.Gelu).  Every element is gated, the saturated region
beyond +-6 and a denormal included; a non-finite output counts as an infinite error."""
import pytest
import torch

import gelu_cases as G
from conftest import note

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    return afdm, ops, gpu


def _gate(family, value, at, gate, detail):
    note(f"{family} (gate {gate:.2e})", value, f"{detail} u={at:.9g}")
    print(f"{family}: {value:.3e} at u={at:.9g} [{detail}], gate {gate:.3e}")
    return value < gate


@pytest.mark.parametrize("S,C", G.filt_act_cases(), ids=[f"S{S}_C{C}" for S, C in G.filt_act_cases()])
def test_table_gelu_per_element_through_filt_act(A, S, C):
    """filt_act_fwd_n3<S, FULL> / filt_act_bwd_n3<S, FULL> (FULL = planes % (64 / S) == 0, else the dead-lane variants): the
    table lookup at every piece boundary and its fp32 neighbours, the fmed3 clamp at +-6, the saturation beyond, zeros and a
    denormal."""
    afdm, ops, dev = A
    assert afdm.lib().afd_filt_act_workspace_bytes(1, C, S, S, 3, 0) == 0          # the fast path, not the general-N kernels
    u = G.grid(C * S * S).reshape(1, C, S, S)
    t = ops.Taps(G.delta_taps())
    x = u.to(dev).requires_grad_(True)
    y = ops.FiltAct.apply(x, t, t)
    (dx,) = torch.autograd.grad(y, x, torch.ones_like(y))
    full = "FULL" if C % max(64 // S, 1) == 0 else "dead lanes"
    f, uf = G.fwd_metric(y.detach().cpu(), u)
    b, ub = G.bwd_metric(dx.cpu(), u)
    ok_f = _gate("GELU table fwd |y - GELU64| / |u|", f, uf, G.gate_fwd(), f"S={S} C={C} {full}")
    ok_b = _gate("GELU table bwd |dx - GELU'64|", b, ub, G.gate_bwd(), f"S={S} C={C} {full}")
    assert ok_f and ok_b, (S, C, f, uf, b, ub)


def _gn_run(A, shape):
    afdm, ops, dev = A
    B, C, H, W = shape
    gn = bool(afdm.lib().afd_filt_act_fwd_gn_supported(C, H, W, 3))
    assert gn == (shape != (1, 64, 32, 32))
    x, gamma, beta = G.gn_inputs(shape)
    u64, _, _ = G.gn_compose(x, gamma, beta, torch.float64)
    t = ops.Taps(G.delta_taps())
    res = torch.zeros(shape, device=dev, requires_grad=True)
    y = ops.GroupNormFiltAct.apply(x.to(dev), gamma.to(dev), beta.to(dev), res, t, t)
    (dres,) = torch.autograd.grad(y, res, torch.ones_like(y))
    return "_gn" if gn else "stats + act", u64, y.detach().cpu(), dres.cpu()


@pytest.mark.parametrize("shape", G.GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_table_gelu_per_element_through_groupnorm_filt_act_fwd(A, shape):
    """The sample-resident `_gn` kernel (filt_act_fwd_n3<S, true, STATS>, one 1024-thread workgroup per sample) at the UNet's
    three sites, and the stats + act form at 64x32x32.  u is the fp64 pre-activation."""
    form, u64, y, _ = _gn_run(A, shape)
    f, uf = G.fwd_metric(y, u64)
    assert _gate(f"GELU table fwd through GroupNorm [{form}]", f, uf, G.gate_gn(shape)[0], shape), (shape, f, uf)


@pytest.mark.parametrize("shape", G.GN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_table_gelu_per_element_through_groupnorm_filt_act_bwd(A, shape):
    """filt_act_bwd_n3<S, true, GNB> at the same sites and filt_act_bwd_n3<32, true> behind the statistics pass: the zero
    residual's gradient under dy = 1 is GELU'(u), u the fp64 pre-activation.

    This is the case that found the index rounding of the table's first form (piece and t from one fma, 16 u + 96): 2.61e-7
    at u = 0.539 (`_gn`) and 2.79e-7 at u = 0.279 (stats + act) on an MI355X against the gate of 2 x 1.24e-7 = 2.48e-7.  With
    piece and t from the exact product 16 u: 1.81e-7 and 1.97e-7 ("GELU per element")."""
    form, u64, _, dres = _gn_run(A, shape)
    b, ub = G.bwd_metric(dres, u64)
    assert _gate(f"GELU table bwd through GroupNorm [{form}]", b, ub, G.gate_gn(shape)[1], shape), (shape, b, ub)


def test_erf_gelu_per_element_aligned_and_offset(A):
    """ops.Gelu (gelu_fwd_k / gelu_bwd_k): the vector form on a 16-byte aligned tensor and the scalar form through a view that
    starts 4 bytes past a 16-byte boundary (n4 = 0 in afd_gelu_fwd / _bwd) -- same grid, bit-equal results."""
    _, ops, dev = A
    u = G.grid()
    n = u.numel()
    got = {}
    for name, off in (("aligned", 0), ("offset", 1)):
        buf = torch.zeros(n + 8, device=dev)
        assert buf.data_ptr() % 16 == 0
        x = buf[off:off + n]
        x.copy_(u)
        assert x.data_ptr() % 16 == 4 * off and x.is_contiguous()
        x.requires_grad_(True)
        y = ops.Gelu.apply(x)
        if off:                                     # the backward's three pointers: keep all of them off the boundary
            dyb = torch.ones(n + 8, device=dev)
            dy = dyb[off:off + n]
        else:
            dy = torch.ones(n, device=dev)
        (dx,) = torch.autograd.grad(y, x, dy)
        got[name] = (y.detach().cpu(), dx.cpu())
        f, uf = G.fwd_metric(got[name][0], u)
        b, ub = G.bwd_metric(got[name][1], u)
        ok_f = _gate("GELU erf fwd |y - GELU64| / |u|", f, uf, G.gate_fwd(), name)
        ok_b = _gate("GELU erf bwd |dx - GELU'64|", b, ub, G.gate_bwd(), name)
        assert ok_f and ok_b, (name, f, uf, b, ub)
    assert torch.equal(got["aligned"][0], got["offset"][0]) and torch.equal(got["aligned"][1], got["offset"][1])
