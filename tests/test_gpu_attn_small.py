"""The attention core at d in {16, 32}, L in {16, 32, 48, 64} (csrc/attn_small.hip: one wave per (batch, head) on the fp32
matrix pipe, whole score tile in registers, softmax and delta redone inside both backward launches) against the fp64 oracle and against the all-vector kernels
of csrc/attn.hip that served these shapes before (afd_debug_attn_rows(30) forces those, (31) is the default)."""
import math

import pytest
import torch

from conftest import check, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    return afdm, ops, gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(cfg, seed=None):
    B, heads, d, L = cfg
    C = heads * d
    g = _g(L + d if seed is None else seed)
    return torch.randn(B, 3 * C, L, generator=g), torch.randn(B, C, L, generator=g)


def _oracle(cfg, qkv, dy):
    """fp64: o (B, C, L), lse (B, heads, L) of the scaled scores, dqkv (B, 3C, L)."""
    B, heads, d, L = cfg
    C = heads * d
    q0 = qkv.double().requires_grad_(True)
    q, k, v = q0.split(C, dim=1)
    sh = lambda z: z.reshape(B, heads, d, L).transpose(2, 3)               # (B, h, L, d)
    s = sh(q) @ sh(k).transpose(-1, -2) / math.sqrt(d)
    o = (torch.softmax(s, dim=-1) @ sh(v)).transpose(2, 3).reshape(B, C, L)
    (g,) = torch.autograd.grad(o, q0, dy.double())
    return o.detach(), torch.logsumexp(s, dim=-1).detach(), g


def _run(A, cfg, qkv, dy):
    """afd_attn_fwd + afd_attn_bwd through the C ABI; o and the delta workspace start as NaN (the backward reads neither
    a stale delta nor anything it did not write)."""
    afdm, ops, dev = A
    B, heads, d, L = cfg
    C = heads * d
    P = lambda t: t.data_ptr()
    qd, gd = qkv.to(dev).contiguous(), dy.to(dev).contiguous()
    o = torch.full((B, C, L), float("nan"), device=dev)
    lse = torch.full((B, heads, L), float("nan"), device=dev)
    dqkv = torch.full((B, 3 * C, L), float("nan"), device=dev)
    ws = torch.full((B, heads, L), float("nan"), device=dev)
    lib = afdm.lib()
    lib.afd_attn_fwd(P(qd), P(o), P(lse), B, heads, d, L, ops._stream())
    lib.afd_attn_bwd(P(qd), P(o), P(gd), P(lse), P(dqkv), P(ws), B, heads, d, L, ops._stream())
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), dqkv.cpu()


def _run_mode(A, code, cfg, qkv, dy):
    lib = A[0].lib()
    try:
        lib.afd_debug_attn_rows(code)
        return _run(A, cfg, qkv, dy)
    finally:
        lib.afd_debug_attn_rows(31)


# sa3's and sa2's tiling; sa4's; L not a power of two; B * heads = 9: the last workgroup has one live wave; a single wave
CASES = [(1, 4, 32, 16), (3, 4, 32, 64), (2, 4, 16, 64), (2, 4, 16, 32), (1, 2, 32, 48), (3, 3, 16, 16), (1, 1, 32, 64)]


@pytest.mark.parametrize("cfg", CASES, ids=lambda c: "B%d_h%d_d%d_L%d" % c)
def test_small_attention_vs_fp64_and_vector_path(A, cfg):
    qkv, dy = _inputs(cfg)
    o64, lse64, g64 = _oracle(cfg, qkv, dy)
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    e = (rel_l2(o, o64), rel_l2(lse, lse64), rel_l2(dqkv, g64))
    print(f"attn_small {cfg}: fwd {e[0]:.2e} lse {e[1]:.2e} bwd {e[2]:.2e}")
    check("F10 attention small (L <= 64) fwd vs fp64", o, o64, TOL, cfg)
    check("F10 attention small (L <= 64) lse vs fp64", lse, lse64, TOL, cfg)
    check("F10 attention small (L <= 64) bwd vs fp64", dqkv, g64, TOL, cfg)
    # the kernels these shapes ran on before: same inputs, the gate between the fused and unfused attention blocks
    ov, lsev, dv = _run_mode(A, 30, cfg, qkv, dy)
    for name, a, b in (("o", o, ov), ("lse", lse, lsev), ("dqkv", dqkv, dv)):
        check("F10 attention small vs vector kernels", a, b, 5e-6, (cfg, name))


@pytest.mark.parametrize("cfg,spike", [((1, 4, 32, 64), 50), ((1, 4, 16, 16), 12)], ids=["d32_L64", "d16_L16"])
def test_small_attention_peaked_softmax(A, cfg, spike):
    """One key scaled x40 late in the sequence, Q x3: rows whose softmax is a one-hot next to rows that never see the spike."""
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = _inputs(cfg, seed=77)
    qkv[:, C:2 * C, spike] *= 40.0
    qkv[:, :C, :] *= 3.0
    o64, lse64, g64 = _oracle(cfg, qkv, dy)
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    check("F10 attention small peaked fwd vs fp64", o, o64, TOL, cfg)
    check("F10 attention small peaked lse vs fp64", lse, lse64, TOL, cfg)
    check("F10 attention small peaked bwd vs fp64", dqkv, g64, TOL, cfg)


@pytest.mark.parametrize("cfg", [(1, 4, 32, 64), (1, 4, 16, 16)], ids=["d32_L64", "d16_L16"])
def test_small_attention_row_shift_invariance(A, cfg):
    """Feature 0 of every query is 1, and feature 0 of every key grows by 30 sqrt(d): every score of every row moves by exactly
    +30, which the softmax does not see.  The fp32 scores then carry ~30 times the rounding error of the unshifted ones
    (half an ulp at 43 in the log2 domain is 1.9e-6, i.e. ~1.3e-6 relative on a probability): still under TOL."""
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = _inputs(cfg, seed=78)
    qkv[:, 0:C:d, :] = 1.0
    o64, _, _ = _oracle(cfg, qkv, dy)
    o_base, lse_base, _ = _run(A, cfg, qkv, dy)
    shifted = qkv.clone()
    shifted[:, C:2 * C:d, :] += 30.0 * math.sqrt(d)
    o, lse, dqkv = _run(A, cfg, shifted, dy)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    print(f"attn_small row shift {cfg}: vs fp64 {rel_l2(o, o64):.2e}, vs unshifted {rel_l2(o, o_base):.2e}")
    check("F10 attention small +30 row shift vs fp64", o, o64, TOL, cfg)
    check("F10 attention small +30 row shift vs unshifted", o, o_base, TOL, cfg)
    check("F10 attention small +30 row shift lse", lse - 30.0, lse_base, TOL, cfg)


def test_small_attention_is_deterministic(A):
    cfg = (3, 4, 32, 64)
    qkv, dy = _inputs(cfg)
    r0, r1 = _run(A, cfg, qkv, dy), _run(A, cfg, qkv, dy)
    assert all(torch.equal(a, b) for a, b in zip(r0, r1))


@pytest.mark.parametrize("cfg", [(2, 4, 64, 48), (2, 2, 8, 100), (3, 4, 16, 256)], ids=lambda c: "B%d_h%d_d%d_L%d" % c)
def test_small_attention_rule_leaves_other_shapes_alone(A, cfg):
    """d = 64, L not a multiple of 16 and L = 256 keep their kernels: the same bits whether the new rule is on or off."""
    qkv, dy = _inputs(cfg)
    off, on = _run_mode(A, 30, cfg, qkv, dy), _run_mode(A, 31, cfg, qkv, dy)
    assert all(torch.equal(a, b) for a, b in zip(off, on))
