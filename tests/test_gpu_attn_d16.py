"""The attention core at d = 16, L % 256 == 0 (csrc/attn_mfma.hip: attn_fwd_pv<16> and attn_bwd_fused<16>: P V, dV, dK and dQ
as two-piece fp16 products on the matrix pipe, the backward in one pass) against the fp64 oracle and against the round-2
kernels that served these shapes before (afd_debug_attn_rows(40) forces those, (41) is the default)."""
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
    """afd_attn_fwd + afd_attn_bwd through the C ABI; o, lse, dqkv and the delta workspace start as NaN (the backward reads
    neither a stale delta nor anything it did not write, and accumulates dQ over key blocks from its own first store)."""
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
        lib.afd_debug_attn_rows(41)


# one workgroup, one key block; two key blocks (dQ accumulated in place, a second forward workgroup per head) with a head count
# that is not a power of two; sa1's tiling
CASES = [(1, 1, 16, 256), (2, 3, 16, 512), (3, 4, 16, 256)]
_ids = lambda c: "B%d_h%d_d%d_L%d" % c
_BASE = {}


def _base(cfg):
    """Inputs and the fp64 oracle of a case, computed once and shared (never modified: callers clone)."""
    if cfg not in _BASE:
        qkv, dy = _inputs(cfg)
        _BASE[cfg] = (qkv, dy) + _oracle(cfg, qkv, dy)
    return _BASE[cfg]


@pytest.mark.parametrize("cfg", CASES, ids=_ids)
def test_d16_attention_vs_fp64_and_round2_kernels(A, cfg):
    qkv, dy, o64, lse64, g64 = _base(cfg)
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    e = (rel_l2(o, o64), rel_l2(lse, lse64), rel_l2(dqkv, g64))
    print(f"attn_d16 {cfg}: fwd {e[0]:.2e} lse {e[1]:.2e} bwd {e[2]:.2e}")
    check("F10 attention d16 (matrix-pipe P V, one-pass bwd) fwd vs fp64", o, o64, TOL, cfg)
    check("F10 attention d16 (matrix-pipe P V, one-pass bwd) lse vs fp64", lse, lse64, TOL, cfg)
    check("F10 attention d16 (matrix-pipe P V, one-pass bwd) bwd vs fp64", dqkv, g64, TOL, cfg)
    # the kernels these shapes ran on before: same inputs, the cross-kernel gate of test_gpu_attn_small.py
    ov, lsev, dv = _run_mode(A, 40, cfg, qkv, dy)
    for name, a, b in (("o", o, ov), ("lse", lse, lsev), ("dqkv", dqkv, dv)):
        check("F10 attention d16 vs round-2 kernels", a, b, 5e-6, (cfg, name))


def test_d16_running_scales_lowered_mid_stream(A):
    """V and dO of tokens >= 320 are 2^12 times larger (L = 512): the power-of-two scales of V (forward), dO and dS (backward)
    are lowered in the middle of the stream -- in the forward's sixth key stage, in the backward's second key block and, per
    key block, in its sixth query stage -- and the accumulators carried over."""
    cfg = (2, 3, 16, 512)
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = (t.clone() for t in _base(cfg)[:2])
    qkv[:, 2 * C:, 320:] *= 4096.0
    dy[:, :, 320:] *= 4096.0
    o64, lse64, g64 = _oracle(cfg, qkv, dy)
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    print(f"attn_d16 scales 2^12 from token 320: fwd {rel_l2(o, o64):.2e} lse {rel_l2(lse, lse64):.2e} bwd {rel_l2(dqkv, g64):.2e}")
    check("F10 attention d16 scales lowered mid-stream fwd", o, o64, TOL, cfg)
    check("F10 attention d16 scales lowered mid-stream lse", lse, lse64, TOL, cfg)
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        check("F10 attention d16 scales lowered mid-stream bwd", dqkv[:, sl], g64[:, sl], TOL, (cfg, name))


@pytest.mark.parametrize("sv,sg", [(1e-20, 1e15), (1e15, 1e-20)], ids=["V1e-20_dO1e15", "V1e15_dO1e-20"])
def test_d16_tiny_and_huge_operands(A, sv, sg):
    """V scaled by sv and dO by sg (1e-20 and 1e+15, both ways round); Q and K are left alone, so the softmax is the same.
    o and dV are linear in one of them, dQ and dK in their product: the outputs divided back are compared with the fp64
    oracle of the unscaled inputs."""
    cfg = (3, 4, 16, 256)
    B, heads, d, L = cfg
    C = heads * d
    qkv0, dy0, o64, lse64, g64 = _base(cfg)
    qkv, dy = qkv0.clone(), dy0.clone()
    qkv[:, 2 * C:] *= sv
    dy *= sg
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    back = {"o": o.double() / sv, "dq": dqkv[:, :C].double() / (sv * sg), "dk": dqkv[:, C:2 * C].double() / (sv * sg),
            "dv": dqkv[:, 2 * C:].double() / sg}
    want = {"o": o64, "dq": g64[:, :C], "dk": g64[:, C:2 * C], "dv": g64[:, 2 * C:]}
    print(f"attn_d16 V x {sv:g}, dO x {sg:g}: " + " ".join(f"{k} {rel_l2(back[k], want[k]):.2e}" for k in back))
    check("F10 attention d16 tiny / huge V, dO: lse", lse, lse64, TOL, cfg)
    for k in back:
        check("F10 attention d16 tiny / huge V, dO", back[k], want[k], TOL, (cfg, k, sv, sg))


def _gate_at_twice_round2(A, tag, cfg, qkv, dy):
    """New kernels against fp64, gated at twice what the round-2 kernels (code 40) give on the same inputs."""
    o64, lse64, g64 = _oracle(cfg, qkv, dy)
    new, old = _run(A, cfg, qkv, dy), _run_mode(A, 40, cfg, qkv, dy)
    assert all(torch.isfinite(t).all() for t in new)
    res = []
    for name, a, b, w in zip(("o", "lse", "dqkv"), new, old, (o64, lse64, g64)):
        e_new, e_old = rel_l2(a, w), rel_l2(b, w)
        print(f"attn_d16 {tag} {cfg} {name}: new {e_new:.2e}  round-2 {e_old:.2e}")
        res.append((name, e_new, e_old))
    for name, e_new, e_old in res:
        assert e_new <= 2.0 * e_old, (tag, name, e_new, e_old)


def test_d16_peaked_softmax(A):
    """One key scaled x40 late in the sequence (in the second key block), Q x3: rows whose softmax is a one-hot next to rows
    that never see the spike.  These kernels take exp2(S - lse) from the stored lse, as the round-2 ones do, so the error on
    peaked rows follows lse's rounding and is not promised to the 1e-5 gate; the gate is twice the round-2 kernels' error on the same inputs
    (a different summation order).  Measured on MI355X (rel-L2 against fp64, new | round-2):
    o 2.36e-7 | 2.78e-7, lse 8.55e-8 | 8.53e-8, dqkv 5.56e-6 | 6.88e-6."""
    cfg = (2, 3, 16, 512)
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = _inputs(cfg, seed=77)
    qkv[:, C:2 * C, 400] *= 40.0
    qkv[:, :C, :] *= 3.0
    _gate_at_twice_round2(A, "peaked", cfg, qkv, dy)


def test_d16_row_shift(A):
    """Feature 0 of every query is 1 and feature 0 of every key grows by 30 sqrt(d): every score of every row moves by exactly
    +30, which the softmax does not see, while the fp32 scores carry ~30 times the rounding error.  Gate: twice the round-2
    kernels' error on the same inputs.  Measured on MI355X (rel-L2 against fp64, new | round-2):
    o 2.66e-6 | 2.68e-6, lse 4.98e-8 | 4.02e-8, dqkv 2.30e-6 | 8.39e-6 (dQ is taken against K - mean(K): 4.91e-5 without)."""
    cfg = (2, 3, 16, 512)
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = _inputs(cfg, seed=78)
    qkv[:, 0:C:d, :] = 1.0
    qkv[:, C:2 * C:d, :] += 30.0 * math.sqrt(d)
    _gate_at_twice_round2(A, "row shift +30", cfg, qkv, dy)


def test_d16_attention_is_deterministic(A):
    cfg = (2, 3, 16, 512)
    qkv, dy = _base(cfg)[:2]
    r0, r1 = _run(A, cfg, qkv, dy), _run(A, cfg, qkv, dy)
    assert all(torch.equal(a, b) for a, b in zip(r0, r1))


@pytest.mark.parametrize("cfg", [(2, 4, 8, 256), (2, 4, 16, 64), (2, 4, 16, 192)], ids=_ids)
def test_d16_rule_leaves_other_shapes_alone(A, cfg):
    """d = 8, L = 64 and L not a multiple of 256 keep their kernels: the same bits whether the new rule is on or off."""
    qkv, dy = _inputs(cfg)
    off, on = _run_mode(A, 40, cfg, qkv, dy), _run_mode(A, 41, cfg, qkv, dy)
    assert all(torch.equal(a, b) for a, b in zip(off, on))
