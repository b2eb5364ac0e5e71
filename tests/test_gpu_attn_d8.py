"""The attention core at d = 8, L % 256 == 0 (csrc/attn_mfma.hip: attn_fwd_pv<8> and attn_bwd_fused<8, 2>, the default of
sa1, sa5 and sa6) against the fp64 oracle and against the round-2 kernels that served these shapes before
(afd_debug_attn_rows(20) forces those, (21) is the default).  The d = 8 counterpart of tests/test_gpu_attn_d16.py: the
backward instance has TWO key tiles per wave (a workgroup walks the keys 256 at a time, not 128), so the running scales
of V, Q, dO, K and dS move at other places than at d = 16.

Geometry read from the kernels (kTK = 64):
  attn_fwd_pv<8>         a workgroup owns 256 queries of one (batch, head) and streams the keys in stages of 64; the V scale
                         is the workgroup's and is looked at once per stage.
  attn_bwd_fused<8, 2>   one workgroup per (batch, head) walks key blocks of 256 (wave w: keys 64 w .. 64 w + 63 of the
                         block, two tiles of 32); per key block it streams the queries in stages of 64.  Q and dO scales:
                         the workgroup's, running over all stages of all key blocks; K scale: per wave and key block;
                         dS scale: restarted per key block, running over its query stages."""
import math

import pytest
import torch

from conftest import check, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
FAM = "F10 attention d8 (matrix-pipe P V, one-pass bwd)"


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    yield afdm, ops, gpu
    afdm.lib().afd_debug_attn_rows(21)


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
        lib.afd_debug_attn_rows(21)


# one forward workgroup, one key block; two key blocks (dQ accumulated in place, a second forward workgroup per head) with a
# head count that is not a power of two; sa6's tiling: four key blocks, sixteen stages
CASES = [(1, 1, 8, 256), (2, 3, 8, 512), (1, 4, 8, 1024)]
_ids = lambda c: "B%d_h%d_d%d_L%d" % c
_BASE = {}


def _base(cfg):
    """Inputs and the fp64 oracle of a case, computed once and shared (never modified: callers clone)."""
    if cfg not in _BASE:
        qkv, dy = _inputs(cfg)
        _BASE[cfg] = (qkv, dy) + _oracle(cfg, qkv, dy)
    return _BASE[cfg]


@pytest.mark.parametrize("cfg", CASES, ids=_ids)
def test_d8_attention_vs_fp64_and_round2_kernels(A, cfg):
    qkv, dy, o64, lse64, g64 = _base(cfg)
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    e = (rel_l2(o, o64), rel_l2(lse, lse64), rel_l2(dqkv, g64))
    print(f"attn_d8 {cfg}: fwd {e[0]:.2e} lse {e[1]:.2e} bwd {e[2]:.2e}")
    check(FAM + " fwd vs fp64", o, o64, TOL, cfg)
    check(FAM + " lse vs fp64", lse, lse64, TOL, cfg)
    check(FAM + " bwd vs fp64", dqkv, g64, TOL, cfg)
    # the kernels these shapes ran on before: same inputs, the cross-kernel gate of test_gpu_attn_small.py
    ov, lsev, dv = _run_mode(A, 20, cfg, qkv, dy)
    for name, a, b in (("o", o, ov), ("lse", lse, lsev), ("dqkv", dqkv, dv)):
        check("F10 attention d8 vs round-2 kernels", a, b, 5e-6, (cfg, name))


@pytest.mark.parametrize("cfg", [(2, 3, 8, 512), (1, 4, 8, 1024)], ids=_ids)
def test_d8_running_scales_lowered_mid_stream(A, cfg):
    """V and dO of tokens >= 320 are 2^12 times larger.  Where that falls in this instantiation (module docstring):
      forward   320 = 5 * 64: the sixth key stage of every query workgroup (of 8 stages at L = 512, of 16 at L = 1024) -- the V
                scale is lowered there and five stages of V-weighted sums are carried over;
      backward  key blocks are 256 wide, so 320 lies INSIDE the second key block (its wave 1 starts there; wave 0 holds only
                small V, waves 1..3 only large) -- not on a block boundary, so the threshold of the d = 16 test is kept.  The
                first key block sees the jump of dO in its sixth query stage: the dO scale (workgroup, running) and the dS
                scale (per key block) are lowered there and accV / accK carried over; from the second key block on the dO
                scale is already low while the dS scale, restarted per key block, is lowered again in the sixth query stage
                (the bound |V|_1 max|dO| + max|delta| grows with dO).  At L = 1024 the third and fourth key blocks hold only
                large V and repeat that with a 2^12 larger |V|_1."""
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = (t.clone() for t in _base(cfg)[:2])
    qkv[:, 2 * C:, 320:] *= 4096.0
    dy[:, :, 320:] *= 4096.0
    o64, lse64, g64 = _oracle(cfg, qkv, dy)
    o, lse, dqkv = _run(A, cfg, qkv, dy)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv).all()
    print(f"attn_d8 {cfg} scales 2^12 from token 320: fwd {rel_l2(o, o64):.2e} lse {rel_l2(lse, lse64):.2e} bwd {rel_l2(dqkv, g64):.2e}")
    check("F10 attention d8 scales lowered mid-stream fwd", o, o64, TOL, cfg)
    check("F10 attention d8 scales lowered mid-stream lse", lse, lse64, TOL, cfg)
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        check("F10 attention d8 scales lowered mid-stream bwd", dqkv[:, sl], g64[:, sl], TOL, (cfg, name))


@pytest.mark.parametrize("sv,sg", [(1e-20, 1e15), (1e15, 1e-20)], ids=["V1e-20_dO1e15", "V1e15_dO1e-20"])
def test_d8_tiny_and_huge_operands(A, sv, sg):
    """V scaled by sv and dO by sg (1e-20 and 1e+15, both ways round); Q and K are left alone, so the softmax is the same.
    o and dV are linear in one of them, dQ and dK in their product: the outputs divided back are compared with the fp64
    oracle of the unscaled inputs."""
    cfg = (2, 3, 8, 512)
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
    print(f"attn_d8 V x {sv:g}, dO x {sg:g}: " + " ".join(f"{k} {rel_l2(back[k], want[k]):.2e}" for k in back))
    check("F10 attention d8 tiny / huge V, dO: lse", lse, lse64, TOL, cfg)
    for k in back:
        check("F10 attention d8 tiny / huge V, dO", back[k], want[k], TOL, (cfg, k, sv, sg))


def _gate_at_twice_round2(A, tag, cfg, qkv, dy):
    """New kernels against fp64, gated at twice what the round-2 kernels (code 20) give on the same inputs."""
    o64, lse64, g64 = _oracle(cfg, qkv, dy)
    new, old = _run(A, cfg, qkv, dy), _run_mode(A, 20, cfg, qkv, dy)
    assert all(torch.isfinite(t).all() for t in new)
    res = []
    for name, a, b, w in zip(("o", "lse", "dqkv"), new, old, (o64, lse64, g64)):
        e_new, e_old = rel_l2(a, w), rel_l2(b, w)
        print(f"attn_d8 {tag} {cfg} {name}: new {e_new:.2e}  round-2 {e_old:.2e}")
        res.append((name, e_new, e_old))
    for name, e_new, e_old in res:
        assert e_new <= 2.0 * e_old, (tag, name, e_new, e_old)


def test_d8_k_of_second_key_block_times_4(A):
    """K of keys 256 .. 511 (the backward's second key block, every wave of it) is 4 times larger: the per-wave K scale of the
    second block sits two powers of two below the first block's, while the running Q scale does not move.  This changes the
    softmax (the late keys' scores spread four times wider), so the error follows lse's rounding as in the peaked case; gate:
    twice the round-2 kernels' error on the same inputs.  Measured on MI355X (rel-L2 against fp64, new | round-2):
    o 4.21e-7 | 4.53e-7, lse 6.62e-8 | 5.39e-8, dqkv 1.38e-6 | 1.04e-6."""
    cfg = (2, 3, 8, 512)
    C = cfg[1] * cfg[2]
    qkv, dy = _inputs(cfg, seed=79)
    qkv[:, C:2 * C, 256:] *= 4.0
    _gate_at_twice_round2(A, "K x4 from key 256", cfg, qkv, dy)


def test_d8_q_of_late_tokens_times_4(A):
    """Q of tokens >= 384 (the seventh query stage on) is 4 times larger: the running Q scale is lowered in the seventh stage
    of the FIRST key block and dK's sums carried over, and stays low through the second key block, whose per-wave K scales
    are unchanged -- the two scales that meet in dQ's and dK's unscaling are driven apart.  Changes the softmax of the late
    rows; gate: twice the round-2 kernels' error on the same inputs.  Measured on MI355X (rel-L2 against fp64, new | round-2):
    o 4.73e-7 | 5.63e-7, lse 9.03e-8 | 5.27e-8, dqkv 1.25e-6 | 1.36e-6."""
    cfg = (2, 3, 8, 512)
    C = cfg[1] * cfg[2]
    qkv, dy = _inputs(cfg, seed=80)
    qkv[:, :C, 384:] *= 4.0
    _gate_at_twice_round2(A, "Q x4 from token 384", cfg, qkv, dy)


def test_d8_peaked_softmax(A):
    """One key scaled x40 late in the sequence (in the second key block), Q x3: rows whose softmax is a one-hot next to rows
    that never see the spike.  These kernels take exp2(S - lse) from the stored lse, as the round-2 ones do, so the error on
    peaked rows follows lse's rounding and is not promised to the 1e-5 gate; the gate is twice the round-2 kernels' error on
    the same inputs (a different summation order).  Measured on MI355X (rel-L2 against fp64, new | round-2):
    o 2.08e-7 | 2.45e-7, lse 6.81e-8 | 6.79e-8, dqkv 4.64e-6 | 6.15e-6."""
    cfg = (2, 3, 8, 512)
    C = cfg[1] * cfg[2]
    qkv, dy = _inputs(cfg, seed=77)
    qkv[:, C:2 * C, 400] *= 40.0
    qkv[:, :C, :] *= 3.0
    _gate_at_twice_round2(A, "peaked", cfg, qkv, dy)


def test_d8_row_shift(A):
    """Feature 0 of every query is 1 and feature 0 of every key grows by 30 sqrt(d): every score of every row moves by exactly
    +30, which the softmax does not see, while the fp32 scores carry ~30 times the rounding error.  Gate: twice the round-2
    kernels' error on the same inputs.  Measured on MI355X (rel-L2 against fp64, new | round-2):
    o 1.82e-6 | 1.83e-6, lse 4.18e-8 | 3.81e-8, dqkv 2.24e-6 | 7.66e-6 (dQ is taken against K - mean(K), as at d = 16; without,
    this test measured 3.48e-5 and failed its gate)."""
    cfg = (2, 3, 8, 512)
    B, heads, d, L = cfg
    C = heads * d
    qkv, dy = _inputs(cfg, seed=78)
    qkv[:, 0:C:d, :] = 1.0
    qkv[:, C:2 * C:d, :] += 30.0 * math.sqrt(d)
    _gate_at_twice_round2(A, "row shift +30", cfg, qkv, dy)


def test_d8_attention_is_deterministic(A):
    cfg = (2, 3, 8, 512)
    qkv, dy = _base(cfg)[:2]
    r0, r1 = _run(A, cfg, qkv, dy), _run(A, cfg, qkv, dy)
    assert all(torch.equal(a, b) for a, b in zip(r0, r1))


@pytest.mark.parametrize("cfg", [(2, 4, 8, 64), (2, 4, 8, 192)], ids=_ids)
def test_d8_rule_leaves_other_shapes_alone(A, cfg):
    """L = 64 and L not a multiple of 256 keep their kernels: the same bits under codes 20 and 21."""
    qkv, dy = _inputs(cfg)
    off, on = _run_mode(A, 20, cfg, qkv, dy), _run_mode(A, 21, cfg, qkv, dy)
    assert all(torch.equal(a, b) for a, b in zip(off, on))
