"""The AdamW step kernel on the MI355X, every form of it (lr by value or from ctl, with or without the fused EMA, 16-byte or
scalar accesses), against an independent restatement of one AdamW element in numpy float32: one operation per line, in
optim.hip's order, compared bit for bit (the int32 view).  The other optimiser tests compare one entry point with another;
this one is the arithmetic's own check, and the only one whose sizes make the grid-stride loops take a second trip."""
import numpy as np
import pytest
import torch

from test_gpu_clip import _ctl
from test_gpu_ema import _adam_inputs, _rule

pytestmark = pytest.mark.gpu
F = np.float32
LR, B1, B2, EPS, WD, GRAD_SCALE = 3e-4, 0.9, 0.999, 1e-8, 0.01, 0.5
COEF = 0.25                      # ctl.coef: grad_scale * (float)coef is then a real product, not a multiply by 1
BETA = 0.995
FORMS = {"plain": (False, False), "ema": (False, True), "ctl": (True, False), "ctl+ema": (True, True)}      # (ctl, ema)


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def adamw_oracle(p, g, m, v, lr, gscale, bc1, bc2):
    """One AdamW step over fp32 arrays: every line is one fp32 operation, hence one rounding.  Returns the new p, m, v."""
    lr, gscale, bc1, bc2, b1, b2, eps, wd, one = F(lr), F(gscale), F(bc1), F(bc2), F(B1), F(B2), F(EPS), F(WD), F(1.0)
    decay = lr * wd
    decay = one - decay
    step_size = lr / bc1
    inv_sqrt_bc2 = np.sqrt(bc2)
    inv_sqrt_bc2 = one / inv_sqrt_bc2
    omb1 = one - b1
    omb2 = one - b2
    gi = g * gscale
    pi = p * decay
    mi = gi - m
    mi = mi * omb1
    mi = m + mi
    vi = v * b2
    sq = gi * gi
    sq = sq * omb2
    vi = vi + sq
    denom = np.sqrt(vi)
    denom = denom * inv_sqrt_bc2
    denom = denom + eps
    q = mi / denom
    q = step_size * q
    pn = pi - q
    assert all(a.dtype == np.float32 for a in (pn, mi, vi))
    return pn, mi, vi


def same_bits(name, got, want, ctx):
    got, want = got.cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (name, ctx, f"{bad.size} elements differ, the first at {bad[0]}: "
                           f"{got[bad[0]:bad[0] + 1].view(np.float32)[0]!r} != {want[bad[0]:bad[0] + 1].view(np.float32)[0]!r}")


def run_form(A, form, n, offset, tail, steps, calls=0, start=1):
    """`steps` consecutive updates through the entry point of `form`; after each, p, m, v and ema against the oracle."""
    afdm, dev = A
    from afdm import ops
    L, s = afdm.lib(), ops._stream()
    use_ctl, use_ema = FORMS[form]
    n_ema = n + tail
    p, g, m, v, ema = _adam_inputs(n_ema, dev, offset, seed=13 * (n % 9973) + 2 * offset + tail)
    assert p.data_ptr() % 16 == 4 * offset
    state = torch.zeros(4, device=dev)
    es = torch.tensor([calls, 0], device=dev, dtype=torch.int32)
    ctl = _ctl(dev, LR, coef=COEF)
    if use_ctl:
        lr, gscale = F(LR), F(GRAD_SCALE) * F(COEF)                                # the kernel's (float)ctl.lr and its fp32 product
    else:
        lr, gscale = F(LR), F(GRAD_SCALE)
    hp, hm, hv = (x.cpu().numpy() for x in (p, m, v))
    for k in range(steps):
        ctx = (form, n, offset, tail, k)
        if k:
            g.copy_(torch.randn(n_ema, device=dev, generator=torch.Generator(device=dev).manual_seed(n % 9973 + k)))
        g0, ema0 = g.clone(), ema.clone()
        ema_args = (ema.data_ptr(), n_ema, es.data_ptr(), BETA, float(1.0 - BETA)) if use_ema else (None, 0, None, 0.0, 0.0)
        if use_ema:
            L.afd_adamw_ema_tick(state.data_ptr(), B1, B2, es.data_ptr(), start, s)
        else:
            L.afd_adamw_tick(state.data_ptr(), B1, B2, s)
        bufs = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr())
        if use_ctl:
            L.afd_adamw_ctl_step(*bufs, ctl.data_ptr(), B1, B2, EPS, WD, GRAD_SCALE, *ema_args, s)
        elif use_ema:
            L.afd_adamw_ema_step(*bufs, LR, B1, B2, EPS, WD, GRAD_SCALE, *ema_args, s)
        else:
            L.afd_adamw_step(*bufs, LR, B1, B2, EPS, WD, GRAD_SCALE, s)
        torch.cuda.synchronize()
        step, bc1, bc2, _ = state.cpu().tolist()                                   # the tick's powers are not under test here
        assert step == k + 1
        hg = g0.cpu().numpy()
        hp[:n], hm[:n], hv[:n] = adamw_oracle(hp[:n], hg[:n], hm[:n], hv[:n], lr, gscale, bc1, bc2)      # beyond n: untouched
        same_bits("p", p, hp, ctx)
        same_bits("m", m, hm, ctx)
        same_bits("v", v, hv, ctx)
        assert torch.equal(g, g0), ctx
        if use_ema:
            copy_ = calls + k < start
            assert es.tolist() == [calls + k + 1, int(copy_)], ctx
            same_bits("ema", ema, _rule(ema0, torch.from_numpy(hp).to(dev), copy_, BETA).cpu().numpy(), ctx)
        else:
            assert torch.equal(ema, ema0), ctx


# no quad, a partial quad, exactly one, one and a remainder, many and a remainder
@pytest.mark.parametrize("offset", (0, 1))                  # the 16-byte form and the scalar form
@pytest.mark.parametrize("n", (1, 3, 4, 5, 4099))
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_bit_exact_against_the_fp32_restatement(A, form, n, offset):
    for tail in (0, 5):
        run_form(A, form, n, offset, tail, steps=3)         # the EMA copies, then blends, then blends


# gs_grid caps the grid at 32768 x 256 threads: the stride loop repeats only beyond 8 388 608 items (elements in the scalar
# form, quads in the 16-byte form).  One blending step each, a partial quad and an EMA tail included.
@pytest.mark.parametrize("form, n, offset", (("plain", 8_388_608 + 5, 1), ("ctl+ema", 8_388_608 + 5, 1),
                                             ("ctl+ema", 33_554_432 + 7, 0)))
def test_grid_stride_second_trip_bit_exact(A, form, n, offset):
    run_form(A, form, n, offset, tail=5, steps=1, calls=3)
