"""Shared cases of the per-element GELU tests (test_gelu_cases_host.py on the CPU, test_gpu_gelu_domain.py on the device).

The project evaluates GELU and GELU' in two ways: csrc/filt.hip reads 192 cubic pieces on [-6, 6) (`gelu_piece`, clamped with
fmed3 at both ends; PIECES and SCALE below restate its constants, OFFSET is half the table), csrc/common.h goes through the Abramowitz-Stegun erf (`gelu_erf`, `gelu_erf_grad`).  Both promise the
ABSOLUTE error of Phi and of GELU' (the 1 + erf cancellation rules out relative accuracy in the negative tail), so the metric is

    forward   |y - GELU64(u)| / max(|u|, 2^-126)        backward (dy = 1)   |dx - GELU'64(u)|

per element, no element left out.  A gate is 2 x the worst value plain fp32 torch reaches on the CPU for the same composition on
the same inputs (REF_* below, measured by test_gelu_cases_host.py, which also asserts that they still hold); the factor 2 covers
another evaluation order, fma contraction and the pieces' interpolation error.  (It did not cover the index rounding of the
table's first form, 16 u + 96 in one fma: see piece_f32 and DESIGN.md, "GELU per element".)"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_ops as R

TINY = 2.0 ** -126
PIECES, SCALE, OFFSET = 192, 16.0, 96.0                      # csrc/filt.hip: kGeluPieces, kGeluScale, kGeluOffset
GRID_N = 4096                                                # one (1, C, S, S) tensor with C * S * S = 4096 at every fast-path S

# ---- measured on the CPU by test_gelu_cases_host.py (plain fp32 torch against fp64, the metric above), rounded up in the third digit.
# F.gelu in float32 overflows an intermediate at u = 3e38 and returns inf there: the reference figure is taken over the elements
# where the reference itself is finite (all but that one); the kernels are gated on every element, that one included.
REF_FWD = 2.56e-7          # F.gelu in float32 on grid(n), the same for every n the tests use; worst at u = 2.957
REF_BWD = 2.12e-7          # its autograd, dy = 1; worst at u = 0.262
# the fused forms: R.groupnorm1 + R.filt_act (delta taps) in float32 against the fp64 pre-activation: the same for every shape,
# since the shapes hold the same 4096 values of x (gn_inputs); worst at u = 2.117 and 1.423
GN_SHAPES = [(1, 256, 4, 4), (1, 128, 8, 8), (1, 64, 16, 16), (1, 64, 32, 32)]        # the three `_gn` sites; stats + act
REF_GN = {sh: (1.97e-7, 1.24e-7) for sh in GN_SHAPES}
GATE_FACTOR = 2.0


def gate_fwd():
    return GATE_FACTOR * REF_FWD


def gate_bwd():
    return GATE_FACTOR * REF_BWD


def gate_gn(shape):
    f, b = REF_GN[tuple(shape)]
    return GATE_FACTOR * f, GATE_FACTOR * b


# ---- the grid --------------------------------------------------------------------------------------------------------------
def _f32_neighbours(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def special_points():
    """Every piece boundary k/16, k in [-130, 130], with its two fp32 neighbours; +-6 with theirs (part of the former); the
    saturated region; zeros, a tiny normal and a denormal."""
    pts = []
    for k in range(-130, 131):
        pts += _f32_neighbours(k / 16.0)
    for v in (6.5, 8.0, 50.0, 1e4, 3e38, 1e-30, 1e-45):
        pts += [np.float32(v), np.float32(-v)]
    pts += [np.float32(0.0), np.float32(-0.0)]
    return np.asarray(pts, dtype=np.float32)


def grid(n=GRID_N):
    """n fp32 values of u: the special points, then uniform draws on [-8, 8]; in a fixed shuffled order, so that the special
    points land on every lane, row and plane slot of the kernels.  grid(m)[:...] and grid(n) share points, not positions."""
    sp = special_points()
    assert n >= sp.size + 1000, n
    g = torch.Generator().manual_seed(20)
    fill = (torch.rand(n - sp.size, generator=g, dtype=torch.float64) * 16 - 8).float().numpy()
    u = np.concatenate([sp, fill])
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).numpy()
    return torch.from_numpy(u[perm].copy())


def filt_act_cases():
    """(S, C) of ops.FiltAct at (1, C, S, S): plane counts that fill whole waves (the FULL kernel variants, C * S * S = 4096), and
    where a wave holds more than one plane (64 // S > 1) one plane more than that (the dead-lane variants)."""
    out = []
    for S in (4, 8, 16, 32, 64):
        C = GRID_N // (S * S)
        assert C % max(64 // S, 1) == 0
        out.append((S, C))
        if 64 // S > 1:
            out.append((S, C + 1))
    return out


def delta_taps():
    k = torch.zeros(3, 3, dtype=torch.float64)
    k[1, 1] = 1.0
    return k


# ---- fp64 references -------------------------------------------------------------------------------------------------------
def phi64(u):
    u = u.double()
    return 0.5 * torch.special.erfc(-u / math.sqrt(2.0))


def gelu64(u):
    u = u.double()
    return u * phi64(u)


def gelu_grad64(u):
    u = u.double()
    return phi64(u) + u * torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def fwd_metric(y, u):
    """-> (worst, u at the worst) of |y - GELU64(u)| / max(|u|, 2^-126); a non-finite y counts as infinite."""
    u = u.double().flatten()
    e = (y.double().flatten() - gelu64(u)).abs() / u.abs().clamp_min(TINY)
    e = torch.where(torch.isfinite(y.double().flatten()), e, torch.full_like(e, math.inf))
    i = int(e.argmax())
    return float(e[i]), float(u[i])


def bwd_metric(dx, u):
    """-> (worst, u at the worst) of |dx - GELU'64(u)|."""
    u = u.double().flatten()
    e = (dx.double().flatten() - gelu_grad64(u)).abs()
    e = torch.where(torch.isfinite(dx.double().flatten()), e, torch.full_like(e, math.inf))
    i = int(e.argmax())
    return float(e[i]), float(u[i])


# ---- plain fp32 torch: the figures behind the gates ------------------------------------------------------------------------
def torch_f32(u):
    """F.gelu and its autograd (dy = 1) in float32 -> (y, dx)."""
    x = u.clone().float().requires_grad_(True)
    y = F.gelu(x)
    (dx,) = torch.autograd.grad(y, x, torch.ones_like(y))
    return y.detach(), dx


def reference_figures(y, dx, u):
    """The reference's own worst forward / backward value over the elements where it is finite
    -> ((fwd, u), (bwd, u), the values of u left out)."""
    ok = torch.isfinite(y.flatten()) & torch.isfinite(dx.flatten())
    uf = u.flatten()
    return fwd_metric(y.flatten()[ok], uf[ok]), bwd_metric(dx.flatten()[ok], uf[ok]), uf[~ok].tolist()


def gn_inputs(shape):
    """x = the 4096 odd multiples of 2^-12 in (-1, 1), each used equally often, shuffled; gamma = +-4.1, beta = 0: the
    pre-activation u covers [-7.1, 7.1].  The sums of such x are exact in fp32 in any order and the mean is exactly 0, so u carries
    only the RELATIVE error of rstd * gamma (about 2e-7): with a beta, or a mean that rounds, u would carry an absolute error, and
    the forward metric's division by |u| would turn the one element that happens to lie nearest to 0 into the figure (measured
    with a random beta: 3e-6 ... 9e-6 for plain fp32 torch, set by chance and growing with the tensor)."""
    B, C, H, W = shape
    n = B * C * H * W
    assert n % 4096 == 0
    g = torch.Generator().manual_seed(n)
    base = (2.0 * torch.arange(-2048, 2048, dtype=torch.float64) + 1.0) / 4096.0
    x = base.repeat(n // 4096)[torch.randperm(n, generator=g)].reshape(shape).float()
    gamma = torch.full((C,), 4.1)
    gamma[1::2] = -4.1
    return x, gamma, torch.zeros(C)


def gn_compose(x, gamma, beta, dtype):
    """GroupNorm(1, C) -> filtered GELU with delta taps, in `dtype`, with a zero residual as a leaf: its gradient under dy = 1
    is GELU'(u).  -> (u, y, dres)."""
    res = torch.zeros_like(x, dtype=dtype).requires_grad_(True)
    k = delta_taps().to(dtype)
    u = R.groupnorm1(x.to(dtype), gamma.to(dtype), beta.to(dtype)) + res
    y = R.filt_act(u, k, k)
    (dres,) = torch.autograd.grad(y, res, torch.ones_like(y))
    return u.detach(), y.detach(), dres


# ---- gelu_piece of csrc/filt.hip, restated in fp32 -------------------------------------------------------------------------
def piece_tables():
    """The coefficients gelu_table_init computes (fp64 Hermite data, rounded to fp32): (192, 4) for Phi and for GELU'."""
    h = 1.0 / 16.0
    a0 = (np.arange(PIECES, dtype=np.float64) - 96.0) * h
    a1 = a0 + h
    phi = lambda a: np.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
    Phi = lambda a: phi64(torch.from_numpy(a)).numpy()
    gfun = lambda a: Phi(a) + a * phi(a)
    gder = lambda a: (2.0 - a * a) * phi(a)

    def hermite(f, d):
        f0, f1, d0, d1 = f(a0), f(a1), h * d(a0), h * d(a1)
        return np.stack([f0, d0, 3.0 * (f1 - f0) - 2.0 * d0 - d1, 2.0 * (f0 - f1) + d0 + d1], axis=1).astype(np.float32)

    return hermite(Phi, phi), hermite(gfun, gder)


def _fma32(a, b, c):
    """fp32 fma rounded once (the product of two fp32 values is exact in fp64)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def piece_f32(u, table, fused_index=False):
    """gelu_piece: sx = med3(16 u, -96, 96 - 0.001) (the product is exact); piece = floor(sx) + 96; t = fract(sx), at most the
    largest fp32 below 1 as v_fract_f32 returns it; Horner with three fmas.
    fused_index: the form the kernel had first, piece and t from ONE fma -- sx = med3(fma(u, 16, 96), 0, 192 - 0.001),
    piece = (int)sx -- kept so that the host test can show what the rounding of that fma cost."""
    u = np.asarray(u, dtype=np.float32)
    with np.errstate(over="ignore"):
        if fused_index:
            sx = np.clip(_fma32(u, np.float32(SCALE), np.float32(OFFSET)), np.float32(0.0), np.float32(PIECES) - np.float32(0.001))
        else:
            sx = np.clip(u * np.float32(SCALE), np.float32(-OFFSET), np.float32(OFFSET) - np.float32(0.001))
    fl = np.floor(sx)
    idx = fl.astype(np.int32) + (0 if fused_index else PIECES // 2)
    t = np.minimum(sx - fl, np.nextafter(np.float32(1.0), np.float32(0.0)))
    c = table[idx]
    return _fma32(_fma32(_fma32(c[:, 3], t, c[:, 2]), t, c[:, 1]), t, c[:, 0])


def restated_f32(u, fused_index=False):
    """gelu_tab and gelu_grad_tab in fp32 -> (y, dx) as tensors."""
    un = u.float().flatten().numpy()
    tp, tg = piece_tables()
    with np.errstate(over="ignore", under="ignore"):
        y = un * piece_f32(un, tp, fused_index)
    return torch.from_numpy(y).reshape(u.shape), torch.from_numpy(piece_f32(un, tg, fused_index)).reshape(u.shape)
