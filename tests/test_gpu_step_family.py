"""The sixteen DDPM / DDIM step entry points (plain, guided, masked, guided and masked; host or device step index), through
their `ops` wrappers, bit for bit against a restatement in CPU torch fp32 that calls none of them.  All sixteen are
instantiations of one kernel template, so comparing them with each other cannot catch a mistake they share; this can.  The
sizes are chosen for the template's loop: below and at one quad, odd, aligned, unaligned (scalar kernel, mask misaligned), and
one size each at which the 16-byte and the scalar grid-stride loop wrap (more than 2048 workgroups of 256 work items).  The plain
DDPM step launches up to 32768 workgroups, so it gets a wrap size of its own."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WRAP_VEC = 2048 * 256 * 4 + 1028        # 16-byte kernel: 2048 * 256 quads, then 257 more
WRAP_SCALAR = 2048 * 256 + 5            # scalar kernel (unaligned): 2048 * 256 elements, then 5 more
WRAP_PLAIN = 32768 * 256 + 517          # the plain DDPM step's grid: 32768 * 256 elements, then 517 more
SIZES = [(3, 0), (4, 0), (315, 0), (768, 0), (768, 1), (WRAP_VEC, 0), (WRAP_SCALAR, 1)]      # (n, offset into a larger buffer)
STEPS = {"ddpm": [(999, 998), (37, 36), (1, 0)], "ddim": [(700, 350), (20, 0), (1, 0)]}
ETAS = [0.0, 0.5, 1.0]
SCALES = [0.3, 3.0]                     # both branches of the lerp


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=gpu)
    tables = {k: getattr(diff, k).detach().cpu() for k in ("alpha", "alpha_hat", "beta")}
    return afdm, gpu, diff, tables


def _f32(v):
    return float(np.float32(v))


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_inputs = {}


def _case_inputs(n, off, dev):
    """Host inputs of one size (x, eps2 of 2n, z, x0, mask) and their device copies `off` elements into larger buffers; made once."""
    if (n, off) not in _inputs:
        g = torch.Generator().manual_seed(1000 * off + n % 9973)
        host = {"x": torch.randn(n, generator=g), "e2": torch.randn(2 * n, generator=g), "z": torch.randn(n, generator=g),
                "x0": torch.randn(n, generator=g), "m": (torch.rand(n, generator=g) < 0.5).to(torch.uint8)}
        host["m"][0], host["m"][n - 1] = 0, 1                       # both values present at every size
        device = {}
        for k, v in host.items():
            buf = torch.zeros(v.numel() + off, dtype=v.dtype, device=dev)
            device[k] = buf[off:]
            device[k].copy_(v)
        _inputs[(n, off)] = (host, device)
    return _inputs[(n, off)]


# ---- the restatement: one torch op per rounding, every scalar a full fp32 tensor (no scalar fast path, e.g. no reciprocal) ------
def _full(like, v):
    return torch.full_like(like, _f32(v))


def _lerp_restated(u, c, s):
    """ATen's scalar lerp (aten/src/ATen/native/Lerp.h)."""
    s = _f32(s)
    d = c - u
    if abs(s) < 0.5:
        return u + _full(d, s) * d
    return c - d * _full(d, _f32(1 - s))


def _ddpm_restated(x, e, z, tab, i):
    """x' = 1/sqrt(a) * (x - ((1-a)/sqrt(1-ah)) * eps) + sqrt(b) * noise; the scalars in fp32, one rounding per operation
    (taken in fp64 and rounded once: exact for + - * / sqrt)."""
    a, ah, b = float(tab["alpha"][i]), float(tab["alpha_hat"][i]), float(tab["beta"][i])
    c1 = _f32(1 / _f32(math.sqrt(a)))
    c2 = _f32(_f32(1 - a) / _f32(math.sqrt(_f32(1 - ah))))
    lhs = _full(x, c1) * (x - _full(x, c2) * e)
    return lhs + (_full(x, _f32(math.sqrt(b))) * z if z is not None else torch.zeros_like(x))


def _ddim_restated(x, e, z, tab, t, tp, eta):
    a_t, a_p, eta = float(tab["alpha_hat"][t]), float(tab["alpha_hat"][tp]), _f32(eta)
    sq = lambda v: _f32(math.sqrt(v))
    r = _f32(_f32(1 - a_p) / _f32(1 - a_t))
    q = _f32(1 - _f32(a_t / a_p))
    var = _f32(_f32(eta * eta) * _f32(r * q))
    direction = sq(max(_f32(_f32(1 - a_p) - var), 0.0))
    x0 = (x - _full(x, sq(_f32(1 - a_t))) * e) / _full(x, sq(a_t))
    mean = _full(x, sq(a_p)) * x0 + _full(x, direction) * e
    return mean + (_full(x, sq(var)) * z if z is not None else torch.zeros_like(x))


def _known_restated(x0, z, tab, tp):
    """x0 noised to t_prev: sqrt(a_p) * x0 + sqrt(1 - a_p) * z, x0 itself at t_prev == 0"""
    if tp == 0:
        return x0
    a_p = float(tab["alpha_hat"][tp])
    return _full(x0, _f32(math.sqrt(a_p))) * x0 + _full(x0, _f32(math.sqrt(_f32(1 - a_p)))) * z


def _want(h, tab, sampler, guided, masked, t, tp, eta, s, use_z):
    n = h["x"].numel()
    e = _lerp_restated(h["e2"][n:], h["e2"][:n], s) if guided else h["e2"][:n]
    z = h["z"] if use_z else None
    if masked:       # the generated region takes the noise only where the chain goes on (and, for DDIM, eta != 0)
        gz = z if (t > 1 if sampler == "ddpm" else eta != 0 and tp > 0) else None
    else:
        gz = z
    gen = _ddpm_restated(h["x"], e, gz, tab, t) if sampler == "ddpm" else _ddim_restated(h["x"], e, gz, tab, t, tp, eta)
    if not masked:
        return gen
    return torch.where(h["m"].bool(), _known_restated(h["x0"], z, tab, tp), gen)


def _run(ops, diff, d, dev, sampler, guided, masked, form, t, tp, eta, s, use_z):
    """One launch through the entry point's wrapper -> (out, out2); the `_dev` forms run in place."""
    n = d["x"].numel()
    e = d["e2"] if guided else d["e2"][:n]
    z = d["z"] if use_z else None
    tables = (diff.alpha, diff.alpha_hat, diff.beta) if sampler == "ddpm" else (diff.alpha_hat,)
    name = ("denoise_step" if sampler == "ddpm" else "ddim_step") + "_masked" * masked + "_cfg" * guided + "_dev" * (form == "dev")
    if form == "dev":
        index = [torch.full((1,), v, device=dev, dtype=torch.long) for v in ((t,) if sampler == "ddpm" else (t, tp))]
        x = torch.empty_like(d["x"]) if d["x"].data_ptr() % 16 == 0 else torch.empty(n + 1, device=dev)[1:]
        x.copy_(d["x"])
        out = x
    else:
        index = [t] if sampler == "ddpm" else [t, tp]
        x, out = d["x"], None
    args = [x, e, z] + ([d["x0"], d["m"]] if masked else []) + list(tables) + index + ([eta] if sampler == "ddim" else [])
    out2 = None
    if guided:
        out2 = torch.full_like(d["x"], float("nan")) if d["x"].data_ptr() % 16 == 0 else torch.full((n + 1,), float("nan"), device=dev)[1:]
        got = getattr(ops, name)(*args, s, out, out2) if form == "dev" else getattr(ops, name)(*args, s, out2=out2)
    else:
        got = getattr(ops, name)(*args, out) if form == "dev" else getattr(ops, name)(*args)
    if form == "dev":
        assert got.data_ptr() == x.data_ptr()
    return got, out2


@pytest.mark.parametrize("n,off", SIZES)
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_step_entry_point_equals_cpu_restatement(A, sampler, guided, masked, form, n, off):
    afdm, dev, diff, tab = A
    from afdm import ops
    h, d = _case_inputs(n, off, dev)
    assert d["x"].data_ptr() % 16 == 4 * off and d["m"].data_ptr() % 4 == off and 0 < int(h["m"].sum()) < n
    combos = [(t, tp, eta, s) for (t, tp) in STEPS[sampler] for eta in (ETAS if sampler == "ddim" else [0.0])
              for s in (SCALES if guided else [0.0])]
    if n >= WRAP_SCALAR:       # the wrap sizes: one launch each; the entry points between them still see every step, eta and scale
        combos = [combos[(2 * guided + masked + 4 * (form == "dev") + 5 * (off > 0)) % len(combos)]]
    for t, tp, eta, s in combos:
        noise_optional = not masked or (form == "host" and tp == 0)
        for use_z in ([True, False] if noise_optional and n < WRAP_SCALAR else [True]):
            want = _want(h, tab, sampler, guided, masked, t, tp, eta, s, use_z)
            got, out2 = _run(ops, diff, d, dev, sampler, guided, masked, form, t, tp, eta, s, use_z)
            assert _same_bits(got.cpu(), want), (t, tp, eta, s, use_z, int((got.cpu() != want).sum()))
            if guided:
                assert _same_bits(out2, got), (t, tp, eta, s, use_z)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_plain_ddpm_step_wraps_its_grid(A, form):
    afdm, dev, diff, tab = A
    from afdm import ops
    h, d = _case_inputs(WRAP_PLAIN, 0, dev)
    t, tp = STEPS["ddpm"][1]
    want = _want(h, tab, "ddpm", False, False, t, tp, 0.0, 0.0, True)
    got, _ = _run(ops, diff, d, dev, "ddpm", False, False, form, t, tp, 0.0, 0.0, True)
    assert _same_bits(got.cpu(), want), int((got.cpu() != want).sum())
