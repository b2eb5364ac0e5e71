"""CPU tests of diffusion posterior sampling's host side: the LinearOperator family's cpu path against F.conv2d and its autograd in
fp64, the adjoint identity for every constructor, the (a, b) table of x0_hat = a x_t + b out for the three predictions, and every
refusal of LinearOperator, of the four C entry points (nothing launched), of Diffusion.posterior_sample and of posterior_results
(the model is never called before the checks pass)."""
import inspect
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import note, rel_l2


@pytest.fixture(scope="module")
def afdm():
    import afdm
    return afdm


def _kernel(K, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.rand(K, K, generator=g) + 0.1
    return k / k.sum()


def _mask(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.6).float()


# (B, C, H, W, K, s, mask shape): the device tests' shapes
CASES = [(3, 3, 32, 32, 9, 1, None), (2, 1, 32, 32, 5, 2, (1, 16, 16)), (2, 3, 16, 16, 15, 4, (3, 4, 4)), (5, 3, 8, 8, 1, 1, (1, 8, 8)),
         (2, 2, 8, 16, 3, 2, None), (1, 1, 64, 64, 15, 1, None)]


def _conv_line(x, k, s, m):
    C, K = x.shape[1], k.shape[0]
    y = F.conv2d(x, k.double().expand(C, 1, K, K), padding=K // 2, stride=s, groups=C)
    return y if m is None else y * m.double()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c[:6]))
def test_cpu_apply_and_adjoint_equal_conv2d_and_its_autograd(afdm, case):
    B, C, H, W, K, s, ms = case
    g = torch.Generator().manual_seed(K * 100 + s)
    k = _kernel(K, K) if K > 1 else None
    m = None if ms is None else _mask(ms, 5)
    op = afdm.LinearOperator(k, s, m)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    r = torch.randn(B, C, H // s, W // s, generator=g, dtype=torch.float64)
    kk = torch.ones(1, 1) if k is None else k
    want = _conv_line(x, kk, s, m)
    got = op.apply(x)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.equal(got, want)
    assert torch.equal(op.apply(x.float()), _conv_line(x.float().double(), kk, s, m))          # fp32 in: widened first, fp64 out
    xg = x.clone().requires_grad_(True)
    (want_adj,) = torch.autograd.grad(_conv_line(xg, kk, s, m), xg, r)
    got_adj = op.adjoint(r)
    assert got_adj.dtype == torch.float64 and got_adj.shape == x.shape
    e = rel_l2(got_adj, want_adj)
    note("dps host: cpu adjoint vs autograd of F.conv2d (fp64)", e, case)
    assert e <= 1e-14
    # autograd passes through the cpu path itself
    (through,) = torch.autograd.grad(op.apply(xg), xg, r)
    assert rel_l2(through, want_adj) <= 1e-14


def _constructors(afdm):
    hole = torch.ones(16, 16)
    hole[4:12, 4:12] = 0
    line = torch.zeros(7, 7)
    line[3, :] = 1.0 / 7
    return {"inpainting": (afdm.LinearOperator.inpainting(hole), 16), "inpainting_c": (afdm.LinearOperator.inpainting(_mask((3, 16, 16), 2)), 16),
            "gaussian_blur": (afdm.LinearOperator.gaussian_blur(9, 2.0), 16),
            "super_resolution": (afdm.LinearOperator.super_resolution(4), 16),
            "super_resolution_2": (afdm.LinearOperator.super_resolution(2, size=5, sigma=1.0), 16),
            "motion_blur": (afdm.LinearOperator.motion_blur(line), 16),
            "combined": (afdm.LinearOperator(afdm.gaussian_kernel(5, 1.0), 2, _mask((1, 8, 8), 3)), 16)}


def test_adjoint_identity_for_every_constructor(afdm):
    g = torch.Generator().manual_seed(0)
    for name, (op, S) in _constructors(afdm).items():
        x = torch.randn(2, 3, S, S, generator=g, dtype=torch.float64)
        y = op.apply(x)
        r = torch.randn(y.shape, generator=g, dtype=torch.float64)
        lhs, rhs = float((y * r).sum()), float((x * op.adjoint(r)).sum())
        scale = float(y.norm() * r.norm())
        note("dps host: |<Ax, r> - <x, A^T r>| / (|Ax| |r|), fp64", abs(lhs - rhs) / scale, name)
        assert abs(lhs - rhs) <= 1e-12 * scale, name


def test_constructors_build_what_they_say(afdm):
    L = afdm.LinearOperator
    sr = L.super_resolution(4)
    assert (sr.K, sr.stride, sr.mask) == (9, 4, None) and "2 factor + 1" in L.super_resolution.__doc__
    assert torch.equal(sr.kernel, afdm.gaussian_kernel(9, 2.0))
    assert L.super_resolution(2).K == 5 and L.super_resolution(1).K == 3
    k = afdm.gaussian_kernel(5, 1.0)
    assert k.dtype == torch.float32 and abs(float(k.double().sum()) - 1) < 1e-6 and torch.equal(k, k.T) and float(k[2, 2]) == float(k.max())
    delta = L()
    assert delta.K == 1 and delta.stride == 1 and delta.mask is None
    x = torch.randn(1, 2, 8, 8, dtype=torch.float64)
    assert torch.equal(delta.apply(x), x) and torch.equal(delta.adjoint(x), x)
    inp = L.inpainting(torch.ones(8, 8, dtype=torch.int64))                     # an integer 0 / 1 mask, 2-D: one mask for every channel
    assert tuple(inp.mask.shape) == (1, 8, 8) and inp.mask.dtype == torch.float32
    # measure: A x + sigma n from the generator given
    op = L.gaussian_blur(3, 1.0)
    y0 = op.measure(x)
    assert torch.equal(y0, op.apply(x))
    y1 = op.measure(x, 0.5, generator=torch.Generator().manual_seed(3))
    n = torch.randn(y0.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    assert torch.equal(y1, y0 + 0.5 * n)


@pytest.mark.parametrize("prediction", ["eps", "v", "x0"])
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_x0_coefficients_invert_the_training_target(afdm, prediction, schedule):
    diff = afdm.Diffusion(noise_steps=1000, img_size=8, device="cpu", prediction=prediction, schedule=schedule)
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(3, 2, 8, 8, generator=g, dtype=torch.float64)
    eps = torch.randn(3, 2, 8, 8, generator=g, dtype=torch.float64)
    t = torch.tensor([1, 500, 999])
    ah = diff.alpha_hat.double()[t].view(-1, 1, 1, 1)
    x_t = ah.sqrt() * x0 + (1 - ah).sqrt() * eps                                  # noise_images' expression, in fp64
    a, b = diff.x0_coefficients(t)
    assert a.dtype == torch.float64 and tuple(a.shape) == (3,)
    got = a.view(-1, 1, 1, 1) * x_t + b.view(-1, 1, 1, 1) * diff.training_target(x0, eps, t)
    e = rel_l2(got, x0)
    note(f"dps host: a x_t + b target returns x0, fp64 ({prediction})", e, schedule)
    # x_t of size ~1 carries three roundings, the two products and the sum three more, and "eps" multiplies them by 1 / sqrt(ah)
    # (157 at t = 999 of the linear table, far more on the cosine one, whose last ah is ~1e-9): 8 machine epsilons times that gain
    gain = float((1 / ah.sqrt()).max()) if prediction == "eps" else 1.0
    assert e <= 8 * 2.2e-16 * gain


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_linear_operator_refusals(afdm):
    L = afdm.LinearOperator
    bad = lambda *a, **kw: pytest.raises(ValueError, match=r"^LinearOperator: ")
    for kernel in (torch.ones(4, 4), torch.ones(17, 17), torch.ones(3, 5), torch.ones(3), torch.ones(3, 3, dtype=torch.long), [[1.0]],
                   torch.full((3, 3), float("nan"))):
        with bad():
            L(kernel)
    for stride in (0, 3, 8, 2.0, True, None):
        with bad():
            L(None, stride)
    for mask in (torch.ones(8, 8), torch.ones(1, 1, 8, 8), torch.ones(1, 8, 8, dtype=torch.long), "center", torch.full((1, 2, 2), float("inf"))):
        with bad():
            L(None, 1, mask)
    with bad():
        L.inpainting(None)
    with bad():
        L.gaussian_blur(4, 1.0)
    with bad():
        L.gaussian_blur(5, 0.0)
    with bad():
        L.super_resolution(3)
    with bad():
        L.motion_blur(torch.ones(3, 3))                                            # not normalised
    with bad():
        L.motion_blur(None)
    op = L(torch.ones(3, 3) / 9, 2, torch.ones(3, 4, 4))
    x = torch.zeros(1, 3, 8, 8)
    assert tuple(op.apply(x).shape) == (1, 3, 4, 4) and tuple(op.adjoint(torch.zeros(1, 3, 4, 4)).shape) == (1, 3, 8, 8)
    for v in (torch.zeros(3, 8, 8), torch.zeros(1, 3, 8, 8, dtype=torch.float16), torch.zeros(0, 3, 8, 8), [1.0],
              torch.zeros(1, 3, 9, 8), torch.zeros(1, 3, 128, 128), torch.zeros(1, 2, 8, 8), torch.zeros(1, 3, 16, 16)):
        with bad():
            op.apply(v)
    for v in (torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 64, 64), torch.zeros(3, 4, 4)):
        with bad():
            op.adjoint(v)
    for sigma in (-1.0, float("nan"), "0.1"):
        with bad():
            op.measure(x, sigma)


def test_entry_points_reject_bad_arguments_without_a_gpu(afdm):
    """AFD_EINVAL with nothing launched: the pointers are host buffers that a refused call never reads."""
    import numpy as np
    L = afdm.lib()
    buf = np.zeros(4096, dtype=np.float64)
    p, q = buf.ctypes.data, buf.ctypes.data + 16384
    k = np.full((3, 3), 1 / 9, dtype=np.float32).ctypes.data
    E = afdm.AfdError
    for fn in (L.afd_linop_apply, L.afd_linop_adjoint):
        with pytest.raises(E, match="NULL"):
            fn(None, q, k, 3, 1, None, 0, 1, 1, 8, 8, None)
        with pytest.raises(E, match="K must be odd"):
            fn(p, q, k, 4, 1, None, 0, 1, 1, 8, 8, None)
        with pytest.raises(E, match="K must be odd"):
            fn(p, q, k, 17, 1, None, 0, 1, 1, 8, 8, None)
        with pytest.raises(E, match="kernel must not be NULL"):
            fn(p, q, None, 3, 1, None, 0, 1, 1, 8, 8, None)
        with pytest.raises(E, match="stride must be 1, 2 or 4"):
            fn(p, q, k, 3, 3, None, 0, 1, 1, 8, 8, None)
        with pytest.raises(E, match="multiples of the stride"):
            fn(p, q, k, 3, 4, None, 0, 1, 1, 6, 8, None)
        with pytest.raises(E, match=r"\[1, 64\]"):
            fn(p, q, k, 3, 1, None, 0, 1, 1, 128, 8, None)
        with pytest.raises(E, match="mask_channels"):
            fn(p, q, k, 3, 1, p, 2, 1, 3, 8, 8, None)
        with pytest.raises(E, match="mask_channels"):
            fn(p, q, k, 3, 1, None, 1, 1, 3, 8, 8, None)
        with pytest.raises(E, match="B and C must be positive"):
            fn(p, q, k, 3, 1, None, 0, 0, 3, 8, 8, None)
        with pytest.raises(E, match="must not overlap"):
            fn(p, p, k, 3, 1, None, 0, 1, 1, 8, 8, None)
    res = lambda **kw: L.afd_dps_residual(*[kw.get(n, d) for n, d in (("x_t", p), ("out", p + 4096), ("t", p + 8192), ("ah", p + 12288),
                                                                       ("kind", 0), ("y", p + 14336), ("kernel", k), ("K", 3), ("s", 1),
                                                                       ("mask", None), ("mc", 0), ("g", q), ("sums", q + 8192), ("B", 1),
                                                                       ("C", 1), ("H", 8), ("W", 8), ("stream", None))])
    with pytest.raises(E, match="NULL"):
        res(sums=None)
    with pytest.raises(E, match="kind must be"):
        res(kind=3)
    with pytest.raises(E, match="8-byte aligned"):
        res(sums=q + 8196)
    with pytest.raises(E, match="stride must be"):
        res(s=8)
    with pytest.raises(E, match="must not overlap"):
        res(g=p)
    with pytest.raises(E, match="must not overlap"):
        res(sums=p + 4096)
    cor = lambda **kw: L.afd_dps_correct(*[kw.get(n, d) for n, d in (("x", p), ("g", p + 4096), ("v", p + 8192), ("sums", q), ("t", q + 4096),
                                                                      ("ah", q + 8192), ("kind", 0), ("zeta", 1.0), ("B", 1), ("C", 1),
                                                                      ("HW", 64), ("stream", None))])
    with pytest.raises(E, match="NULL"):
        cor(v=None)
    with pytest.raises(E, match="kind must be"):
        cor(kind=-1)
    for z in (-1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="zeta must be finite"):
            cor(zeta=z)
    with pytest.raises(E, match="must be positive"):
        cor(HW=0)
    with pytest.raises(E, match="must not overlap"):
        cor(g=p)


class _Never(torch.nn.Module):
    """A model that must not be called."""
    calls = 0

    def forward(self, x, t, y=None):
        type(self).calls += 1
        raise AssertionError("the model was called before the checks passed")


def test_posterior_sample_refusals_never_call_the_model(afdm):
    diff = afdm.Diffusion(noise_steps=50, img_size=16, device="cpu")
    op = afdm.LinearOperator.super_resolution(2)
    y = torch.zeros(2, 3, 8, 8)
    model = _Never()
    bad = lambda: pytest.raises(ValueError, match=r"^Diffusion\.posterior_sample: ")
    for zeta in (-1.0, float("nan"), float("inf"), "1", None, True):
        with bad():
            diff.posterior_sample(model, y, op, zeta=zeta)
    for meas in (torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 8, 4), torch.zeros(3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.float64),
                 torch.zeros(0, 3, 8, 8), [[0.0]]):
        with bad():
            diff.posterior_sample(model, meas, op)
    for wrong in (None, "blur", torch.ones(3, 3), lambda x: x):
        with bad():
            diff.posterior_sample(model, y, wrong)
    with bad():                                                                    # a mask that does not fit the measurement
        diff.posterior_sample(model, y, afdm.LinearOperator(None, 2, torch.ones(1, 4, 4)))
    with bad():                                                                    # eta without steps
        diff.posterior_sample(model, y, op, eta=1.0)
    with pytest.raises(ValueError):
        diff.posterior_sample(model, y, op, steps=[5, 5])
    with pytest.raises(ValueError, match="no label embedding"):
        diff.posterior_sample(model, y, op, labels=torch.zeros(2, dtype=torch.long))
    learned = afdm.Diffusion(noise_steps=50, img_size=16, device="cpu", variance="learned")
    with pytest.raises(ValueError, match=r"^Diffusion\.posterior_sample: variance='learned'"):
        learned.posterior_sample(model, y, op)
    assert _Never.calls == 0
    params = list(inspect.signature(afdm.Diffusion.posterior_sample).parameters)
    assert params == ["self", "model", "measurement", "operator", "zeta", "steps", "eta", "labels", "noise_source", "return_float"]
    assert "cfg_scale" not in params and "graph" not in params and "theta" not in params      # not offered: see the docstring
    assert "Classifier-free guidance is not offered" in afdm.Diffusion.posterior_sample.__doc__


def test_posterior_results_is_exported_and_checks_first(afdm):
    from afdm import tasks
    assert tasks.posterior_results is afdm.posterior_results
    assert list(inspect.signature(afdm.posterior_results).parameters) == ["model_data", "images", "operator", "sigma", "zeta", "n", "steps",
                                                                          "eta", "kw"]
    assert not any(e.key == "eval_posterior" for e in tasks.EVALS)
    images = torch.zeros(4, 3, 16, 16, dtype=torch.uint8)
    with pytest.raises(ValueError, match="posterior_results: operator must be"):
        afdm.posterior_results({}, images, "blur")                                  # (fails before the checkpoint is read)
    with pytest.raises(ValueError, match="posterior_results: n must be an int in"):
        afdm.posterior_results({}, images, afdm.LinearOperator(), n=5)
    with pytest.raises(ValueError, match="posterior_results: images must be"):
        afdm.posterior_results({}, images.float(), afdm.LinearOperator(), n=2)
