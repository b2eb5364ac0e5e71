"""CPU tests of the probability-flow ODE likelihood's host side: the public signatures and the header's two declarations, the
refusals of the two C entry points (nothing launched), the (c1, c2) table of J_eps = c1 I + c2 J_out against autograd, the accuracy
and the order of both integration rules on Gaussian data through `ode_likelihood_reference`, the exact trace on a non-diagonal
Jacobian, the bpd / logp relation, the dequantisation, and every refusal of Diffusion.ode_likelihood (the model is never called)."""
import inspect
import math

import pytest
import torch

from conftest import note


@pytest.fixture(scope="module")
def afdm():
    import afdm
    return afdm


# ---- signatures ------------------------------------------------------------------------------------------------------------------
def _defaults(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures_and_declarations(afdm):
    import ctypes
    from afdm import likelihood, ops, tasks
    from afdm._lib import parse_header
    E = inspect.Parameter.empty
    assert _defaults(afdm.Diffusion.ode_likelihood) == [
        ("self", E), ("model", E), ("images", E), ("steps", 100), ("method", "heun"), ("probes", 1), ("probe", "rademacher"),
        ("labels", None), ("dequantize", False), ("noise_source", "device"), ("return_latents", False)]
    assert _defaults(afdm.likelihood_results) == [("model_data", E), ("images", E), ("n", 4), ("steps", 100), ("kw", E)]
    assert tasks.likelihood_results is afdm.likelihood_results
    assert _defaults(ops.ode_trace_rows) == [("v", E), ("w", E), ("cvv", E), ("cvw", E), ("acc", E)]
    assert _defaults(ops.ode_heun_step) == [("x", E), ("eps_s", E), ("eps_u", E), ("alpha_hat", E), ("s", E), ("u", E), ("out", None)]
    assert _defaults(likelihood.ode_likelihood_reference) == [
        ("eps_fn", E), ("x0", E), ("alpha_hat", E), ("levels", E), ("probes_tensor", E), ("method", "heun"), ("coefficients", None)]
    assert afdm.ode_likelihood_reference is likelihood.ode_likelihood_reference
    sigs = parse_header()
    p, i, L, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    assert sigs["afd_ode_trace_rows"] == (i, [p, p, D, D, p, L, L, p])
    assert sigs["afd_ode_heun_step"] == (i, [p, p, p, p, i, i, p, L, p])
    lib = afdm.lib()
    assert hasattr(lib.cdll, "afd_ode_trace_rows") and hasattr(lib.cdll, "afd_ode_heun_step")
    assert not any(e.key == "eval_likelihood" for e in tasks.EVALS)
    doc = afdm.Diffusion.ode_likelihood.__doc__
    for said in ("BASELINE", "Do not quote a likelihood from it", "-0.160", "+0.0052", "Not offered: classifier-free guidance",
                 "graph capture", "adaptive step control", "for small images and tests", "in this order"):
        assert said in doc, said


# ---- the C entry points refuse bad arguments with nothing launched ---------------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_a_gpu(afdm):
    """AFD_EINVAL with nothing launched: the pointers are host buffers that a refused call never reads."""
    import numpy as np
    L = afdm.lib()
    E = afdm.AfdError
    buf = np.zeros(8192, dtype=np.float64)
    p = buf.ctypes.data
    tr = lambda **kw: L.afd_ode_trace_rows(*[kw.get(n, d) for n, d in (("v", p), ("w", p + 4096), ("cvv", 1.0), ("cvw", 1.0),
                                                                       ("acc", p + 16384), ("rows", 4), ("per", 64), ("stream", None))])
    with pytest.raises(E, match="v and acc must not be NULL"):
        tr(v=None)
    with pytest.raises(E, match="v and acc must not be NULL"):
        tr(acc=None)
    with pytest.raises(E, match="w must not be NULL unless cvw == 0"):
        tr(w=None)
    for bad in (0, -3):
        with pytest.raises(E, match="rows and per must be positive"):
            tr(rows=bad)
        with pytest.raises(E, match="rows and per must be positive"):
            tr(per=bad)
    with pytest.raises(E, match="at most 2\\^31 - 1 rows"):
        tr(rows=1 << 31, per=1)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(E, match="must be finite"):
            tr(cvv=bad)
        with pytest.raises(E, match="must be finite"):
            tr(cvw=bad)
    with pytest.raises(E, match="aligned"):
        tr(acc=p + 16388)
    with pytest.raises(E, match="aligned"):
        tr(v=p + 2)
    with pytest.raises(E, match="acc must not overlap v or w"):
        tr(acc=p + 512)                                                           # inside v's 4 x 64 floats
    with pytest.raises(E, match="acc must not overlap v or w"):
        tr(acc=p + 4096 + 1016)                                                   # the last 8 bytes of w
    hs = lambda **kw: L.afd_ode_heun_step(*[kw.get(n, d) for n, d in (("x", p), ("es", p + 4096), ("eu", p + 8192), ("ah", p + 32768),
                                                                      ("s", 1), ("u", 2), ("out", p + 12288), ("n", 1024),
                                                                      ("stream", None))])
    for name in ("x", "es", "eu", "ah", "out"):
        with pytest.raises(E, match="must not be NULL"):
            hs(**{name: None})
    with pytest.raises(E, match="n must be positive"):
        hs(n=0)
    for s, u in ((0, 1), (-1, 5), (5, 5), (7, 3)):
        with pytest.raises(E, match="need 1 <= s < u"):
            hs(s=s, u=u)
    with pytest.raises(E, match="x_out must not overlap eps_s or eps_u"):
        hs(out=p + 4096)
    with pytest.raises(E, match="x_out must not overlap eps_s or eps_u"):
        hs(out=p + 8192 + 4092)
    with pytest.raises(E, match="x itself or apart"):
        hs(out=p + 16, es=p + 16384, eu=p + 24576)


# ---- the coefficients of J_eps = c1 I + c2 J_out ---------------------------------------------------------------------------------
@pytest.mark.parametrize("prediction", ["eps", "v", "x0"])
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_eps_jacobian_coefficients_match_autograd(afdm, prediction, schedule):
    diff = afdm.Diffusion(noise_steps=1000, img_size=4, device="cpu", prediction=prediction, schedule=schedule)
    g = torch.Generator().manual_seed(3)
    A = torch.randn(16, 16, generator=g, dtype=torch.float64)                      # out = A x + b, a random linear model on 1 x 4 x 4
    b = torch.randn(16, generator=g, dtype=torch.float64)
    x = torch.randn(16, generator=g, dtype=torch.float64)
    ts = [1, 500, 999]
    c1, c2 = diff.eps_jacobian_coefficients(torch.tensor(ts))
    assert c1.dtype == torch.float64 and c2.dtype == torch.float64 and tuple(c1.shape) == (3,) and tuple(c2.shape) == (3,)
    for k, t in enumerate(ts):
        ah = diff.alpha_hat.double()[t]
        sa, sb = ah.sqrt(), (1 - ah).sqrt()

        def eps_of(xx):                                                            # eps from the output by its definition
            out = A @ xx + b
            if prediction == "eps":
                return out
            if prediction == "v":                                                  # v = sa eps - sb x0, x_t = sa x0 + sb eps
                return sb * xx + sa * out
            return (xx - sa * out) / sb                                            # out = x0
        J = torch.autograd.functional.jacobian(eps_of, x)
        want = float(c1[k]) * torch.eye(16, dtype=torch.float64) + float(c2[k]) * A
        e = float((J - want).norm() / J.norm())
        note(f"likelihood host: J_eps = c1 I + c2 J_out vs autograd ({prediction})", e, (schedule, t))
        assert e <= 1e-12
        # eps itself is c1 x + c2 out: what the reference path relies on
        assert float((eps_of(x) - (float(c1[k]) * x + float(c2[k]) * (A @ x + b))).norm() / eps_of(x).norm()) <= 1e-12


# ---- accuracy of both rules on Gaussian data, through the reference path ------------------------------------------------------------
VARIANCES = (0.05, 0.25, 1.0)


@pytest.fixture(scope="module")
def gaussian_runs(afdm):
    """{(method, S): the error of log p in nats per dimension, (4,)} for images (4, 3, 8, 8) with per-channel data variances
    0.05 / 0.25 / 1.0, the exact eps model, T = 1000 linear, ddim_timesteps(S), Rademacher, P = 1."""
    diff = afdm.Diffusion(noise_steps=1000, img_size=8, device="cpu")
    ah = diff.alpha_hat.double()
    s2 = torch.tensor(VARIANCES, dtype=torch.float64).view(1, 3, 1, 1)

    def out_fn(x, t):
        a = float(ah[t])
        return math.sqrt(1 - a) * x / (a * s2 + 1 - a)
    g = torch.Generator().manual_seed(0)
    V0 = float(ah[0]) * s2 + 1 - float(ah[0])
    x0 = torch.randn(4, 3, 8, 8, generator=g, dtype=torch.float64) * V0.sqrt()
    exact = (-(x0 * x0) / (2 * V0) - 0.5 * torch.log(2 * math.pi * V0)).flatten(1).sum(1)
    v = (torch.randint(0, 2, (1, 4, 3, 8, 8), generator=g) * 2 - 1).double()
    runs = {}
    for method in ("heun", "euler"):
        for S in (50, 100):
            levels = [0] + list(reversed(diff.ddim_timesteps(S)))
            res = afdm.ode_likelihood_reference(out_fn, x0, diff.alpha_hat, levels, v, method)
            runs[method, S] = (res["logp"] - exact) / 192
            assert float(res["trace_sem"].abs().max()) == 0.0
    return runs


def test_heun_is_accurate_to_a_hundredth_of_a_nat_per_dimension_at_100_steps(gaussian_runs):
    err = gaussian_runs["heun", 100]
    note("likelihood host: |error| of log p, heun S = 100, nats / dim (absolute)", float(err.abs().max()))
    assert float(err.abs().max()) <= 1e-2                                           # measured 4.9e-3 .. 5.2e-3


@pytest.mark.parametrize("method,lo,hi", [("heun", 3.5, 4.7), ("euler", 1.8, 2.2)])
def test_halving_the_step_divides_the_error_by_the_rules_order(gaussian_runs, method, lo, hi):
    ratio = gaussian_runs[method, 50] / gaussian_runs[method, 100]                  # measured 4.08 .. 4.10 and 1.975 .. 1.976
    print(f"{method}: err(50) / err(100) = {ratio.tolist()}")
    assert bool(((ratio >= lo) & (ratio <= hi)).all()), ratio.tolist()


# ---- the exact trace on a non-diagonal Jacobian ---------------------------------------------------------------------------------
def _matrix_model():
    g = torch.Generator().manual_seed(11)
    M = torch.randn(64, 64, generator=g, dtype=torch.float64) / 8
    f = lambda t: 0.5 + t / 1000.0
    return M, f, (lambda x, t: f(t) * (x.flatten(1) @ M.T).view_as(x))


def test_basis_probes_give_the_exact_trace_per_evaluation(afdm):
    from afdm import likelihood
    diff = afdm.Diffusion(noise_steps=1000, img_size=8, device="cpu")
    M, f, out_fn = _matrix_model()
    x0 = torch.randn(2, 1, 8, 8, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    v = likelihood.basis_probes(2, (1, 8, 8))
    assert tuple(v.shape) == (64, 2, 1, 8, 8) and float(v.sum()) == 128.0
    levels = [0, 1, 100, 400, 800]
    for method, count in (("heun", 1 + 2 * 3), ("euler", 4)):
        res = afdm.ode_likelihood_reference(out_fn, x0, diff.alpha_hat, levels, v, method)
        assert len(res["evaluations"]) == count
        want_total = torch.zeros(2, dtype=torch.float64)
        for ev in res["evaluations"]:
            want = f(ev["t"]) * float(torch.trace(M))
            got = ev["tr"].sum(0)
            assert float((got - want).abs().max()) <= 1e-12 * abs(want), (method, ev["t"])
            want_total += ev["weight"] * want
        assert float((res["trace_probes"].sum(0) - want_total).abs().max()) <= 1e-12 * float(want_total.abs().max())
    assert [ev["t"] for ev in res["evaluations"]] == [1, 100, 400, 800]            # euler evaluates at the upper level
    res = afdm.ode_likelihood_reference(out_fn, x0, diff.alpha_hat, levels, v, "heun")
    assert [ev["t"] for ev in res["evaluations"]] == [1, 1, 100, 100, 400, 400, 800]


@pytest.mark.parametrize("method", ["heun", "euler"])
def test_reference_path_equals_a_hand_loop_over_the_same_probes(afdm, method):
    diff = afdm.Diffusion(noise_steps=1000, img_size=8, device="cpu")
    M, f, out_fn = _matrix_model()
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 1, 8, 8, generator=g, dtype=torch.float64)
    v = (torch.randint(0, 2, (3, 2, 1, 8, 8), generator=g) * 2 - 1).double()
    levels = [0, 1, 250, 600, 999]
    res = afdm.ode_likelihood_reference(out_fn, x0, diff.alpha_hat, levels, v, method)
    # by hand: J_eps = f(t) M for every x, so v^T J v = f(t) v^T M v, and the state moves with eps = f(t) M x
    ah = diff.alpha_hat.double()
    a = [float(ah[t]) for t in levels]
    sig = [math.sqrt((1 - q) / q) for q in a]
    quad = torch.einsum("pni,ij,pnj->pn", v.flatten(2), M, v.flatten(2))
    x = x0.flatten(1)
    trace = torch.zeros(3, 2, dtype=torch.float64)
    for k in range(4):
        s, u, h = levels[k], levels[k + 1], sig[k + 1] - sig[k]
        if method == "euler" or s == 0:
            trace += h * math.sqrt(a[k + 1]) * f(u) * quad
            x = math.sqrt(a[k + 1]) * (x / math.sqrt(a[k]) + h * f(u) * (x @ M.T))
            continue
        es = f(s) * (x @ M.T)
        pred = math.sqrt(a[k + 1]) * (x / math.sqrt(a[k]) + h * es)
        eu = f(u) * (pred @ M.T)
        trace += 0.5 * h * (math.sqrt(a[k]) * f(s) + math.sqrt(a[k + 1]) * f(u)) * quad
        x = math.sqrt(a[k + 1]) * (x / math.sqrt(a[k]) + 0.5 * h * (es + eu))
    assert float((res["trace_probes"] - trace).abs().max()) <= 1e-12 * float(trace.abs().max())
    assert float((res["latents"].flatten(1) - x).norm() / x.norm()) <= 1e-13
    assert float((res["trace"] - trace.mean(0)).abs().max()) <= 1e-12 * float(trace.abs().max())
    sem = trace.std(0, unbiased=True) / math.sqrt(3)
    assert float((res["trace_sem"] - sem).abs().max()) <= 1e-12 * float(sem.max())
    prior = -0.5 * (x * x).sum(1) - 32 * math.log(2 * math.pi)
    logp = prior + 32 * (math.log(a[-1]) - math.log(a[0])) + trace.mean(0)
    assert float((res["prior_logp"] - prior).abs().max()) <= 1e-12 * float(prior.abs().max())
    assert float((res["logp"] - logp).abs().max()) <= 1e-12 * float(logp.abs().max())
    # bpd is the stated affine image of logp
    bpd = -res["logp"] / (64 * math.log(2.0)) + math.log2(127.5)
    assert float((res["bpd"] - bpd).abs().max()) <= 1e-13 * float(bpd.abs().max())


def test_reference_refuses_bad_levels_and_probes(afdm):
    diff = afdm.Diffusion(noise_steps=100, img_size=8, device="cpu")
    x0 = torch.zeros(1, 1, 8, 8)
    v = torch.ones(1, 1, 1, 8, 8)
    fn = lambda x, t: x
    for levels in ([1, 5], [0], [0, 5, 5], [0, 9, 4]):
        with pytest.raises(ValueError, match="levels must ascend from 0"):
            afdm.ode_likelihood_reference(fn, x0, diff.alpha_hat, levels, v)
    with pytest.raises(ValueError, match="unknown method"):
        afdm.ode_likelihood_reference(fn, x0, diff.alpha_hat, [0, 5], v, "rk4")
    with pytest.raises(ValueError, match="probes_tensor must be"):
        afdm.ode_likelihood_reference(fn, x0, diff.alpha_hat, [0, 5], torch.ones(1, 2, 1, 8, 8))


# ---- dequantisation and the probes ------------------------------------------------------------------------------------------------
def test_dequantize_stays_within_half_a_level_and_probes_are_what_they_say(afdm):
    from afdm import likelihood
    diff = afdm.Diffusion(noise_steps=50, img_size=8, device="cpu")
    g = torch.Generator().manual_seed(4)
    images = torch.rand(3, 3, 8, 8, generator=g) * 2 - 1
    images[0, 0, 0, :4] = torch.tensor([-1.0, 1.0, 0.0, 0.999])
    snapped = diff.snap_8bit(images)
    torch.manual_seed(7)
    got = diff.dequantize(images, "cpu")
    torch.manual_seed(7)
    u = torch.rand(3, 3, 8, 8)
    assert got.dtype == torch.float32 and torch.equal(got, snapped + (u - 0.5) / 127.5)         # one draw, the stated expression
    gap = (got.double() - snapped.double()).abs().max()
    assert float(gap) <= 0.5 / 127.5 + 1e-7                                         # half a level, and one fp32 rounding at |x| <= 1
    assert float(gap) > 0.4 / 127.5                                                 # (and the noise is there)
    torch.manual_seed(9)
    r = likelihood.draw_probes("rademacher", 2, 3, (3, 8, 8))
    torch.manual_seed(9)
    assert torch.equal(r, (torch.randint(0, 2, (2, 3, 3, 8, 8)) * 2 - 1).float())
    assert r.dtype == torch.float32 and bool((r.abs() == 1).all()) and 0.3 < float((r > 0).float().mean()) < 0.7
    torch.manual_seed(9)
    n = likelihood.draw_probes("gaussian", 2, 3, (3, 8, 8))
    torch.manual_seed(9)
    assert torch.equal(n, torch.randn(2, 3, 3, 8, 8))
    state = torch.get_rng_state()
    b = likelihood.draw_probes("basis", 5, 2, (1, 2, 2))
    assert torch.equal(torch.get_rng_state(), state) and tuple(b.shape) == (4, 2, 1, 2, 2)     # nothing drawn, `probes` ignored
    assert torch.equal(b[:, 1].flatten(1), torch.eye(4))
    with pytest.raises(ValueError, match="unknown probe"):
        likelihood.draw_probes("sphere", 1, 1, (1, 2, 2))


# ---- refusals of Diffusion.ode_likelihood ----------------------------------------------------------------------------------------
class _Never(torch.nn.Module):
    """A model that must not be called."""
    calls = 0

    def forward(self, x, t, y=None):
        type(self).calls += 1
        raise AssertionError("the model was called before the checks passed")


def test_ode_likelihood_refusals_never_call_the_model(afdm):
    diff = afdm.Diffusion(noise_steps=50, img_size=16, device="cpu")
    x = torch.zeros(2, 3, 16, 16)
    model = _Never()
    bad = lambda: pytest.raises(ValueError, match=r"^Diffusion\.ode_likelihood: ")
    for method in ("rk4", "Heun", None, 2):
        with bad():
            diff.ode_likelihood(model, x, 5, method=method)
    for probe in ("sphere", "Rademacher", None, 1):
        with bad():
            diff.ode_likelihood(model, x, 5, probe=probe)
    for probes in (0, -1, 1.0, "1", None, True):
        with bad():
            diff.ode_likelihood(model, x, 5, probes=probes)
    for source in ("reference", "cuda", None, 0):
        with bad():
            diff.ode_likelihood(model, x, 5, noise_source=source)
    for images in (torch.zeros(2, 3, 8, 8), torch.zeros(3, 16, 16), torch.zeros(2, 3, 16, 16, dtype=torch.float64),
                   torch.zeros(0, 3, 16, 16), torch.zeros(2, 3, 16, 16, dtype=torch.uint8), [[0.0]]):
        with bad():
            diff.ode_likelihood(model, images, 5)
    for steps in (0, 50, 2.0, True, None, [5, 5], [3, 7], [0], [50], [], "10"):
        with bad():
            diff.ode_likelihood(model, x, steps)
    with bad():
        diff.ode_likelihood(model, x, 5, labels=torch.zeros(2, dtype=torch.long))  # labels on an unconditional model
    learned = afdm.Diffusion(noise_steps=50, img_size=16, device="cpu", variance="learned")
    with pytest.raises(ValueError, match=r"^Diffusion\.ode_likelihood: variance='learned'"):
        learned.ode_likelihood(model, x, 5)
    assert _Never.calls == 0
    params = list(inspect.signature(afdm.Diffusion.ode_likelihood).parameters)
    assert "cfg_scale" not in params and "graph" not in params and "theta" not in params      # not offered: see the docstring


def test_likelihood_results_checks_first(afdm):
    images = torch.zeros(4, 3, 16, 16, dtype=torch.uint8)
    for n in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="likelihood_results: n must be an int in"):
            afdm.likelihood_results({}, images, n=n)                               # (fails before the checkpoint is read)
    with pytest.raises(ValueError, match="likelihood_results: images must be"):
        afdm.likelihood_results({}, images.float(), n=2)
