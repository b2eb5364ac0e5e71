"""Training objectives, host side: the cosine noise schedule, v- / x0-prediction targets, Min-SNR weights, argument errors.
No GPU: tables, formulas and validation only (the kernels are checked in test_gpu_objective.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import note

P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int


def _diff(T=1000, **kw):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu", **kw)


def _cosine_beta64(T, s=0.008):
    f = [math.cos(((u / T + s) / (1.0 + s)) * (math.pi / 2.0)) ** 2 for u in range(T + 1)]
    return np.array([min(1.0 - f[t + 1] / f[t], 0.999) for t in range(T)], dtype=np.float64)


@pytest.mark.parametrize("T", (10, 300, 1000))
def test_cosine_tables_against_the_closed_form(T):
    d = _diff(T, schedule="cosine")
    want = _cosine_beta64(T)
    assert d.beta.dtype == torch.float32 and tuple(d.beta.shape) == (T,)
    # exactly, after the single rounding to fp32
    assert torch.equal(d.beta, torch.from_numpy(want.astype(np.float32)))
    assert float(d.beta.max()) <= np.float32(0.999) and float(d.beta.min()) > 0
    assert torch.equal(d.alpha, 1.0 - d.beta)
    assert torch.equal(d.alpha_hat, torch.cumprod(1.0 - d.beta, dim=0))
    ah = d.alpha_hat.double()
    assert bool((ah[1:] < ah[:-1]).all()) and float(ah.min()) > 0 and float(ah.max()) < 1
    # and the product follows f(t + 1) / f(0) until the clip at 0.999 sets in
    f = np.cos(((np.arange(T + 1) / T + 0.008) / 1.008) * (np.pi / 2)) ** 2
    free = np.nonzero(want < 0.999)[0]
    e = float(np.max(np.abs(ah.numpy()[free] / (f[free + 1] / f[0]) - 1.0)))
    note("cosine alpha_hat vs f(t+1)/f(0) (max rel)", e, f"T={T}")
    assert e < 1e-4, e                    # T fp32 factors of relative error 2^-24 each: at most 1000 * 6e-8


def test_cosine_offset_is_an_argument():
    a, b = _diff(50, schedule="cosine"), _diff(50, schedule="cosine", cosine_s=0.02)
    assert torch.equal(b.beta, torch.from_numpy(_cosine_beta64(50, 0.02).astype(np.float32)))
    assert not torch.equal(a.beta, b.beta)


def test_linear_is_the_default_bit_for_bit():
    a, b = _diff(), _diff(schedule="linear", prediction="eps")
    for k in ("beta", "alpha", "alpha_hat"):
        assert torch.equal(getattr(a, k), getattr(b, k))
    assert torch.equal(a.beta, torch.linspace(1e-4, 0.02, 1000))
    assert a.schedule == "linear" and a.prediction == "eps"


@pytest.mark.parametrize("T", (10, 1000))
def test_samplers_host_tables_on_the_cosine_schedule(T):
    d, lin = _diff(T, schedule="cosine"), _diff(T)
    for S in sorted({1, 2, 10, 50, T - 1} & set(range(1, T))):
        r = d.logsnr_timesteps(S)
        assert len(r) == S and r[0] == T - 1 and all(a > b for a, b in zip(r, r[1:])) and (S == 1 or r[-1] == 1)
        assert bool(torch.isfinite(d.dpmpp_coefficients(d.dpmpp_pairs(S))).all())
        assert d.ddim_timesteps(S) == lin.ddim_timesteps(S)
    for sigma in ("beta", "posterior"):
        assert bool(torch.isfinite(d.vlb_coefficients(sigma)).all())


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("gamma", (1.0, 5.0, 20.0))
def test_snr_weights_follow_the_formulas(schedule, gamma):
    ah = _diff(schedule=schedule).alpha_hat.double()
    snr = ah / (1.0 - ah)
    m = torch.minimum(snr, torch.tensor(gamma, dtype=torch.float64))
    want = {"eps": m / snr, "x0": m, "v": m / (snr + 1.0)}
    for kind in ("eps", "v", "x0"):
        w = _diff(schedule=schedule, prediction=kind).snr_weights("min_snr", gamma)
        assert w.dtype == torch.float64 and tuple(w.shape) == (1000,) and not w.is_cuda
        assert torch.equal(w, want[kind])
        assert bool((w > 0).all()) and bool(torch.isfinite(w).all())
        if kind != "x0":
            assert float(w.max()) <= 1.0
    # continuous where the clip sets in: the two branches of each weight meet at snr = gamma ...
    for below, above in ((lambda s: 1.0, lambda s: gamma / s), (lambda s: s, lambda s: gamma),
                         (lambda s: s / (s + 1.0), lambda s: gamma / (s + 1.0))):
        assert abs(below(gamma) - above(gamma)) < 1e-15
    # ... and as functions of snr they are Lipschitz on both sides (|d/ds| of 1, gamma / s (s >= gamma), s, gamma, s / (s + 1),
    # gamma / (s + 1) is at most max(1, gamma, 1 / gamma)), so no step of the table exceeds that times the step of snr
    lip = max(1.0, gamma, 1.0 / gamma)
    for kind in ("eps", "v", "x0"):
        w = _diff(schedule=schedule, prediction=kind).snr_weights("min_snr", gamma)
        assert bool(((w[1:] - w[:-1]).abs() <= lip * (snr[1:] - snr[:-1]).abs() * (1 + 1e-12)).all()), kind


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
def test_training_target_round_trip_in_fp64(schedule):
    g = torch.Generator().manual_seed(3)
    B = 64
    x0 = torch.rand(B, 3, 8, 8, generator=g, dtype=torch.float64) * 2 - 1
    eps = torch.randn(B, 3, 8, 8, generator=g, dtype=torch.float64)
    t = torch.randint(0, 1000, (B,), generator=g)
    t[:2] = torch.tensor([0, 999])
    for kind in ("eps", "v", "x0"):
        d = _diff(schedule=schedule, prediction=kind)
        ah = d.alpha_hat.double()[t].reshape(B, 1, 1, 1)
        sa, sb = torch.sqrt(ah), torch.sqrt(1.0 - ah)
        x_t = sa * x0 + sb * eps
        tgt = d.training_target(x0, eps, t)
        assert tgt.dtype == torch.float64 and tgt.shape == x0.shape
        if kind == "eps":
            assert tgt is eps
            continue
        if kind == "x0":
            assert tgt is x0
            back = (x_t - sa * tgt) / sb                               # the conversion's formula gives eps back ...
            e = float(((back - eps).abs() / (1.0 + eps.abs() / sb)).max())        # (the division by sb amplifies x_t's rounding)
        else:
            assert torch.equal(tgt, sa * eps - sb * x0)
            back = sa * tgt + sb * x_t
            e = float((back - eps).abs().max())
            x0_back = sa * x_t - sb * tgt                              # ... and v gives x0 back
            assert float((x0_back - x0).abs().max()) < 1e-13
        note(f"training_target round trip fp64 ({kind})", e, schedule)
        assert e < 1e-13, (kind, e)


def test_argument_errors():
    import afdm
    for kw, pat in ((dict(schedule="quadratic"), "schedule.*'linear' or 'cosine'"), (dict(schedule=None), "schedule"),
                    (dict(prediction="velocity"), "prediction.*'eps', 'v' or 'x0'"), (dict(prediction=1), "prediction"),
                    (dict(schedule="cosine", cosine_s=-1.0), "cosine_s"), (dict(schedule="cosine", cosine_s="a"), "cosine_s")):
        with pytest.raises(ValueError, match=pat):
            _diff(10, **kw)
    d = _diff(10)
    with pytest.raises(ValueError, match="snr_weights: unknown kind"):
        d.snr_weights("p2", 5.0)
    for gamma in (0, -1.0, float("nan"), float("inf"), True, "5"):
        with pytest.raises(ValueError, match="gamma"):
            d.snr_weights("min_snr", gamma)
    model = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="TrainStep: unknown loss_weighting 'p2'"):
        afdm.TrainStep(model, d, lr=1e-3, loss_weighting="p2")
    for gamma in (0, -2.0, float("nan"), None):
        with pytest.raises(ValueError, match="TrainStep: snr_gamma"):
            afdm.TrainStep(model, d, lr=1e-3, loss_weighting="min_snr", snr_gamma=gamma)


def test_predict_eps_is_the_models_own_tensor_for_eps_prediction():
    d = _diff(10)
    x, t, y = torch.zeros(2, 1, 4, 4), torch.tensor([1, 2]), torch.tensor([0, 1])
    outs, calls = [], []

    def model(*a):
        calls.append(a)
        outs.append(torch.ones(2, 1, 4, 4))
        return outs[-1]
    assert d.predict_eps(model, x, t) is outs[0] and len(calls[0]) == 2
    assert d.predict_eps(model, x, t, y) is outs[1] and calls[1][2] is y
    import afdm
    with pytest.raises(afdm.AfdError, match="HIP device"):             # a conversion is device work: no CPU fallback
        _diff(10, prediction="v").predict_eps(model, x, t)


def test_drop_in_keys_reach_the_diffusion_and_only_when_present():
    import afdm
    from afdm.training import diffusion_kwargs
    assert diffusion_kwargs(afdm.argument()) == {}
    assert diffusion_kwargs(afdm.argument(noise_schedule="cosine", prediction="v")) == {"schedule": "cosine", "prediction": "v"}
    a = afdm.argument(loss_weighting="min_snr", snr_gamma=3.0)
    assert (a.loss_weighting, a.snr_gamma, a.prediction, a.noise_schedule) == ("min_snr", 3.0, None, None)


def test_header_declares_and_types_the_objective_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_objective_loss_fwd"] == (ctypes.c_int, [P, P, P, P, P, P, I, P, P, L, L, P])
    assert sigs["afd_objective_loss_bwd"] == (ctypes.c_int, [P, P, P, P, P, P, I, P, P, L, L, P])
    assert sigs["afd_pred_to_eps"] == (ctypes.c_int, [P, P, P, P, I, P, L, L, P])
    src = open(__import__("afdm")._lib.HEADER).read()
    for name, v in (("AFD_PRED_EPS", 0), ("AFD_PRED_V", 1), ("AFD_PRED_X0", 2)):
        assert f"#define {name} {v}" in src
    import afdm
    assert afdm.ops.PRED_KINDS == {"eps": 0, "v": 1, "x0": 2}


def test_objective_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_float * 4096)()
    at = lambda i: ctypes.addressof(buf) + 4 * i
    fwd = [at(0), at(64), at(128), at(192), at(256), None, 1, at(320), at(384), 2, 8, None]
    bwd = [at(0), at(64), at(128), at(192), at(256), None, 1, at(320), at(384), 2, 8, None]
    cvt = [at(0), at(64), at(192), at(256), 1, at(0), 2, 8, None]
    for fn, args, ptrs, ikind, idims in ((lib.afd_objective_loss_fwd, fwd, (0, 1, 2, 3, 4, 7, 8), 6, (9, 10)),
                                         (lib.afd_objective_loss_bwd, bwd, (0, 1, 2, 3, 4, 7, 8), 6, (9, 10)),
                                         (lib.afd_pred_to_eps, cvt, (0, 1, 2, 3, 5), 4, (6, 7))):
        name = fn.__name__
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            with pytest.raises(afdm.AfdError, match=f"{name}: .*NULL"):
                fn(*bad)
        for k in (-1, 3, 7):
            bad = list(args)
            bad[ikind] = k
            with pytest.raises(afdm.AfdError, match=f"{name}: kind must be"):
                fn(*bad)
        for i in idims:
            for v in (0, -4):
                bad = list(args)
                bad[i] = v
                with pytest.raises(afdm.AfdError, match=f"{name}: .*positive"):
                    fn(*bad)
    bad = list(cvt)
    bad[4] = 0                                                           # an eps output needs no conversion: never launched
    with pytest.raises(afdm.AfdError, match="afd_pred_to_eps: kind must be AFD_PRED_V or AFD_PRED_X0"):
        lib.afd_pred_to_eps(*bad)
    # the torch-level wrappers: host tensors, unknown kinds, mismatched shapes
    x = torch.zeros(2, 3, 4, 4)
    t, ah = torch.tensor([1, 2]), torch.full((10,), 0.5)
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.objective_loss(x, x, x, t, ah, None, "v")
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.pred_to_eps(x, x, t, ah, "x0")
    with pytest.raises(afdm.AfdError, match="unknown prediction 'velocity'"):
        afdm.ops.objective_loss(x, x, x, t, ah, None, "velocity")
    with pytest.raises(afdm.AfdError, match="unknown prediction None"):
        afdm.ops.pred_to_eps(x, x, t, ah, None)
