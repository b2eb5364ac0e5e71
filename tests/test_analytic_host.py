"""CPU-side tests of Analytic-DPM (Bao et al. 2022): `AnalyticVariance.sigma2` against a restated fp64 loop and against the true
conditional variance of Gaussian data, the variance recursion of a short chain with and without the analytic table, clipping,
the checks, the .npz round trip, `vlb_coefficients(av)`, the C ABI of the six entry points with their argument checks (which
return before any device is touched), and the `sample_analytic` requests that are refused before any device work."""
import ctypes
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
T = 1000
CHAINS = [1, 5, 10, [999, 640, 120, 40, 3], T - 1]
ETAS = [0.0, 0.5, 1.0]


def _diff(noise_steps=T, **kw):
    import afdm
    return afdm.Diffusion(noise_steps=noise_steps, img_size=32, device="cpu", **kw)


def _ah(d):
    return d.alpha_hat.double().numpy()


def _gauss_gamma(d, s2=0.25):
    """G_t of the exact eps-model of x0 ~ N(mu, s2 I): eps_hat = sqrt(1 - a) (x_t - sqrt(a) mu) / (s2 a + 1 - a), whose second
    moment per element is (1 - a) / (s2 a + 1 - a)."""
    a = _ah(d)
    return (1.0 - a) / (s2 * a + 1.0 - a)


def _table(d, gamma):
    import afdm
    g = np.asarray(gamma, dtype=np.float64)
    return afdm.AnalyticVariance(g, (~np.isnan(g)).astype(np.int64), d.noise_steps, d.schedule, d.prediction, d.alpha_hat)


def _lam2_dir(a_t, a_p, eta):
    lam2 = eta * eta * ((1.0 - a_p) / (1.0 - a_t)) * (1.0 - a_t / a_p)
    return lam2, math.sqrt(max((1.0 - a_p) - lam2, 0.0))


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("chain", CHAINS)
def test_sigma2_matches_the_restated_formula(chain, eta):
    d = _diff()
    rng = np.random.default_rng(3)
    gamma = rng.uniform(0.0, 1.0, T)
    av = _table(d, gamma)
    pairs = d._ddim_pairs(chain, eta)
    got = av.sigma2(d, pairs, eta)
    assert got.dtype == np.float64 and got.shape == (len(pairs),)
    a = _ah(d)
    for k, (t, p) in enumerate(pairs):
        lam2, dr = _lam2_dir(a[t], a[p], eta)
        want = lam2 + (math.sqrt((1.0 - a[t]) * a[p] / a[t]) - dr) ** 2 * (1.0 - gamma[t])
        assert abs(got[k] - want) <= 1e-12 * want, (t, p, got[k], want)
    tab = av.sigma_table(d, pairs, eta)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (T,)
    want_tab = np.zeros(T)
    want_tab[[t for t, _ in pairs]] = np.sqrt(got)
    assert np.array_equal(tab.numpy(), want_tab.astype(np.float32))          # rounded once, zero elsewhere


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("chain", CHAINS)
def test_gaussian_identity(chain, eta):
    """For Gaussian data the reverse conditional is Gaussian and its variance is known: sigma*2 must be that variance."""
    d = _diff()
    av = _table(d, _gauss_gamma(d))
    pairs = d._ddim_pairs(chain, eta)
    got = av.sigma2(d, pairs, eta)
    a = _ah(d)
    worst = 0.0
    for k, (t, p) in enumerate(pairs):
        lam2, dr = _lam2_dir(a[t], a[p], eta)
        post = 0.25 * (1.0 - a[t]) / (0.25 * a[t] + 1.0 - a[t])            # Var(x0 | x_t)
        want = lam2 + (math.sqrt(a[p]) - dr * math.sqrt(a[t] / (1.0 - a[t]))) ** 2 * post
        worst = max(worst, abs(got[k] - want) / want)
    assert worst <= 1e-9, worst


def _final_variance(d, pairs, eta, s2):
    """Variance per element of the chain's final sample for x0 ~ N(mu, 0.25 I) and its exact eps-model, started at variance 1:
    each step is linear in (x - sqrt(a_t) mu), so the variance follows v' = c^2 v + s2, with no noise on the last step."""
    a = _ah(d)
    v = 1.0
    for k, (t, p) in enumerate(pairs):
        _, dr = _lam2_dir(a[t], a[p], eta)
        e = math.sqrt(1.0 - a[t]) / (0.25 * a[t] + 1.0 - a[t])             # eps_hat = e (x - sqrt(a_t) mu)
        c = math.sqrt(a[p]) / math.sqrt(a[t]) * (1.0 - math.sqrt(1.0 - a[t]) * e) + dr * e
        v = c * c * v + (s2[k] if p > 0 else 0.0)
    return v


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("S", [5, 10, 20, 50])
def test_variance_recursion(S, eta):
    d = _diff()
    av = _table(d, _gauss_gamma(d))
    pairs = d._ddim_pairs(S, eta)
    a = _ah(d)
    target = 0.25 * a[0] + 1.0 - a[0]
    analytic = _final_variance(d, pairs, eta, av.sigma2(d, pairs, eta))
    plain = _final_variance(d, pairs, eta, [_lam2_dir(a[t], a[p], eta)[0] for t, p in pairs])
    assert abs(analytic - target) <= 1e-3, (analytic, target)
    assert plain < 0.9 * target, (plain, target)                            # lambda^2 alone: more than 10 % short


def test_gamma_outside_the_unit_interval_is_clipped():
    d = _diff()
    pairs = d._ddim_pairs(10, 1.0)
    g = np.full(T, 0.5)
    lo, hi = g.copy(), g.copy()
    lo[pairs[2][0]], hi[pairs[2][0]] = -0.25, 0.0
    assert np.array_equal(_table(d, lo).sigma2(d, pairs, 1.0), _table(d, hi).sigma2(d, pairs, 1.0))
    lo[pairs[2][0]], hi[pairs[2][0]] = 1.75, 1.0
    top = _table(d, lo).sigma2(d, pairs, 1.0)
    assert np.array_equal(top, _table(d, hi).sigma2(d, pairs, 1.0))
    a = _ah(d)
    assert top[2] == _lam2_dir(a[pairs[2][0]], a[pairs[2][1]], 1.0)[0]      # G = 1: lambda^2 alone


def test_last_sigma_max_caps_only_the_last_noisy_step():
    d = _diff()
    av = _table(d, _gauss_gamma(d))
    for chain in (10, [999, 640, 120, 40, 3]):
        pairs = d._ddim_pairs(chain, 0.0)
        free = av.sigma2(d, pairs, 0.0)
        cap = 0.5 * math.sqrt(free[-2])
        got = av.sigma2(d, pairs, 0.0, last_sigma_max=cap)
        assert pairs[-1][1] == 0 and pairs[-2][1] > 0
        assert got[-2] == cap * cap
        assert np.array_equal(np.delete(got, -2), np.delete(free, -2))
        assert np.array_equal(av.sigma2(d, pairs, 0.0, last_sigma_max=10.0), free)     # a cap above sigma* changes nothing
        assert float(av.sigma_table(d, pairs, 0.0, last_sigma_max=cap)[pairs[-2][0]]) == np.float32(cap)
    one = d._ddim_pairs(1, 0.0)                                             # no noisy step: nothing to cap
    assert np.array_equal(av.sigma2(d, one, 0.0, last_sigma_max=0.0), av.sigma2(d, one, 0.0))
    with pytest.raises(ValueError, match="last_sigma_max"):
        av.sigma2(d, one, 0.0, last_sigma_max=-1.0)


def test_missing_timesteps_and_foreign_processes_are_refused():
    d = _diff()
    g = np.full(T, np.nan)
    chain = d.ddim_timesteps(10)
    g[chain] = 0.5
    av = _table(d, g)
    av.sigma2(d, d._ddim_pairs(10, 1.0), 1.0)
    with pytest.raises(ValueError, match="no estimate at timesteps 640, 120"):
        av.sigma2(d, d._ddim_pairs([999, 640, 120, 1], 1.0), 1.0)
    with pytest.raises(ValueError, match="no estimate"):
        av.sigma_table(d, d._ddim_pairs(11, 0.0), 0.0)
    with pytest.raises(ValueError, match="noise_steps = 1000"):
        av.sigma2(_diff(500), [(499, 0)], 1.0)
    with pytest.raises(ValueError, match="another noise schedule"):
        av.sigma2(_diff(schedule="cosine"), d._ddim_pairs(10, 1.0), 1.0)
    with pytest.raises(ValueError, match="another noise schedule"):
        av.sigma2(_diff(beta_end=0.03), d._ddim_pairs(10, 1.0), 1.0)
    with pytest.raises(ValueError, match="eta"):
        av.sigma2(d, d._ddim_pairs(10, 1.0), -1.0)


def test_save_load_round_trip(tmp_path):
    import afdm
    d = _diff(prediction="v")
    g = np.full(T, np.nan)
    g[1:] = np.random.default_rng(5).uniform(0, 1, T - 1)
    av = afdm.AnalyticVariance(g, np.arange(T), T, d.schedule, d.prediction, d.alpha_hat)
    path = tmp_path / "analytic.npz"
    av.save(str(path))
    back = afdm.AnalyticVariance.load(str(path))
    assert back.gamma.tobytes() == av.gamma.tobytes() and back.gamma.dtype == np.float64         # (NaN included)
    assert np.array_equal(back.count, av.count) and back.count.dtype == np.int64
    assert back.alpha_hat.tobytes() == d.alpha_hat.numpy().tobytes() and back.alpha_hat.dtype == np.float32
    assert (back.noise_steps, back.schedule, back.prediction) == (T, "linear", "v")
    pairs = d._ddim_pairs(20, 0.5)
    assert np.array_equal(back.sigma2(d, pairs, 0.5), av.sigma2(d, pairs, 0.5))


def test_vlb_coefficients_of_an_analytic_table():
    d = _diff()
    gamma = _gauss_gamma(d, 0.01)
    av = _table(d, gamma)
    got = d.vlb_coefficients(av).numpy()
    assert got.shape == (T, 4)
    b, al, a = d.beta.double().numpy(), d.alpha.double().numpy(), _ah(d)
    s2 = av.sigma2(d, [(t, t - 1) for t in range(1, T)], 1.0)
    ref = d.vlb_coefficients("posterior").numpy()
    assert np.array_equal(got[:, 3], ref[:, 3]) and not got[0, :3].any()
    for t in range(1, T):
        bt = (1.0 - a[t - 1]) / (1.0 - a[t]) * b[t]
        w = b[t] ** 2 / (2.0 * s2[t - 1] * al[t] * (1.0 - a[t]))
        c = 0.5 * (-1.0 + math.log(s2[t - 1] / bt) + bt / s2[t - 1])
        assert abs(got[t, 0] - w) <= 1e-12 * w
        assert abs(got[t, 1] - c) <= 1e-12 * c + 2e-15, (t, got[t, 1], c)       # (the naive form cancels: a few ulps of 1)
        assert abs(got[t, 2] - 0.5 * math.log(s2[t - 1])) <= 1e-12 * abs(0.5 * math.log(s2[t - 1]))
    # a table that misses a timestep is refused; the strings and their message stay
    hole = gamma.copy()
    hole[17] = np.nan
    with pytest.raises(ValueError, match="no estimate at timestep 17"):
        d.vlb_coefficients(_table(d, hole))
    with pytest.raises(ValueError, match=r"unknown sigma 'best' \('beta' or 'posterior'\)"):
        d.vlb_coefficients("best")
    assert d.VLB_SIGMAS == ("beta", "posterior")


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_analytic_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_ddim_step_var"] == (I, [P, P, P, P, P, I, I, F, P, L, P])
    assert sigs["afd_ddim_step_var_dev"] == (I, [P, P, P, P, P, P, P, F, P, L, P])
    assert sigs["afd_ddim_step_var_cfg"] == (I, [P, P, P, P, P, I, I, F, F, P, P, L, P])
    assert sigs["afd_ddim_step_var_cfg_dev"] == (I, [P, P, P, P, P, P, P, F, F, P, P, L, P])
    assert sigs["afd_eps_sqnorm_rows"] == (I, [P, P, L, L, P])
    assert sigs["afd_eps_sqnorm_rows_cfg"] == (I, [P, F, P, L, L, P])


def test_analytic_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    at = lambda i: base + 4 * i                               # element i of the buffer; never dereferenced
    n = 8
    x, e, z, ah, sg, o, o2, td, tpd = at(0), at(16), at(48), at(64), at(80), at(96), at(112), at(128), at(136)
    forms = {                                                  # name -> (arguments, positions of the required pointers)
        "afd_ddim_step_var": ([x, e, z, ah, sg, 5, 3, 1.0, o, n, None], (0, 1, 3, 4, 8)),
        "afd_ddim_step_var_dev": ([x, e, z, ah, sg, td, tpd, 1.0, o, n, None], (0, 1, 3, 4, 5, 6, 8)),
        "afd_ddim_step_var_cfg": ([x, e, z, ah, sg, 5, 3, 1.0, 3.0, o, o2, n, None], (0, 1, 3, 4, 9)),
        "afd_ddim_step_var_cfg_dev": ([x, e, z, ah, sg, td, tpd, 1.0, 3.0, o, o2, n, None], (0, 1, 3, 4, 5, 6, 9)),
    }
    for name, (good, required) in forms.items():
        fn = getattr(lib, name)
        for j in required:                                    # each required pointer in turn, sig among them
            args = list(good)
            args[j] = None
            with pytest.raises(afdm.AfdError, match=f"{name}: .*sig.* must not be NULL"):
                fn(*args)
        for bad_n in (0, -4):
            args = list(good)
            args[-2] = bad_n
            with pytest.raises(afdm.AfdError, match=f"{name}: n must be positive"):
                fn(*args)
        args = list(good)
        args[7] = -0.5
        with pytest.raises(afdm.AfdError, match=f"{name}: eta must be >= 0"):
            fn(*args)
        args[7] = float("nan")
        with pytest.raises(afdm.AfdError, match=f"{name}: eta must be >= 0"):
            fn(*args)
        if not name.endswith("_dev"):
            for t, tp in ((3, 3), (3, 5), (3, -1)):
                args = list(good)
                args[5], args[6] = t, tp
                with pytest.raises(afdm.AfdError, match=f"{name}: need 0 <= t_prev < t"):
                    fn(*args)
    rows = at(200)
    with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows: eps and rows must not be NULL"):
        lib.afd_eps_sqnorm_rows(None, rows, 2, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows: eps and rows must not be NULL"):
        lib.afd_eps_sqnorm_rows(e, None, 2, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows_cfg: eps2 and rows must not be NULL"):
        lib.afd_eps_sqnorm_rows_cfg(None, 3.0, rows, 2, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows_cfg: eps2 and rows must not be NULL"):
        lib.afd_eps_sqnorm_rows_cfg(e, 3.0, None, 2, 8, None)
    for B, chw in ((0, 8), (-1, 8), (2, 0), (2, -3)):
        with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows: B and chw must be positive"):
            lib.afd_eps_sqnorm_rows(e, rows, B, chw, None)
        with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows_cfg: B and chw must be positive"):
            lib.afd_eps_sqnorm_rows_cfg(e, 3.0, rows, B, chw, None)
    with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows: rows must not overlap"):
        lib.afd_eps_sqnorm_rows(e, at(20), 2, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_eps_sqnorm_rows_cfg: rows must not overlap"):
        lib.afd_eps_sqnorm_rows_cfg(e, 3.0, at(16 + 2 * 8 + 4), 2, 8, None)      # inside the unconditional half


# ---- the public interface ------------------------------------------------------------------------------------------------------
def test_analytic_requests_that_are_refused_before_touching_a_device():
    import afdm
    d = _diff()
    av = _table(d, _gauss_gamma(d))
    m = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    with pytest.raises(ValueError, match=r"steps=999.*full chain"):
        d.sample_analytic(m, 2, 1, av)
    for name in ("dpmpp_2m", "unipc", "unipc_3"):
        with pytest.raises(ValueError, match="analytic goes with sampler None or 'ddim'"):
            d.sample_analytic(m, 2, 1, av, steps=10, sampler=name)
    with pytest.raises(ValueError, match="theta"):
        d.sample_analytic(m, 2, 1, av, steps=10, theta=30)
    dl = _diff(variance="learned")
    m2 = afdm.UNet(c_in=1, c_out=2, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    with pytest.raises(ValueError, match="variance='fixed'"):
        dl.sample_analytic(m2, 2, 1, _table(dl, _gauss_gamma(dl)), steps=10, eta=1.0)
    with pytest.raises(ValueError, match="must be an AnalyticVariance"):
        d.sample_analytic(m, 2, 1, _gauss_gamma(d), steps=10)
    # a table of another process, or one that misses a timestep of the chain
    with pytest.raises(ValueError, match="another noise schedule"):
        d.sample_analytic(m, 2, 1, _table(_diff(schedule="cosine"), _gauss_gamma(d)), steps=10)
    g = np.full(T, np.nan)
    g[d.ddim_timesteps(10)] = 0.5
    with pytest.raises(ValueError, match="no estimate"):
        d.sample_analytic(m, 2, 1, _table(d, g), steps=12, eta=1.0)
    with pytest.raises(ValueError, match="cfg_scale needs class labels"):
        d.sample_analytic(m, 2, 1, av, steps=10, cfg_scale=2.0)
    assert m.training and m._t_range is None
    # the method takes what `sample` takes, with the table after image_channels
    import inspect
    own, base = inspect.signature(afdm.Diffusion.sample_analytic).parameters, inspect.signature(afdm.Diffusion.sample).parameters
    assert [k for k in own if k != "analytic"] == list(base) and list(own)[4] == "analytic"
    assert all(own[k].default == base[k].default for k in base)
