"""CPU-side tests of the bits/dim likelihood: the bound's coefficient table against an independent high-precision restatement,
the row, chunk and timestep-sampling rules, the (T - 1) / K weighting, the 8-bit snapping rule, every argument check of
Diffusion.calc_bpd (all raised before a device is touched), and the C ABI of the three new entry points with their argument
checks (which return before any launch)."""
import ctypes
import decimal
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, L, DBL = ctypes.c_void_p, ctypes.c_long, ctypes.c_double


def _diff(T=1000):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu")


def _model(c=1):
    import afdm
    return afdm.UNet(c_in=c, c_out=c, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)


# ---- the coefficient table ------------------------------------------------------------------------------------------------
def _restated(d, t, sigma):
    """w_t, c_t and the log-scale from the definitions, in 60-digit decimal arithmetic on the fp32 tables."""
    ctx = decimal.Context(prec=60)
    D = lambda v: ctx.create_decimal(float(v))
    b, a = D(d.beta[t]), D(d.alpha[t])
    ah, ahp = D(d.alpha_hat[t]), D(d.alpha_hat[t - 1])
    bt = ctx.multiply(ctx.divide(1 - ahp, 1 - ah), b)
    s2 = b if sigma == "beta" else bt
    w = ctx.divide(b * b, 2 * s2 * a * (1 - ah))
    c = (-1 + ctx.ln(ctx.divide(s2, bt)) + ctx.divide(bt, s2)) / 2
    return float(w), float(c), float(ctx.ln(s2) / 2)


@pytest.mark.parametrize("sigma", ["beta", "posterior"])
@pytest.mark.parametrize("T", [1000, 21])
def test_vlb_coefficients_against_a_high_precision_restatement(sigma, T):
    d = _diff(T)
    tab = d.vlb_coefficients(sigma)
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (T, 4)
    for t in sorted({1, 2, 3, T // 2, T - 1}):
        w, c, ls = _restated(d, t, sigma)
        assert math.isclose(float(tab[t, 0]), w, rel_tol=1e-13), (t, float(tab[t, 0]), w)
        assert math.isclose(float(tab[t, 2]), ls, rel_tol=1e-13), (t, float(tab[t, 2]), ls)
        if sigma == "beta":
            assert math.isclose(float(tab[t, 1]), c, rel_tol=1e-11), (t, float(tab[t, 1]), c)
    one_m = 1.0 - float(d.alpha_hat[T - 1])
    assert torch.all(tab[:, 3] == 0.5 * (-1.0 - math.log(one_m) + one_m))
    assert torch.all(tab[0, :3] == 0)


def test_vlb_coefficients_c_t_signs():
    d = _diff()
    post, beta = d.vlb_coefficients("posterior"), d.vlb_coefficients("beta")
    assert torch.all(post[:, 1] == 0.0)                                   # exactly: s2 = beta~
    c = beta[1:, 1]
    assert torch.all(torch.isfinite(c)) and torch.all(c >= 0) and torch.all(c[1:] > 0)
    # sigma = "posterior" makes each KL term's weight w_t = beta_t / beta~_t times the "beta" one
    bt = torch.exp(2 * post[1:, 2])
    assert torch.allclose(post[1:, 0], beta[1:, 0] * d.beta[1:].double() / bt, rtol=1e-13)


# ---- rows, chunks, timestep sampling, weighting -----------------------------------------------------------------------------
def test_rows_are_image_major_with_t_descending():
    d = _diff(6)
    ts = d.bpd_timesteps(3)
    assert ts == [[5, 4, 3, 2, 1]] * 3
    img, t = d.bpd_rows(ts)
    assert img.tolist() == [0] * 5 + [1] * 5 + [2] * 5 and t.tolist() == [5, 4, 3, 2, 1] * 3
    assert img.dtype == np.int64 and t.dtype == np.int64
    assert d.bpd_timesteps(2, 5) == ts[:2]                                # K = T - 1 is the full bound, nothing drawn
    assert d.bpd_chunks(15, 4) == [(0, 4), (4, 8), (8, 12), (12, 15)]
    assert d.bpd_chunks(15, 15) == [(0, 15)] and d.bpd_chunks(15, 256) == [(0, 15)]
    assert d.bpd_chunks(3, 1) == [(0, 1), (1, 2), (2, 3)]


def test_sampled_timesteps_are_distinct_descending_and_drawn_by_randperm():
    d = _diff(101)
    torch.manual_seed(4)
    ts = d.bpd_timesteps(5, 10, noise_source="cpu")
    after = torch.randn(3)
    torch.manual_seed(4)
    want = [sorted((int(v) + 1 for v in torch.randperm(100)[:10]), reverse=True) for _ in range(5)]
    assert ts == want and torch.equal(after, torch.randn(3))              # one randperm per image, nothing else drawn
    for row in ts:
        assert len(set(row)) == 10 and row == sorted(row, reverse=True) and 1 <= min(row) and max(row) <= 100


def test_combine_weights_the_sampled_terms_by_T_minus_1_over_K():
    d = _diff(11)
    n, per, K = 2, 12, 3
    ts = [[9, 4, 1], [10, 7, 2]]
    img, t = d.bpd_rows(ts)
    term = np.array([1.5, 2.0, 7.0, 0.25, 0.5, 3.0])
    sq = np.arange(6, dtype=np.float64) * per
    prior = np.array([0.125, 4.0])
    r = d.bpd_combine(n, per, img, t, term, sq, prior, K, return_terms=True)
    norm = per * math.log(2)
    s = 10 / 3
    assert torch.allclose(r["vb_bpd"], torch.tensor([s * 3.5, s * 3.75], dtype=torch.float64) / norm, rtol=1e-15)
    assert torch.allclose(r["decoder_bpd"], torch.tensor([s * 7.0, 0.0], dtype=torch.float64) / norm, rtol=1e-15)
    assert torch.allclose(r["prior_bpd"], torch.tensor(prior) / norm, rtol=1e-15)
    assert torch.allclose(r["bpd"], r["prior_bpd"] + r["vb_bpd"] + r["decoder_bpd"], rtol=1e-15)
    assert r["terms"].shape == (2, 11) and r["terms"][0, 1] == 7.0 and r["terms"][1, 7] == 0.5 and r["terms"][0, 7] == 0
    assert float(r["terms"].sum()) == float(term.sum()) and r["mse"][1, 2] == 5.0
    assert all(v.dtype == torch.float64 and v.device.type == "cpu" for v in r.values())
    full = d.bpd_combine(n, per, img, t, term, sq, prior, 10)             # K = T - 1: no scaling
    assert torch.allclose(full["vb_bpd"] * s, r["vb_bpd"], rtol=1e-15) and "terms" not in full


def test_snap_8bit():
    import afdm
    D = afdm.Diffusion
    k = torch.arange(256, dtype=torch.uint8)
    grid = k.float() / 127.5 - 1.0
    assert torch.equal(D.snap_8bit(k), grid)
    assert torch.equal(D.snap_8bit(grid), grid)                          # the grid is a fixed point
    x = torch.tensor([-1.0, -1.0 + 0.4 / 127.5, -1.0 + 0.6 / 127.5, 0.0, 1 / 255, 1.0 - 1e-7, 1.0 + 1e-6, -1.0 - 1e-6])
    want = torch.round((x + 1.0) * 127.5).clamp(0, 255) / 127.5 - 1.0
    assert torch.equal(D.snap_8bit(x), want)
    assert D.snap_8bit(x).tolist()[:3] == [-1.0, -1.0, float(np.float32(1 / 127.5) - np.float32(1.0))]
    assert float(D.snap_8bit(torch.tensor([1 / 255]))) == float(torch.tensor(128.0) / 127.5 - 1)   # 127.5 -> 128: half to even


# ---- calc_bpd's argument checks: all before any device work --------------------------------------------------------------
def test_calc_bpd_rejects_bad_requests_before_touching_a_device():
    d = _diff(21)
    m = _model(1)
    x = torch.zeros(2, 1, 32, 32)
    with pytest.raises(ValueError, match="do not match"):
        d.calc_bpd(m, torch.zeros(2, 3, 32, 32))                          # channels
    with pytest.raises(ValueError, match="do not match"):
        d.calc_bpd(m, torch.zeros(2, 1, 16, 16))                          # size
    with pytest.raises(ValueError, match=r"\(n, C, H, W\)"):
        d.calc_bpd(m, torch.zeros(1, 32, 32))
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        d.calc_bpd(m, x + 1.01)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        d.calc_bpd(m, x - 1.5)
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        d.calc_bpd(m, x.clone().fill_(float("nan")))
    with pytest.raises(ValueError, match="unknown sigma"):
        d.calc_bpd(m, x, sigma="learned")
    for K in (0, 21, -3, 2.5, True):
        with pytest.raises(ValueError, match="t_samples"):
            d.calc_bpd(m, x, t_samples=K)
    with pytest.raises(ValueError, match="noise_steps >= 3"):
        _diff(2).calc_bpd(m, x)
    with pytest.raises(ValueError, match="batch"):
        d.calc_bpd(m, x, batch=0)
    with pytest.raises(ValueError, match="noise_source"):
        d.calc_bpd(m, x, noise_source="reference")
    with pytest.raises(ValueError, match="label embedding"):
        d.calc_bpd(m, x, labels=[1, 2])
    with pytest.raises(ValueError, match="unknown sigma"):
        d.vlb_coefficients("fixedlarge")
    assert m.training and m._t_range is None


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_bpd_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_noise_images_gather"] == (ctypes.c_int, [P, L, P, P, P, P, P, L, L, P])
    assert sigs["afd_vlb_terms"] == (ctypes.c_int, [P, L, P, P, P, P, P, P, L, P, P, P, P, P, L, L, P])
    assert sigs["afd_vlb_prior"] == (ctypes.c_int, [P, DBL, P, L, L, P])


def test_bpd_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_double * 4096)()
    base = ctypes.addressof(buf)
    at = lambda i: base + 8 * i                                          # 8-byte slots
    # gathered noising: 2 images of 8 floats (4 slots each), 3 rows
    x0, img, eps, t, ah, xt = at(0), at(100), at(200), at(300), at(400), at(500)
    args = [x0, 2, img, eps, t, ah, xt, 3, 8, None]
    for i in (0, 2, 3, 4, 5, 6):
        bad = list(args)
        bad[i] = None
        with pytest.raises(afdm.AfdError, match="afd_noise_images_gather: .*NULL"):
            lib.afd_noise_images_gather(*bad)
    for i, v in ((1, 0), (7, 0), (7, -1), (8, 0)):
        bad = list(args)
        bad[i] = v
        with pytest.raises(afdm.AfdError, match="afd_noise_images_gather: .*positive"):
            lib.afd_noise_images_gather(*bad)
    for o in (at(0), at(7), at(199), at(210), at(100), at(300)):         # x_t over x0, eps, img, t
        bad = list(args)
        bad[6] = o
        with pytest.raises(afdm.AfdError, match="afd_noise_images_gather: x_t must not overlap"):
            lib.afd_noise_images_gather(*bad)
    # bound terms: T = 5 (coef 20 doubles), 3 rows of 8 floats
    xt2, e, eh, coef, a, b, term, sq = at(600), at(700), at(800), at(900), at(1000), at(1100), at(1200), at(1300)
    args = [x0, 2, img, xt2, e, eh, t, coef, 5, a, ah, b, term, sq, 3, 8, None]
    for i in (0, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13):
        bad = list(args)
        bad[i] = None
        with pytest.raises(afdm.AfdError, match="afd_vlb_terms: no pointer may be NULL"):
            lib.afd_vlb_terms(*bad)
    for i, v in ((1, 0), (14, 0), (15, -8), (8, 1)):
        bad = list(args)
        bad[i] = v
        with pytest.raises(afdm.AfdError, match="afd_vlb_terms: .*positive"):
            lib.afd_vlb_terms(*bad)
    for i in (12, 13):
        for o in (x0, at(7), img, xt2, e, eh, t, at(919), a, ah, b, term if i == 13 else sq, at(1202) if i == 13 else at(1302)):
            bad = list(args)
            bad[i] = o
            with pytest.raises(afdm.AfdError, match="afd_vlb_terms: term and sq must not overlap"):
                lib.afd_vlb_terms(*bad)
    # prior
    with pytest.raises(afdm.AfdError, match="afd_vlb_prior: .*NULL"):
        lib.afd_vlb_prior(None, 0.5, at(10), 2, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_vlb_prior: .*NULL"):
        lib.afd_vlb_prior(x0, 0.5, None, 2, 8, None)
    for n, per in ((0, 8), (2, 0), (-1, 8)):
        with pytest.raises(afdm.AfdError, match="afd_vlb_prior: .*positive"):
            lib.afd_vlb_prior(x0, 0.5, at(10), n, per, None)
    for o in (x0, at(7)):
        with pytest.raises(afdm.AfdError, match="afd_vlb_prior: out must not overlap"):
            lib.afd_vlb_prior(x0, 0.5, o, 2, 8, None)
