"""Learned reverse-process variances, host side: the coefficient table, argument validation, untouched defaults, and the
coverage of the decoder inputs the GPU tests rely on (checked with the fp64 restatement alone)."""
import math

import numpy as np
import pytest
import torch

import lvar_oracle as O


def _diff(T=1000, **kw):
    from afdm import Diffusion
    return Diffusion(noise_steps=T, img_size=32, device="cpu", **kw)


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("T", (10, 300, 1000))
def test_lvar_coefficients_against_an_independent_restatement(T, schedule):
    d = _diff(T, schedule=schedule, variance="learned")
    tab = d.lvar_coefficients()
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (T, 3)
    b = [float(v) for v in d.beta]              # Python floats hold the fp32 values exactly
    a = [float(v) for v in d.alpha]
    ah = [float(v) for v in d.alpha_hat]
    want = np.zeros((T, 3))
    for t in range(1, T):
        bt = (1.0 - ah[t - 1]) / (1.0 - ah[t]) * b[t]
        want[t] = [math.log(b[t]), math.log(bt), b[t] ** 2 / (a[t] * (1.0 - ah[t]))]
    got = tab.numpy()
    assert np.all(got[0] == 0.0)
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    assert np.allclose(got, O.tables64(d.beta, d.alpha, d.alpha_hat).numpy(), rtol=1e-14, atol=0)
    assert np.all(np.isfinite(got))                                  # the cosine schedule's last rows (beta = 0.999) included
    assert np.all(got[1:, 1] < got[1:, 0])                           # log beta~_t < log beta_t for every t >= 1
    assert np.all(got[1:, 2] > 0)


def test_defaults_are_untouched():
    from afdm import Diffusion
    base = _diff()
    assert base.variance == "fixed" and base.output_channels(3) == 3
    lin = torch.linspace(1e-4, 0.02, 1000)
    assert torch.equal(base.beta, lin) and torch.equal(base.alpha, 1.0 - lin)
    assert torch.equal(base.alpha_hat, torch.cumprod(1.0 - lin, dim=0))
    for kw in (dict(), dict(schedule="cosine", prediction="v")):
        d0, d1 = _diff(**kw), _diff(variance="learned", **kw)
        for name in ("beta", "alpha", "alpha_hat"):
            assert torch.equal(getattr(d0, name), getattr(d1, name))
        assert torch.equal(d0.vlb_coefficients(), d1.vlb_coefficients())
        assert torch.equal(d0.snr_weights(), d1.snr_weights())
    assert d1.variance == "learned" and d1.output_channels(3) == 6
    assert Diffusion.VARIANCES == ("fixed", "learned")


def test_argument_validation():
    from afdm import Diffusion, TrainStep, UNet, argument
    from afdm.training import diffusion_kwargs, model_out_channels
    for bad in ("Learned", "", None, 1, True):
        with pytest.raises(ValueError, match="unknown variance"):
            Diffusion(noise_steps=10, device="cpu", variance=bad)
    with pytest.raises(ValueError, match="noise_steps >= 2"):
        _diff(1, variance="learned").lvar_coefficients()
    fs = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
    narrow = UNet(c_in=3, c_out=3, image_size=32, f_settings=fs, device="cpu", variant=3)
    wide = UNet(c_in=3, c_out=6, image_size=32, f_settings=fs, device="cpu", variant=3)
    learned, fixed = _diff(21, variance="learned"), _diff(21)
    learned.check_model(wide, 3)
    fixed.check_model(narrow, 3)
    with pytest.raises(ValueError, match=r"emits 3 channels .* needs 6"):
        learned.check_model(narrow, 3)
    with pytest.raises(ValueError, match=r"emits 6 channels .* needs 3"):
        fixed.check_model(wide)
    with pytest.raises(ValueError, match=r"emits 3 channels .* needs 6"):
        learned.sample(narrow, n=1, image_channels=3)
    with pytest.raises(ValueError, match=r"emits 6 channels .* needs 3"):
        fixed.sample(wide, n=1, image_channels=3)
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(ValueError, match=r"emits 3 channels .* needs 6"):
        learned.calc_bpd(narrow, x, sigma="learned")
    with pytest.raises(ValueError, match="unknown sigma"):
        fixed.calc_bpd(narrow, x, sigma="learned")
    with pytest.raises(ValueError, match="unknown sigma"):
        learned.calc_bpd(wide, x, sigma="nope")
    # the run settings
    a = argument(image_channels=3, variance="learned", vlb_lambda=0.01)
    assert diffusion_kwargs(a) == {"variance": "learned"} and model_out_channels(a) == 6
    assert diffusion_kwargs(argument()) == {} and model_out_channels(argument(image_channels=1)) == 1
    for bad in (-1.0, float("nan"), float("inf"), True, "0.1", None):
        with pytest.raises(ValueError, match="vlb_lambda"):
            TrainStep(wide, learned, lr=1e-3, vlb_lambda=bad)


def test_decoder_inputs_cover_edge_bins_and_the_clamp():
    """What tests/test_gpu_lvar.py's decoder test relies on, from the fp64 restatement alone: each edge bin is used, more than
    100 elements hit the 1e-12 clamp and more than 100 do not, and dv is exactly 0 on the clamped ones."""
    d = _diff()
    for rows, chw in ((5, 255), (8, 3072)):
        out2, x0, eps, t = O.decoder_case(rows, chw, 11)
        r = O.hybrid(d.beta, d.alpha, d.alpha_hat, "eps", out2, x0, eps, t, None, 0.999)
        lo, hi = x0 < -0.999, x0 > 0.999
        assert int(lo.sum()) > 0 and int(hi.sum()) > 0
        assert int(r["clamped"].sum()) > 100 and int((~r["clamped"]).sum()) > 100
        assert int((r["clamped"] & lo).sum()) > 0 and int((r["clamped"] & hi).sum()) > 0 and int((r["clamped"] & ~lo & ~hi).sum()) > 0
        assert bool((r["dv"][r["clamped"]] == 0).all()) and bool((r["dv"][~r["clamped"]] != 0).any())
        assert bool(torch.isfinite(r["dv"]).all()) and bool(torch.isfinite(r["L"]))


@pytest.mark.parametrize("kind", ("eps", "v", "x0"))
def test_oracle_d_form_is_the_kl_between_the_two_gaussians(kind):
    """The restatement the GPU tests are gated on against the textbook KL (difference of the posterior means) where that form is
    well conditioned (t >= 100): 1e-6 relative per row, on the tables widened to fp64."""
    d = _diff()
    out2, x0, eps, t = O.case(6, 96, 1000, 3, (d.beta, d.alpha, d.alpha_hat), kind)
    t = torch.tensor([100, 250, 500, 750, 900, 999])
    r = O.hybrid(d.beta, d.alpha, d.alpha_hat, kind, out2, x0, eps, t)
    b, a, ah = (v.double() for v in (d.beta, d.alpha, d.alpha_hat))
    bt, at, aht, ahp = b[t][:, None], a[t][:, None], ah[t][:, None], ah[t - 1][:, None]
    p, v = out2[:, :96].double(), out2[:, 96:].double()
    xt = torch.sqrt(aht) * x0.double() + torch.sqrt(1 - aht) * eps.double()
    eh = {"eps": p, "v": torch.sqrt(aht) * p + torch.sqrt(1 - aht) * xt, "x0": (xt - torch.sqrt(aht) * p) / torch.sqrt(1 - aht)}[kind]
    x0h = (xt - torch.sqrt(1 - aht) * eh) / torch.sqrt(aht)
    c0, c1 = torch.sqrt(ahp) * bt / (1 - aht), torch.sqrt(at) * (1 - ahp) / (1 - aht)
    mq, mp = c0 * x0.double() + c1 * xt, c0 * x0h + c1 * xt
    lvq = torch.log((1 - ahp) / (1 - aht) * bt)
    lvp = O.logvar64(v, torch.log(bt), lvq)
    kl = 0.5 * (-1.0 + lvp - lvq + torch.exp(lvq - lvp) + (mq - mp) ** 2 * torch.exp(-lvp))
    want = kl.sum(dim=1)
    assert float(((r["term"] - want).abs() / want.abs()).max()) < 1e-6
