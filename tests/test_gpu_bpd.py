"""GPU tests of the bits/dim likelihood: gathered noising bit for bit against noise_images, the bound-terms kernel against an
fp64 restatement (and run twice for identical bits), the argument checks, a model that predicts the noise exactly, the closed
form of the bound's KL part on Gaussian data, the whole bound against the CPU oracle, sampled timesteps, the conditional
UNet, the model state after an exception, and ddpm_run's eval_bpd."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import note

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42, num_classes=None, c=3):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=c, c_out=c, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


def _grid_images(g, n, c=3, size=32):
    """8-bit images with both edge levels and interior levels."""
    k = torch.randint(0, 256, (n, c, size, size), generator=g)
    k.view(-1)[::7] = 0
    k.view(-1)[3::11] = 255
    return k.float() / 127.5 - 1.0


# ---- fp64 restatements -------------------------------------------------------------------------------------------------------
def _f32(v):
    return np.float32(v)


def _noised_f32(x0, eps, ah_t):
    """noise_images' expression in numpy fp32, one rounding per operation (x0, eps: fp32 arrays; ah_t: fp32 per row)."""
    sa = np.sqrt(ah_t.astype(np.float32)).reshape(-1, 1)
    sb = np.sqrt(np.float32(1) - ah_t.astype(np.float32)).reshape(-1, 1)
    return (sa * x0) + (sb * eps)


def _decoder_mean_f32(diff, xt, eh):
    """denoise_step's fp32 expression at i = 1 without noise: c1 * (x - c2 * eps_hat)."""
    a, ah = _f32(diff.alpha[1].item()), _f32(diff.alpha_hat[1].item())
    c1 = np.float32(1) / np.sqrt(a)
    c2 = (np.float32(1) - a) / np.sqrt(np.float32(1) - ah)
    return c1 * (xt - c2 * eh)


def _decoder_nll64(x0, mean, log_scale, dev):
    """-sum log P(x0 | mean, exp(log_scale)), Ho et al.'s discretised Gaussian, per row, in fp64 -> (nll, log P) as numpy.
    Evaluated with torch's fp64 operations on the device, one per operation in the kernel's order: 1 + tanh cancels in the
    tails, where one ulp of a different host tanh would move log P by more than the gate."""
    x = torch.as_tensor(x0).to(dev).double()
    c = x - torch.as_tensor(mean).to(dev).double()
    inv = torch.exp(torch.tensor(-log_scale, dtype=torch.float64, device=dev))

    def cdf(v):
        cube = (v * v) * v
        return 0.5 * (1.0 + torch.tanh(0.7978845608028654 * (v + 0.044715 * cube)))

    cp, cm = cdf(inv * (c + 1.0 / 255.0)), cdf(inv * (c - 1.0 / 255.0))
    lp = torch.where(x < -0.999, torch.log(torch.clamp(cp, min=1e-12)),
                     torch.where(x > 0.999, torch.log(torch.clamp(1.0 - cm, min=1e-12)), torch.log(torch.clamp(cp - cm, min=1e-12))))
    lp = lp.cpu().numpy()
    return -lp.sum(axis=-1), lp


def _terms64(diff, coef, x0_rows, xt, eps, eh, t, dev):
    """(term, sq) per row in fp64 from the definitions (numpy arrays of shape (rows, D))."""
    d = eh.astype(np.float64) - eps.astype(np.float64)
    sq = (d * d).sum(axis=1)
    D = eps.shape[1]
    term = coef[t, 0] * sq + D * coef[t, 1]
    dec = t == 1
    if dec.any():
        term[dec] = _decoder_nll64(x0_rows[dec], _decoder_mean_f32(diff, xt[dec], eh[dec]), float(coef[1, 2]), dev)[0]
    return term, sq


# ---- 1. gathered noising ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["vec", "odd", "offset"])
def test_gathered_noising_is_noise_images_bit_for_bit(A, layout):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    g = torch.Generator().manual_seed(["vec", "odd", "offset"].index(layout))
    shape = (3, 5, 7) if layout == "odd" else (3, 32, 32)
    off = 1 if layout == "offset" else 0                            # every float operand 4 bytes past a 16-byte boundary
    n_img, rows = 5, 37

    def buf(*s):
        c = int(np.prod(s))
        return torch.randn(c + off, generator=g).to(dev)[off:].view(*s)

    x0 = buf(n_img, *shape)
    eps = buf(rows, *shape)
    img = torch.randint(0, n_img, (rows,), generator=g).to(dev)
    t = torch.randint(1, 1000, (rows,), generator=g).to(dev)
    t[:3] = torch.tensor([1, 999, 500])
    got = ops.noise_images_gather(x0, img, eps, t, diff.alpha_hat, out=buf(rows, *shape))
    want = ops.noise_images(x0[img], eps, t, diff.alpha_hat)
    assert _same_bits(got, want)
    with pytest.raises(afdm.AfdError, match="img must lie"):
        ops.noise_images_gather(x0, img + n_img, eps, t, diff.alpha_hat)
    with pytest.raises(afdm.AfdError, match="t must lie"):
        ops.noise_images_gather(x0, img, eps, t * 0, diff.alpha_hat)


# ---- 2. the terms kernel against fp64 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", ["beta", "posterior"])
@pytest.mark.parametrize("layout", ["vec", "odd"])
def test_terms_kernel_against_fp64(A, sigma, layout):
    afdm, dev = A
    from afdm import ops
    T = 1000
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    coef = diff.vlb_coefficients(sigma)
    coef_d = coef.to(dev)
    g = torch.Generator().manual_seed(7 + (layout == "odd"))
    shape = (3, 5, 7) if layout == "odd" else (3, 32, 32)
    D = int(np.prod(shape))
    n_img, rows = 4, 24
    k = torch.randint(0, 256, (n_img, D), generator=g)
    k[:, ::5] = 0
    k[:, 1::9] = 255
    x0 = (k.float() / 127.5 - 1.0).view(n_img, *shape)
    img = torch.randint(0, n_img, (rows,), generator=g)
    t = torch.randint(2, T, (rows,), generator=g)
    t[::3] = 1                                                      # 8 decoder rows among 16 KL rows
    t[1] = 2
    t[2] = T - 1
    eps = torch.randn(rows, D, generator=g)
    ah = diff.alpha_hat.cpu().numpy()
    xt = _noised_f32(x0.view(n_img, D).numpy()[img.numpy()], eps.numpy(), ah[t.numpy()])
    # eps_hat: eps plus an error whose scale varies per element, so the decoder means fall inside bins, a few sigma off, and
    # far enough off that the 1e-12 clamp is hit (and in both edge bins)
    scale = torch.tensor([0.0, 0.05, 0.5, 2.0, 8.0, 40.0, 400.0])[torch.randint(0, 7, (rows, D), generator=g)]
    eh = eps + scale * torch.randn(rows, D, generator=g)
    xd, xtd = x0.to(dev), torch.from_numpy(xt).view(rows, *shape).to(dev)
    ed, ehd = eps.view(rows, *shape).to(dev), eh.view(rows, *shape).to(dev)
    id_, td = img.to(dev), t.to(dev)
    args = (xd, id_, xtd, ed, ehd, td, coef_d, diff.alpha, diff.alpha_hat, diff.beta)
    term, sq = ops.vlb_terms(*args)
    term2, sq2 = ops.vlb_terms(*args)
    assert _same_bits(term, term2) and _same_bits(sq, sq2)          # deterministic
    want, want_sq = _terms64(diff, coef.numpy(), x0.view(n_img, D).numpy()[img.numpy()], xt, eps.numpy(), eh.numpy(), t.numpy(),
                             dev)
    got, got_sq = term.cpu().numpy(), sq.cpu().numpy()
    dec = t.numpy() == 1
    rel = np.abs(got - want) / np.abs(want)
    rel_sq = np.abs(got_sq - want_sq) / np.abs(want_sq)
    kl_worst, dec_worst = float(rel[~dec].max()), float(rel[dec].max())
    note("bpd: KL rows vs fp64 (relative, per row)", kl_worst, (sigma, layout))
    note("bpd: decoder rows vs fp64 (relative, per row)", dec_worst, (sigma, layout))
    print(f"terms vs fp64 ({sigma}, {layout}): KL worst {kl_worst:.2e}, decoder worst {dec_worst:.2e}, sq worst {rel_sq.max():.2e}")
    assert kl_worst < 1e-12 and float(rel_sq.max()) < 1e-12
    assert dec_worst < 1e-10
    # the decoder rows cover both edge bins, interior bins and the clamp
    _, lp = _decoder_nll64(x0.view(n_img, D).numpy()[img.numpy()][dec],
                           _decoder_mean_f32(diff, xt[dec], eh.numpy()[dec]), float(coef[1, 2]), dev)
    assert (lp == math.log(1e-12)).sum() > 100 and (lp > -2.0).sum() > 100


def test_prior_kernel_against_fp64(A):
    afdm, dev = A
    from afdm import ops
    g = torch.Generator().manual_seed(3)
    for shape in ((6, 3, 32, 32), (5, 3, 5, 7)):
        x0 = _grid_images(g, shape[0], shape[1], 32)[:, :, :shape[2], :shape[3]].contiguous()
        got = ops.vlb_prior(x0.to(dev), 0.5 * 4.03e-5).cpu()
        want = 0.5 * 4.03e-5 * (x0.double() ** 2).flatten(1).sum(1)
        assert torch.allclose(got, want, rtol=1e-13, atol=0)


def test_bpd_kernels_reject_overlaps_and_write_nothing(A):
    afdm, dev = A
    lib = afdm.lib()
    p = lambda v: v.data_ptr()
    x0 = torch.zeros(2, 8, device=dev)
    eps = torch.zeros(3, 8, device=dev)
    img = torch.zeros(3, dtype=torch.long, device=dev)
    t = torch.ones(3, dtype=torch.long, device=dev)
    diff = afdm.Diffusion(noise_steps=5, img_size=32, device=dev)
    coef = diff.vlb_coefficients().to(dev)
    out = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    with pytest.raises(afdm.AfdError, match="term and sq must not overlap"):
        lib.afd_vlb_terms(p(x0), 2, p(img), p(eps), p(eps), p(eps), p(t), p(coef), 5, p(diff.alpha), p(diff.alpha_hat),
                          p(diff.beta), p(out), out.data_ptr() + 16, 3, 8, None)
    with pytest.raises(afdm.AfdError, match="term and sq must not overlap"):
        lib.afd_vlb_terms(p(x0), 2, p(img), p(eps), p(eps), p(eps), p(t), p(coef), 5, p(diff.alpha), p(diff.alpha_hat),
                          p(diff.beta), p(coef), p(out), 3, 8, None)
    with pytest.raises(afdm.AfdError, match="positive"):
        lib.afd_vlb_terms(p(x0), 2, p(img), p(eps), p(eps), p(eps), p(t), p(coef), 5, p(diff.alpha), p(diff.alpha_hat),
                          p(diff.beta), p(out), out.data_ptr() + 256, 0, 8, None)
    xt = torch.full((3, 8), float("nan"), device=dev)
    with pytest.raises(afdm.AfdError, match="x_t must not overlap"):
        lib.afd_noise_images_gather(p(x0), 2, p(img), p(eps), p(t), p(diff.alpha_hat), p(eps), 3, 8, None)
    with pytest.raises(afdm.AfdError, match="NULL"):
        lib.afd_noise_images_gather(p(x0), 2, None, p(eps), p(t), p(diff.alpha_hat), p(xt), 3, 8, None)
    with pytest.raises(afdm.AfdError, match="out must not overlap"):
        lib.afd_vlb_prior(p(x0), 0.5, p(x0), 2, 8, None)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(xt).all())
    assert bool((coef.cpu() == diff.vlb_coefficients()).all()) and bool((eps == 0).all()) and bool((x0 == 0).all())


# ---- 3. a model that predicts the noise exactly ---------------------------------------------------------------------------------
class _Recorder:
    def __init__(self, dev, gen=None):
        self.chunks, self.dev, self.gen = [], dev, gen

    def __call__(self, shape):
        z = torch.randn(shape, generator=self.gen).to(self.dev) if self.gen is not None else torch.randn(shape, device=self.dev)
        self.chunks.append(z)
        return z


class _Cheat(torch.nn.Module):
    """Returns the noise of the chunk being scored."""

    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def forward(self, x, t):
        return self.rec.chunks[-1]


def test_exact_noise_model_has_zero_kl_terms(A):
    afdm, dev = A
    T, n = 21, 3
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    g = torch.Generator().manual_seed(5)
    x0 = _grid_images(g, n)
    rec = _Recorder(dev)
    r = diff.calc_bpd(_Cheat(rec), x0, sigma="posterior", batch=7, noise_fn=rec, return_terms=True)
    assert [c.shape[0] for c in rec.chunks] == [7] * 8 + [4]
    assert torch.all(r["terms"][:, 2:] == 0.0) and torch.all(r["vb_bpd"] == 0.0)
    assert torch.all(r["mse"][:, 1:] == 0.0)
    coef = diff.vlb_coefficients("posterior").numpy()
    D = 3 * 32 * 32
    eps = torch.cat(rec.chunks).cpu().view(n * (T - 1), D).numpy()
    ah = diff.alpha_hat.cpu().numpy()
    xf = x0.view(n, D).numpy()
    rows = [i * (T - 1) + (T - 2) for i in range(n)]                 # t = 1 is each image's last row
    xt = _noised_f32(xf, eps[rows], np.full(n, ah[1], dtype=np.float32))
    dec, _ = _decoder_nll64(xf, _decoder_mean_f32(diff, xt, eps[rows]), float(coef[1, 2]), dev)
    prior = D * coef[0, 3] + 0.5 * float(ah[T - 1]) * (xf.astype(np.float64) ** 2).sum(1)
    norm = D * math.log(2)
    got_dec, got_prior = r["decoder_bpd"].numpy() * norm, r["prior_bpd"].numpy() * norm
    e_dec = float(np.max(np.abs(got_dec - dec) / np.abs(dec)))
    e_prior = float(np.max(np.abs(got_prior - prior) / np.abs(prior)))
    note("bpd: exact-noise model, decoder vs fp64", e_dec)
    print(f"exact-noise model: decoder {dec} nats (rel err {e_dec:.2e}), prior rel err {e_prior:.2e}")
    assert e_dec < 1e-10 and e_prior < 1e-12
    assert torch.allclose(r["bpd"], r["prior_bpd"] + r["decoder_bpd"], rtol=1e-15, atol=0)


# ---- 4. the closed form of the KL part on Gaussian data ---------------------------------------------------------------------
class _GaussEps(torch.nn.Module):
    """The exact eps of x0 ~ N(mu, s^2 I): eps(x, t) = sqrt(1 - a)(x - sqrt(a) mu) / (s^2 a + 1 - a), a = alpha_hat[t], in
    fp64 and rounded to fp32 (test_gpu_dpm.py's model with s a parameter)."""

    def __init__(self, mu, alpha_hat, s):
        super().__init__()
        self.mu, self.ah, self.s2 = mu, alpha_hat.double(), s * s

    def forward(self, x, t):
        a = self.ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (self.s2 * a + 1 - a)).float()


# s = 0.2 keeps x0 inside [-1, 1] (|z| > 4 is needed to leave it); the bound rejects images outside, and clipping would make
# the data non-Gaussian.  With s = 0.5 about a tenth of the pixels would leave the range.
S_DATA = 0.2


def _gauss_data(dev, n, seed):
    g = torch.Generator().manual_seed(seed)
    mu = (torch.rand(1, 3, 32, 32, generator=g, dtype=torch.float64) * 0.4 - 0.2)
    x0 = (mu + S_DATA * torch.randn(n, 3, 32, 32, generator=g, dtype=torch.float64)).clamp(-1, 1).float()
    return mu.to(dev), x0


def test_kl_part_matches_the_closed_form_on_gaussian_data(A):
    afdm, dev = A
    T, n = 1000, 16
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    mu, x0 = _gauss_data(dev, n, 0)
    model = _GaussEps(mu, diff.alpha_hat, S_DATA)
    afdm.set_seed(1)
    r = diff.calc_bpd(model, x0, batch=512, return_terms=True)
    coef = diff.vlb_coefficients().numpy()
    ah = diff.alpha_hat.cpu().double().numpy()
    D = 3 * 32 * 32
    t = np.arange(2, T)
    a, w, s2 = ah[t], coef[t, 0], S_DATA ** 2
    v = a * s2 / (a * s2 + 1 - a)                                   # E[(eps_hat - eps)^2] per element
    want = float(np.sum(w * D * v + D * coef[t, 1]))
    # eps_hat - eps = k sqrt(a) (x0 - mu) + (k sqrt(1 - a) - 1) eps, k = sqrt(1 - a) / (a s2 + 1 - a).  Every row of an image
    # shares its x0, so the variance per image has an x0 part common to all t (chi^2_D of (x0 - mu)^2 / s2) besides the
    # independent eps part of each row (a non-central chi^2_D given x0).
    k = np.sqrt(1 - a) / (a * s2 + 1 - a)
    c, e2 = k * k * a, (k * np.sqrt(1 - a) - 1) ** 2
    var = 2 * D * s2 ** 2 * float(np.sum(w * c)) ** 2 + D * float(np.sum(w * w * (2 * e2 ** 2 + 4 * c * s2 * e2)))
    sd = math.sqrt(var / n)
    got = float(r["vb_bpd"].mean()) * D * math.log(2)
    z = (got - want) / sd
    note("bpd: Gaussian data, KL part vs closed form (in standard deviations)", abs(z))
    mse_ratio = float((r["mse"][:, 2:].mean(0).numpy() / v).mean())
    print(f"Gaussian data: KL part {got:.3f} nats vs closed form {want:.3f} (sd {sd:.3f}, z = {z:+.2f}); "
          f"mean mse / v = {mse_ratio:.5f}; bpd {float(r['bpd'].mean()):.4f}")
    assert abs(z) < 3


# ---- 5. the whole bound against the CPU oracle ---------------------------------------------------------------------------------
def test_bound_against_the_cpu_oracle(A):
    afdm, dev = A
    from oracle import ref_ops as R
    T, n, batch = 21, 2, 16
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    g = torch.Generator().manual_seed(9)
    x0 = _grid_images(g, n)
    afdm.set_seed(21)
    r = diff.calc_bpd(model, x0, noise_source="cpu", batch=batch, return_terms=True)
    afdm.set_seed(21)
    img, t = diff.bpd_rows(diff.bpd_timesteps(n))
    eps = torch.cat([torch.randn((hi - lo, 3, 32, 32)) for lo, hi in diff.bpd_chunks(len(t), batch)])
    D = 3 * 32 * 32
    ah = diff.alpha_hat.cpu().numpy()
    xf = x0.view(n, D).numpy()
    xt = _noised_f32(xf[img], eps.view(-1, D).numpy(), ah[t])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        eh = R.unet_forward(sd, torch.from_numpy(xt).view(-1, 3, 32, 32), torch.from_numpy(t), 3, F_SET).double()
    coef = diff.vlb_coefficients().numpy()
    e64 = eps.view(-1, D).double().numpy()
    d = eh.reshape(-1, D).numpy() - e64
    term = coef[t, 0] * (d * d).sum(1) + D * coef[t, 1]
    dec = t == 1
    a1, ah1 = float(diff.alpha[1]), float(ah[1])
    mean = (xt[dec].astype(np.float64) - (1 - a1) / math.sqrt(1 - ah1) * eh.reshape(-1, D).numpy()[dec]) / math.sqrt(a1)
    term[dec] = _decoder_nll64(xf[img[dec]], mean, float(coef[1, 2]), dev)[0]
    norm = D * math.log(2)
    want = {"vb_bpd": np.bincount(img[~dec], term[~dec], n) / norm, "decoder_bpd": np.bincount(img[dec], term[dec], n) / norm,
            "prior_bpd": (D * coef[0, 3] + 0.5 * float(ah[T - 1]) * (xf.astype(np.float64) ** 2).sum(1)) / norm}
    want["bpd"] = want["vb_bpd"] + want["decoder_bpd"] + want["prior_bpd"]
    worst = 0.0
    for k, w in want.items():
        e = float(np.max(np.abs(r[k].numpy() - w) / np.abs(w)))
        note(f"bpd: T = 21 bound vs CPU oracle: {k}", e)
        worst = max(worst, e)
        assert e < 1e-5, (k, r[k], w)
    print(f"bound vs CPU oracle (T = 21): bpd {r['bpd'].tolist()}, worst part rel err {worst:.2e}")


# ---- 6. sampled timesteps ---------------------------------------------------------------------------------------------------
def test_sampled_timesteps_rows_and_estimate(A):
    afdm, dev = A
    from afdm import ops
    T, n, K, batch = 101, 64, 10, 256
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    mu, x0 = _gauss_data(dev, n, 1)
    model = _GaussEps(mu, diff.alpha_hat, S_DATA)
    afdm.set_seed(3)
    rec = _Recorder(dev)
    r = diff.calc_bpd(model, x0, t_samples=K, batch=batch, noise_fn=rec, return_terms=True)
    afdm.set_seed(3)
    ts = diff.bpd_timesteps(n, K)                                    # the same draws: nothing is drawn before them
    img, t = diff.bpd_rows(ts)
    assert all(len(set(row)) == K for row in ts)
    evaluated = r["mse"].numpy() > 0
    assert evaluated.sum() == n * K and all(evaluated[i, row].all() for i, row in enumerate(ts))
    # replay each chunk with the recorded noise through the kernels: the same terms, bit for bit
    snapped = diff.snap_8bit(x0).to(dev)
    coef = diff.vlb_coefficients().to(dev)
    img_d, t_d = torch.from_numpy(img).to(dev), torch.from_numpy(t).to(dev)
    terms = []
    with torch.no_grad():
        for (lo, hi), eps in zip(diff.bpd_chunks(len(t), batch), rec.chunks):
            xt = ops.noise_images_gather(snapped, img_d[lo:hi], eps, t_d[lo:hi], diff.alpha_hat)
            terms.append(ops.vlb_terms(snapped, img_d[lo:hi], xt, eps, model(xt, t_d[lo:hi]), t_d[lo:hi], coef, diff.alpha,
                                       diff.alpha_hat, diff.beta)[0])
    terms = torch.cat(terms).cpu()
    assert _same_bits(r["terms"][torch.from_numpy(img), torch.from_numpy(t)], terms)
    est = r["prior_bpd"] + (T - 1) / K * r["terms"].sum(1) / (3 * 32 * 32 * math.log(2))
    assert torch.allclose(r["bpd"], est, rtol=1e-13, atol=0)
    full = diff.calc_bpd(model, x0, batch=batch)["bpd"]
    se = float(r["bpd"].std()) / math.sqrt(n)
    z = (float(r["bpd"].mean()) - float(full.mean())) / se
    note("bpd: K = 10 estimate vs the full bound (in standard errors)", abs(z))
    print(f"sampled timesteps: K = 10 mean {float(r['bpd'].mean()):.4f} bpd, full bound {float(full.mean()):.4f}, "
          f"se {se:.4f}, z = {z:+.2f}")
    assert abs(z) < 3


# ---- 7. the conditional UNet -------------------------------------------------------------------------------------------------
def test_conditional_bound_equals_a_hand_loop(A):
    afdm, dev = A
    from afdm import ops
    T, n, batch = 11, 3, 8
    model = _model(afdm, dev, num_classes=10)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    x0 = _grid_images(torch.Generator().manual_seed(4), n)
    labels = torch.tensor([3, afdm.NULL_LABEL, 7])
    afdm.set_seed(8)
    r = diff.calc_bpd(model, x0, labels=labels, batch=batch, return_terms=True)
    afdm.set_seed(8)
    img, t = diff.bpd_rows(diff.bpd_timesteps(n))
    snapped = diff.snap_8bit(x0).to(dev)
    coef = diff.vlb_coefficients().to(dev)
    img_d, t_d = torch.from_numpy(img).to(dev), torch.from_numpy(t).to(dev)
    y = labels.to(dev)[img_d]
    term, sq = [], []
    model.eval()
    with torch.no_grad():
        for lo, hi in diff.bpd_chunks(len(t), batch):
            eps = torch.randn((hi - lo, 3, 32, 32), device=dev)
            xt = ops.noise_images_gather(snapped, img_d[lo:hi], eps, t_d[lo:hi], diff.alpha_hat)
            a, b = ops.vlb_terms(snapped, img_d[lo:hi], xt, eps, model(xt, t_d[lo:hi], y[lo:hi]), t_d[lo:hi], coef, diff.alpha,
                                 diff.alpha_hat, diff.beta)
            term.append(a)
            sq.append(b)
    model.train()
    prior = ops.vlb_prior(snapped, 0.5 * float(diff.alpha_hat[T - 1])).cpu().numpy() + 3072 * float(coef[0, 3])
    want = diff.bpd_combine(n, 3072, img, t, torch.cat(term).cpu().numpy(), torch.cat(sq).cpu().numpy(), prior, T - 1, True)
    for k in want:
        assert _same_bits(r[k], want[k]), k
    # NULL_LABEL rows are the unconditional bound
    afdm.set_seed(8)
    nul = diff.calc_bpd(model, x0, labels=[afdm.NULL_LABEL] * n, batch=batch)
    afdm.set_seed(8)
    unc = diff.calc_bpd(model, x0, batch=batch)
    assert torch.allclose(nul["bpd"], unc["bpd"], rtol=1e-12, atol=0)
    assert torch.allclose(nul["bpd"][1], r["bpd"][1], rtol=1e-12, atol=0)
    assert model.training and model._t_range is None


# ---- 8. model state after an exception -------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_model_state_is_restored_after_an_exception(A, training):
    afdm, dev = A

    class Boom(afdm.UNet):
        calls = 0

        def forward(self, *a, **kw):
            Boom.calls += 1
            if Boom.calls == 2:
                raise RuntimeError("boom in the second chunk")
            return super().forward(*a, **kw)

    afdm.set_seed(42)
    model = Boom(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    model.train(training)
    diff = afdm.Diffusion(noise_steps=21, img_size=32, device=dev)
    x0 = _grid_images(torch.Generator().manual_seed(1), 2)
    with pytest.raises(RuntimeError, match="second chunk"):
        diff.calc_bpd(model, x0, batch=8)
    assert Boom.calls == 2 and model.training == training and model._t_range is None


# ---- 9. ddpm_run ---------------------------------------------------------------------------------------------------------------
def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = p
    return out


def test_ddpm_run_eval_bpd(A, tmp_path, monkeypatch):
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    runs = {}
    for key in ("plain", "bpd"):
        wd = tmp_path / key
        wd.mkdir()
        csvp = wd / "mnist.csv"
        np.savetxt(csvp, arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "bpd":
            params["eval_bpd"] = 4
        runs[key] = (afdm.ddpm_run(params), _files(wd))
    out, files = runs["bpd"]
    plain_out, plain_files = runs["plain"]
    bpd_file = os.path.join("runs", "DDPM_Uncondtional_MNIST_3", "bpd_MNIST_3.txt")
    assert set(files) - set(plain_files) == {bpd_file} and set(plain_files) <= set(files)
    assert "bpd" not in plain_out and set(out) - set(plain_out) == {"bpd"}
    assert math.isfinite(out["bpd"]) and out["bpd"] > 0
    lines = dict(ln.split(": ", 1) for ln in open(files[bpd_file]).read().splitlines())
    assert set(lines) == {"bpd", "bpd_stderr", "prior_bpd", "vb_bpd", "decoder_bpd", "N", "t_samples", "sigma"}
    assert lines["N"] == "4" and lines["t_samples"] == "11" and lines["sigma"] == "beta"
    assert abs(float(lines["bpd"]) - out["bpd"]) < 1e-5 * out["bpd"]
    parts = sum(float(lines[k]) for k in ("prior_bpd", "vb_bpd", "decoder_bpd"))
    assert abs(parts - out["bpd"]) < 1e-5 * out["bpd"]
    rel = os.path.join("runs", "DDPM_Uncondtional_MNIST_3", "settings_MNIST_3.txt")
    assert open(files[rel]).read().replace(str(tmp_path / "bpd"), "") == open(plain_files[rel]).read().replace(str(tmp_path / "plain"), "")
