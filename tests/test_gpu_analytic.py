"""GPU tests of Analytic-DPM (Bao et al. 2022): the DDIM step with sigma from a table (afd_ddim_step_var[_cfg][_dev]) against torch
fp32 restatements and against afd_ddim_step, the per-row squared norms (afd_eps_sqnorm_rows[_cfg]) against fp64 sums, and the
feature end to end on Gaussian data, whose optimal variances and sample variance are known in closed form: estimation, sampling,
graph replay, the noise drawn, the model's state, other model kinds, and the likelihood bound."""
import math

import numpy as np
import pytest
import torch

from conftest import note

pytestmark = pytest.mark.gpu

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10
T = 1000
LAYOUTS = ["vec", "odd", "offset", "inplace"]
TWO_TRIPS = 2048 * 256 * 4 + 4096                       # the 16-byte form's 2048 workgroups take a second trip of the loop


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42, num_classes=None, c_out=3):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=3, c_out=c_out, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _f32(v):
    return float(np.float32(v))


def _lerp_restated(u, c, s):
    """ATen's scalar lerp, one device op per step (as in test_gpu_cfg.py)."""
    d = c - u
    if abs(s) < 0.5:
        return u + d * s
    return c - d * _f32(1 - _f32(s))


def _coef32(ah, t, tp, eta):
    """DDIM's per-step scalars in fp32, one IEEE rounding per operation (taken in fp64 and rounded once: exact for + - * / sqrt)."""
    a_t, a_p, eta = float(ah[t]), float(ah[tp]), _f32(eta)
    sq = lambda v: _f32(math.sqrt(v))
    r = _f32(_f32(1 - a_p) / _f32(1 - a_t))
    q = _f32(1 - _f32(a_t / a_p))
    var = _f32(_f32(eta * eta) * _f32(r * q))
    return {"sq1m": sq(_f32(1 - a_t)), "sqat": sq(a_t), "sqap": sq(a_p), "sigma": sq(var),
            "dir": sq(max(_f32(_f32(1 - a_p) - var), 0.0))}


def _var_restated(x, e, z, ah, sigma, t, tp, eta):
    """The update as separate fp32 device ops, each a full-tensor operand: DDIM's, with the table's sigma."""
    k = _coef32(ah, t, tp, eta)
    full = lambda v: torch.full_like(x, v)
    pe = e * full(k["sq1m"])
    x0 = (x - pe) / full(k["sqat"])
    mean = x0 * full(k["sqap"]) + e * full(k["dir"])
    nz = z * full(sigma) if z is not None else torch.zeros_like(x)
    return mean + nz


class _GaussEps(torch.nn.Module):
    """The exact eps of x0 ~ N(mu, s2 I): eps(x, t) = sqrt(1 - a)(x - sqrt(a) mu) / (s2 a + 1 - a), a = alpha_hat[t], in fp64 and
    rounded to fp32 (s2 = 0.25: the model of test_gpu_dpm.py and test_gpu_unipc.py)."""

    def __init__(self, mu, alpha_hat, s2=0.25):
        super().__init__()
        self.mu, self.ah, self.s2 = mu, alpha_hat.double(), s2

    def forward(self, x, t):
        a = self.ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (self.s2 * a + 1 - a)).float()


def _gauss_gamma(diff, s2=0.25):
    a = diff.alpha_hat.double().cpu().numpy()
    return (1.0 - a) / (s2 * a + 1.0 - a)


def _mu(dev, half_width, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 2 - 1) * half_width).to(dev)


# ---- 1. the four entry points of the step -----------------------------------------------------------------------------------------
# every layout at the small sizes; the second trip once per access form (vec: 16-byte accesses, offset: scalar ones)
STEP_CASES = [(n, layout) for n in (1, 1023, 4096) for layout in LAYOUTS] + [(TWO_TRIPS, "vec"), (TWO_TRIPS, "offset")]


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("n,layout", STEP_CASES)
def test_ddim_step_var_equals_the_restatement(A, n, layout, guided):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    ah = diff.alpha_hat
    ah_host = ah.cpu()
    g = torch.Generator().manual_seed(LAYOUTS.index(layout) * 2 + guided)
    if layout == "odd":
        n = n + 3 if n % 4 == 0 else n                                 # never a multiple of 4: the scalar form
    off = 1 if layout == "offset" else 0                               # every operand 4 bytes past a 16-byte boundary
    s = 3.0
    sig = (torch.rand(T, generator=g) * 0.9 + 0.05).to(dev)
    sig_host = sig.cpu()

    def buf(count):
        return torch.randn(count + off, generator=g).to(dev)[off:]

    cases = [(999, 888, 1.0, True), (500, 1, 0.0, True), (37, 0, 0.5, False)] if n != TWO_TRIPS else [(640, 120, 1.0, True)]
    for t, tp, eta, use_z in cases:
        x, z = buf(n), (buf(n) if use_z else None)
        if guided:
            eps = buf(2 * n)
            e = _lerp_restated(eps[n:], eps[:n], s)
        else:
            eps = e = buf(n)
        want = _var_restated(x, e, z, ah_host, float(sig_host[t]), t, tp, eta)
        for dev_form in (False, True):
            idx = (torch.tensor([t], device=dev), torch.tensor([tp], device=dev)) if dev_form else (t, tp)
            got = x.clone() if layout == "inplace" else buf(n)         # in place: x_out = x, as the sampler runs it
            src = got if layout == "inplace" else x
            out2 = buf(n).fill_(float("nan"))
            if guided:
                step = ops.ddim_step_var_cfg_dev if dev_form else ops.ddim_step_var_cfg
                step(src, eps, z, ah, sig, *idx, eta, s, got, out2)
                assert _same_bits(out2, got), (layout, t, dev_form)
            else:
                step = ops.ddim_step_var_dev if dev_form else ops.ddim_step_var
                step(src, eps, z, ah, sig, *idx, eta, got)
            assert _same_bits(got, want), (layout, n, t, tp, eta, dev_form)
    torch.cuda.synchronize()


@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_ddim_step_var_with_ddims_own_sigma_is_ddim_step(A, eta):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    ah = diff.alpha_hat
    ah_host = ah.cpu()
    g = torch.Generator().manual_seed(7)
    pairs = diff._ddim_pairs(10, eta)
    sig = torch.zeros(T)
    for t, tp in pairs:
        sig[t] = _coef32(ah_host, t, tp, eta)["sigma"]
    sig = sig.to(dev)
    for n in (1023, 4096):
        for t, tp in pairs:
            x, e = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
            z = torch.randn(n, generator=g).to(dev) if tp > 0 else None
            assert _same_bits(ops.ddim_step_var(x, e, z, ah, sig, t, tp, eta), ops.ddim_step(x, e, z, ah, t, tp, eta)), (n, t, tp)
            e2 = torch.randn(2 * n, generator=g).to(dev)
            assert _same_bits(ops.ddim_step_var_cfg(x, e2, z, ah, sig, t, tp, eta, 2.5), ops.ddim_step_cfg(x, e2, z, ah, t, tp, eta, 2.5))


def test_ddim_step_var_last_step_and_bad_arguments(A):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    ah = diff.alpha_hat
    sig = torch.full((T,), 0.75, device=dev)
    x, e = torch.randn(2, 3, 8, 8, device=dev), torch.randn(2, 3, 8, 8, device=dev)
    # the last step of a chain is handed no noise: the mean alone, whatever sig[t] holds
    got = ops.ddim_step_var(x, e, None, ah, sig, 3, 0, 1.0)
    assert _same_bits(got, _var_restated(x, e, None, ah.cpu(), 0.75, 3, 0, 1.0))
    assert _same_bits(got, ops.ddim_step(x, e, None, ah, 3, 0, 1.0))
    z = torch.randn_like(x)
    with pytest.raises(afdm.AfdError, match="sig must be a contiguous table"):
        ops.ddim_step_var(x, e, z, ah, sig[:10], 5, 3, 1.0)
    with pytest.raises(afdm.AfdError, match="fp32"):
        ops.ddim_step_var(x, e, z, ah, sig.double(), 5, 3, 1.0)
    with pytest.raises(afdm.AfdError, match="HIP device"):
        ops.ddim_step_var(x, e, z, ah, sig.cpu(), 5, 3, 1.0)
    with pytest.raises(afdm.AfdError, match="t_prev < t"):
        ops.ddim_step_var(x, e, z, ah, sig, 3, 3, 1.0)
    with pytest.raises(afdm.AfdError, match="eta >= 0"):
        ops.ddim_step_var(x, e, z, ah, sig, 5, 3, -1.0)
    with pytest.raises(afdm.AfdError, match="eps2"):
        ops.ddim_step_var_cfg(x, e, z, ah, sig, 5, 3, 1.0, 3.0)
    with pytest.raises(afdm.AfdError, match="contiguous"):
        ops.ddim_step_var(x, e.transpose(2, 3), z, ah, sig, 5, 3, 1.0)
    with pytest.raises(afdm.AfdError, match="int64 device"):
        ops.ddim_step_var_dev(x, e, z, ah, sig, torch.tensor([5]), torch.tensor([3]), 1.0, x.clone())
    lib = afdm.lib()                                                    # the C entry point itself: NULL sig, nothing launched
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_var: .*sig.* must not be NULL"):
        lib.afd_ddim_step_var(x.data_ptr(), e.data_ptr(), None, ah.data_ptr(), None, 5, 3, 1.0, x.data_ptr(), x.numel(), None)
    torch.cuda.synchronize()


# ---- 2. the per-row squared norms -------------------------------------------------------------------------------------------------
SQNORM_SHAPES = [(1, 1), (5, 193), (3, 255), (2, 4096), (2, 12288)]


def _placed(v, off):
    """A copy of the contiguous v whose first element lies 4 * off bytes past a 16-byte boundary."""
    flat = torch.empty(v.numel() + 4, device=v.device, dtype=v.dtype)
    base = (-(flat.data_ptr() // 4)) % 4                               # elements up to the next 16-byte boundary
    out = flat[base + off:base + off + v.numel()].view(v.shape)
    out.copy_(v)
    assert out.data_ptr() % 16 == 4 * off
    return out


@pytest.mark.parametrize("B,chw", SQNORM_SHAPES)
def test_eps_sqnorm_rows(A, B, chw):
    afdm, dev = A
    from afdm import ops
    g = torch.Generator().manual_seed(B * 100003 + chw)
    eps = torch.randn(B, chw, generator=g)
    eps[B - 1, chw // 2] = 1e20                                         # its square overflows fp32, not fp64
    want = eps.double().square().sum(1)
    aligned, shifted = _placed(eps.to(dev), 0), _placed(eps.to(dev), 1)
    got = ops.eps_sqnorm_rows(aligned)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B,) and bool(torch.isfinite(got).all())
    rel = float(((got.cpu() - want).abs() / want).max())
    note("Analytic-DPM: eps_sqnorm_rows vs an fp64 sum", rel, (B, chw))
    assert rel <= 4 * chw * 2.0 ** -53, (B, chw, rel)                   # the squares are exact in fp64: only the order differs
    assert torch.equal(got, ops.eps_sqnorm_rows(aligned))               # call to call
    assert torch.equal(got, ops.eps_sqnorm_rows(shifted))               # 16-byte loads or scalar loads
    out = torch.full((B,), float("nan"), device=dev, dtype=torch.float64)
    assert ops.eps_sqnorm_rows(aligned, out=out) is out and torch.equal(out, got)
    # the guided form: the plain form of the lerped halves, bit for bit, on either side of ATen's |s| < 0.5 branch
    eps2 = torch.randn(2 * B, chw, generator=g).to(dev)
    for s in (3.0, 0.3):
        lerped = _lerp_restated(eps2[B:], eps2[:B], s).contiguous()
        want_g = ops.eps_sqnorm_rows(lerped)
        for off in (0, 1):
            assert torch.equal(ops.eps_sqnorm_rows(_placed(eps2, off), s), want_g), (B, chw, s, off)
    torch.cuda.synchronize()


def test_eps_sqnorm_rows_checks_its_arguments(A):
    afdm, dev = A
    from afdm import ops
    e = torch.randn(3, 4, 8, 8, device=dev)
    with pytest.raises(afdm.AfdError, match="fp32"):
        ops.eps_sqnorm_rows(e.double())
    with pytest.raises(afdm.AfdError, match="HIP device"):
        ops.eps_sqnorm_rows(e.cpu())
    with pytest.raises(afdm.AfdError, match="2B rows"):
        ops.eps_sqnorm_rows(e, 3.0)
    with pytest.raises(afdm.AfdError, match="non-empty"):
        ops.eps_sqnorm_rows(e.flatten())
    with pytest.raises(afdm.AfdError, match="out must be a contiguous fp64 device tensor"):
        ops.eps_sqnorm_rows(e, out=torch.empty(3, device=dev))
    assert torch.equal(ops.eps_sqnorm_rows(e.transpose(2, 3)), ops.eps_sqnorm_rows(e.transpose(2, 3).contiguous()))


# ---- 3. Gaussian data: estimation and sampling -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gauss(A):
    """x0 ~ N(mu, 0.5^2 I) on 4 x 32 x 32, its exact eps-model, the exact table and the one estimated on ddim_timesteps(10)."""
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    mu = _mu(dev, 0.8)
    model = _GaussEps(mu, diff.alpha_hat)
    exact = _gauss_gamma(diff)
    afdm.set_seed(21)
    images = (mu + 0.5 * torch.randn((160, 4, 32, 32), device=dev, dtype=torch.float64)).float()      # beyond [-1, 1]: nothing is clipped
    est = diff.estimate_analytic_variance(model, images, timesteps=10, rows_per_step=16, batch=64)
    return {"diff": diff, "mu": mu, "model": model, "exact": exact, "estimated": est,
            "exact_table": afdm.AnalyticVariance.for_diffusion(diff, exact)}


def test_estimate_recovers_the_exact_table(A, gauss):
    diff, est, exact = gauss["diff"], gauss["estimated"], gauss["exact"]
    chain = diff.ddim_timesteps(10)
    assert est.gamma.dtype == np.float64 and est.gamma.shape == (T,) and est.count.dtype == np.int64
    assert sorted(np.flatnonzero(~np.isnan(est.gamma)).tolist()) == sorted(chain)
    assert est.count.sum() == 160 and all(est.count[t] == 16 for t in chain)
    assert (est.noise_steps, est.schedule, est.prediction) == (T, "linear", "eps")
    assert np.array_equal(est.alpha_hat, diff.alpha_hat.cpu().numpy())
    worst = max(abs(est.gamma[t] / exact[t] - 1.0) for t in chain)
    note("Analytic-DPM: estimated G_t vs exact (16 rows per step)", worst, "Gaussian data")
    print(f"estimated G_t: worst relative error {worst:.3%}")
    assert worst <= 0.03                                                # the Monte-Carlo sd is sqrt(2 / (16 * 4096)) = 0.55 %
    assert gauss["model"].training                                      # found in train mode, left in it


@pytest.mark.parametrize("table,eta", [("exact_table", 0.0), ("exact_table", 1.0), ("estimated", 1.0)])
def test_analytic_sampling_has_the_data_variance(A, gauss, table, eta):
    afdm, dev = A
    diff, mu, model = gauss["diff"], gauss["mu"], gauss["model"]
    a0 = float(diff.alpha_hat[0].double())
    target = 0.25 * a0 + 1.0 - a0

    def pooled(**kw):
        afdm.set_seed(31)
        draw = diff.sample_analytic if "analytic" in kw else diff.sample
        x = draw(model, n=64, image_channels=4, steps=10, eta=eta, noise_source="device", return_float=True, **kw)[2]
        return float((x.double() - math.sqrt(a0) * mu).square().mean())

    with_table, without = pooled(analytic=gauss[table]), pooled()
    note(f"Analytic-DPM: sample variance vs the data's, S = 10, eta = {eta}", abs(with_table / target - 1.0), table)
    print(f"S = 10, eta = {eta}, {table}: variance / target = {with_table / target:.4f} (analytic), {without / target:.4f} (lambda^2 alone)")
    assert abs(with_table / target - 1.0) <= 0.03
    assert abs(without / target - 1.0) > 0.30                            # derived: 47 % (eta = 0) and 58 % (eta = 1) short
    assert model.training


# ---- 4. the loop: graph replay, the noise drawn, the model's state ------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_analytic_graph_equals_eager(A, guided, eta):
    afdm, dev = A
    model = _model(afdm, dev, num_classes=K if guided else None)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    av = afdm.AnalyticVariance.for_diffusion(diff, np.random.default_rng(1).uniform(0.2, 0.9, T))
    kw = {"labels": torch.tensor([1, afdm.NULL_LABEL, 8], device=dev), "cfg_scale": 3.0} if guided else {}
    outs = []
    for use_graph in (False, True):
        afdm.set_seed(5)
        xq, rq, xf = diff.sample_analytic(model, n=3, image_channels=3, analytic=av, noise_source="device", return_float=True,
                                          graph=use_graph, steps=6, eta=eta, **kw)
        outs.append((xq.cpu(), rq.cpu(), xf.cpu(), [s.cpu() for s in diff.last_float_snapshots], torch.randn(8, device=dev).cpu()))
    assert model.training and model._t_range is None
    assert bool(torch.isfinite(outs[0][2]).all())
    assert _same_bits(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert len(outs[0][3]) == len(outs[1][3]) and all(_same_bits(a, b) for a, b in zip(outs[0][3], outs[1][3]))
    assert torch.equal(outs[0][4], outs[1][4])                                 # the generator state after the trajectory


@pytest.mark.parametrize("graph", [False, True])
def test_analytic_draws_the_noise_of_ancestral_ddim_also_at_eta_0(A, graph):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    av = afdm.AnalyticVariance.for_diffusion(diff, np.full(T, 0.5))
    S, after = 6, []
    for kw in ({"eta": 1.0}, {"eta": 0.0, "analytic": av}, {"eta": 1.0, "analytic": av}):
        afdm.set_seed(3)
        draw = diff.sample_analytic if "analytic" in kw else diff.sample
        draw(model, n=2, image_channels=3, noise_source="device", steps=S, graph=graph, **kw)
        after.append(torch.randn(64, device=dev))
    afdm.set_seed(3)
    for _ in range(1 + (S - 1)):                                         # x_T and one draw per step but the last
        torch.randn((2, 3, 32, 32), device=dev)
    want = torch.randn(64, device=dev)
    assert all(torch.equal(a, want) for a in after)
    # ... and with DDIM's own sigmas in the table the trajectory is ancestral DDIM's, bit for bit
    afdm.set_seed(3)
    plain = diff.sample(model, n=2, image_channels=3, noise_source="device", steps=S, eta=1.0, return_float=True, graph=graph)[2]
    afdm.set_seed(3)
    got = diff.sample_analytic(model, 2, 3, _Own(diff, 1.0), noise_source="device", steps=S, eta=1.0, return_float=True, graph=graph)[2]
    assert _same_bits(got, plain)


def _Own(diff, eta):
    """An AnalyticVariance whose sigma table holds DDIM's own fp32 sigmas, whatever its gamma says."""
    import afdm

    class Own(afdm.AnalyticVariance):
        def sigma_table(self, diffusion, pairs, eta_, last_sigma_max=None):
            ah = diffusion.alpha_hat.cpu()
            tab = torch.zeros(diffusion.noise_steps)
            for t, tp in pairs:
                tab[t] = _coef32(ah, t, tp, eta_)["sigma"]
            return tab

    return Own.for_diffusion(diff, np.full(diff.noise_steps, 0.5))


def test_analytic_loop_restores_the_model_after_an_exception(A):
    afdm, dev = A

    class Boom(afdm.UNet):
        calls = 0

        def forward(self, *a, **kw):
            Boom.calls += 1
            if Boom.calls == 3:
                raise RuntimeError("boom at the third step")
            return super().forward(*a, **kw)

    afdm.set_seed(42)
    model = Boom(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    av = afdm.AnalyticVariance.for_diffusion(diff, np.full(T, 0.5))
    with pytest.raises(RuntimeError, match="third step"):
        diff.sample_analytic(model, n=2, image_channels=3, analytic=av, noise_source="device", steps=10, eta=1.0)
    assert Boom.calls == 3 and model.training and model._t_range is None


# ---- 5. v-prediction and learned variances go through predict_eps -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v", "learned", "guided"])
def test_estimate_on_other_model_kinds_equals_a_hand_loop(A, kind):
    afdm, dev = A
    from afdm import ops
    learned, guided = kind == "learned", kind == "guided"
    model = _model(afdm, dev, c_out=6 if learned else 3, num_classes=K if guided else None)
    kw = {"variance": "learned"} if learned else ({} if guided else {"prediction": "v"})
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, **kw)
    ts, per_step, batch, N = [900, 500, 37], 2, 4, 3
    g = torch.Generator().manual_seed(9)
    images = torch.rand(N, 3, 32, 32, generator=g) * 2 - 1
    labels = torch.tensor([1, 7, afdm.NULL_LABEL]) if guided else None
    s = 2.0
    drawn = []

    def noise_fn(shape):
        drawn.append(torch.randn(shape, generator=g).to(dev))
        return drawn[-1]

    model.eval()                                                         # (found in eval mode: it must come back in it)
    av = diff.estimate_analytic_variance(model, images, timesteps=ts, rows_per_step=per_step, batch=batch, noise_fn=noise_fn,
                                         **({"labels": labels, "cfg_scale": s} if guided else {}))
    assert not model.training and model._t_range is None
    assert [tuple(z.shape) for z in drawn] == [(4, 3, 32, 32), (2, 3, 32, 32)]
    t_rows = torch.tensor(np.repeat(ts, per_step), device=dev)
    img = torch.arange(len(ts) * per_step, device=dev) % N
    x0 = images.to(dev)
    sums = []
    with torch.no_grad():
        for (lo, hi), z in zip(((0, 4), (4, 6)), drawn):
            t = t_rows[lo:hi].contiguous()
            xt = ops.noise_images(x0[img[lo:hi]].contiguous(), z, t, diff.alpha_hat)
            if learned:
                e = ops.split_pred(model(xt, t).contiguous(), xt, t, diff.alpha_hat, "eps")
            elif guided:
                y = labels.to(dev)[img[lo:hi]]
                e2 = diff.predict_eps(model, torch.cat([xt, xt]), torch.cat([t, t]), torch.cat([y, torch.full_like(y, afdm.NULL_LABEL)]))
                e = _lerp_restated(e2[hi - lo:], e2[:hi - lo], s)
            else:
                e = diff.predict_eps(model, xt, t)
            sums.append(e.double().square().sum((1, 2, 3)))
    sums = torch.cat(sums).cpu().numpy()
    model.train()
    per = 3 * 32 * 32
    for k, t in enumerate(ts):
        want = sums[k * per_step:(k + 1) * per_step].sum() / (per_step * per)
        assert av.count[t] == per_step
        assert abs(av.gamma[t] - want) <= 4 * per * 2.0 ** -53 * want, (kind, t, av.gamma[t], want)
    assert np.isnan(av.gamma).sum() == T - len(ts) and av.prediction == diff.prediction


# ---- 6. the likelihood bound with the analytic variance -----------------------------------------------------------------------------
def _bounds_on_the_cpu(x0, mu, s2):
    """vb_bpd per image for sigma = "beta", "posterior" and the exact analytic table, in torch fp64 on the CPU from
    vlb_coefficients' formulas: sum_{t >= 2} (w_t |eps_hat - eps|^2 + D c_t) / (D ln 2)."""
    import afdm
    d = afdm.Diffusion(noise_steps=T, img_size=32, device="cpu")
    ah = d.alpha_hat.double()
    x0 = d.snap_8bit(x0).double()
    per = x0[0].numel()
    eps = torch.randn((T,) + tuple(x0.shape), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    out = {}
    for name, sigma in (("beta", "beta"), ("posterior", "posterior"), ("analytic", afdm.AnalyticVariance.for_diffusion(d, _gauss_gamma(d, s2)))):
        c = d.vlb_coefficients(sigma)
        vb = torch.zeros(x0.shape[0], dtype=torch.float64)
        for t in range(2, T):
            a = ah[t]
            xt = a.sqrt() * x0 + (1 - a).sqrt() * eps[t]
            eh = (1 - a).sqrt() * (xt - a.sqrt() * mu) / (s2 * a + 1 - a)
            vb += c[t, 0] * (eh - eps[t]).square().flatten(1).sum(1) + per * c[t, 1]
        out[name] = vb / (per * math.log(2.0))
    return out


def test_calc_bpd_with_the_analytic_variance_is_the_tightest(A):
    """The optimal variance minimises every KL term of the bound, so vb_bpd with the analytic table is not above the bound with
    beta or with beta~.  The CPU evaluation (fp64, the exact table, its own noise) gives, for the two images,
    beta 2.7920 / 2.8026, posterior 3.0433 / 3.0539, analytic 2.7636 / 2.7746 bits per dimension: a gap of 0.0284 and 0.0280.
    On the GPU the inequality is asserted with half that gap as slack: vb_bpd(analytic) <= min(beta, posterior) - gap / 2 (measured on
    one MI355X with the estimated table: 2.7880 / 2.7983, 3.0376 / 3.0466 and 2.7596 / 2.7703)."""
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    s2 = 0.01
    mu_host = _mu("cpu", 0.5)
    g = torch.Generator().manual_seed(0)
    images = (mu_host + 0.1 * torch.randn(2, 4, 32, 32, generator=g, dtype=torch.float64)).float()     # within [-1, 1]: nothing clips
    assert float(images.abs().max()) < 1.0
    cpu = _bounds_on_the_cpu(images, mu_host, s2)
    gap = torch.minimum(cpu["beta"], cpu["posterior"]) - cpu["analytic"]
    print("CPU vb_bpd:", {k: v.tolist() for k, v in cpu.items()}, "gap", gap.tolist())
    assert bool((gap > 0).all())
    model = _GaussEps(mu_host.to(dev), diff.alpha_hat, s2)
    afdm.set_seed(17)
    av = diff.estimate_analytic_variance(model, images, rows_per_step=16, batch=1024)
    assert not np.isnan(av.gamma[1:]).any() and np.isnan(av.gamma[0])

    def run(sigma):
        gen = torch.Generator(device=dev).manual_seed(2)
        return diff.calc_bpd(model, images, sigma=sigma, batch=1024,
                             noise_fn=lambda shape: torch.randn(shape, generator=gen, device=dev))["vb_bpd"]

    vb = {"beta": run("beta"), "posterior": run("posterior"), "analytic": run(av)}
    print("GPU vb_bpd:", {k: v.tolist() for k, v in vb.items()})
    assert bool((vb["analytic"] <= torch.minimum(vb["beta"], vb["posterior"]) - 0.5 * gap).all())
    hole = afdm.AnalyticVariance.for_diffusion(diff, np.where(np.arange(T) == 500, np.nan, 0.5))
    with pytest.raises(ValueError, match="no estimate at timestep 500"):
        diff.calc_bpd(model, images, sigma=hole)


# ---- 7. from a checkpoint: uint8 pixels and a DeviceDataset ---------------------------------------------------------------------------
def test_analytic_results_from_a_checkpoint(A, tmp_path):
    afdm, dev = A
    model = _model(afdm, dev)
    path = tmp_path / "ckpt.pt"
    torch.save(model.state_dict(), path)
    data = {"args": afdm.argument(image_size=32, image_channels=3, device="cuda", noise_steps=T), "unet_v": 3, "seed": 42,
            "f_settings": dict(F_SET), "modelpath": str(path), "dataset": "toy"}
    pixels = torch.randint(0, 256, (3, 3, 32, 32), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    kw = {"timesteps": [900, 40], "rows_per_step": 4, "batch": 8}
    av = afdm.analytic_results(data, pixels, **kw)
    assert av.path == str(tmp_path / "analytic_toy_3.npz")
    back = afdm.AnalyticVariance.load(av.path)
    assert back.gamma.tobytes() == av.gamma.tobytes() and np.array_equal(back.count, av.count)
    assert sorted(np.flatnonzero(~np.isnan(av.gamma)).tolist()) == [40, 900] and av.count[900] == 4
    # the same table by hand after the checkpoint's seed (uint8 k -> k / 127.5 - 1), and through a DeviceDataset of those values
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    afdm.set_seed(42)
    x0 = pixels.float() / 127.5 - 1.0
    assert diff.estimate_analytic_variance(model, x0, **kw).gamma.tobytes() == av.gamma.tobytes()
    afdm.set_seed(42)
    ds = afdm.DeviceDataset(x0, device=dev)
    assert diff.estimate_analytic_variance(model, ds, **kw).gamma.tobytes() == av.gamma.tobytes()
    assert 0.0 < av.gamma[900] < 2.0 and model.training
