"""GPU tests of diffusion posterior sampling: the operator kernels against LinearOperator's cpu fp64 path and the adjoint identity,
ops.dps_residual and ops.dps_correct against fp64 restatements (bit-identical from call to call; a row whose sums are 0 is not
touched), the UNet's input vector-Jacobian product against autograd on the CPU oracle, `posterior_sample` against a loop restated
in torch fp64 with autograd on an analytic Gaussian model, that the guidance pulls the sample onto the measurement, what a step
runs (one forward, one backward) and leaves behind (the model's mode, hint and requires_grad flags, also after an exception), the
refusals, and `posterior_results` on a checkpoint."""
import math

import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
T = 1000
KINDS = ("eps", "v", "x0")


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _kernel(K, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.rand(K, K, generator=g) + 0.1
    return k / k.sum()


def _mask(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) < 0.6).float()


# (B, C, H, W, K, s, mask shape): a window wider than the measurement plane (K = 15 on 4 x 4), a non-square plane, odd B, the largest
# plane, the delta kernel
CASES = [(3, 3, 32, 32, 9, 1, None), (2, 1, 32, 32, 5, 2, (1, 16, 16)), (2, 3, 16, 16, 15, 4, (3, 4, 4)), (5, 3, 8, 8, 1, 1, (1, 8, 8)),
         (2, 2, 8, 16, 3, 2, None), (1, 1, 64, 64, 15, 1, None)]
IDS = ["x".join(str(v) for v in c[:6]) for c in CASES]


def _operator(afdm, case):
    B, C, H, W, K, s, ms = case
    return afdm.LinearOperator(_kernel(K, K) if K > 1 else None, s, None if ms is None else _mask(ms, 5))


# ---- 1. A and A^T against the cpu fp64 path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_operator_kernels_equal_the_cpu_path(A, case):
    afdm, dev = A
    B, C, H, W, K, s, ms = case
    op = _operator(afdm, case)
    g = torch.Generator().manual_seed(K + 10 * s)
    x = torch.randn(B, C, H, W, generator=g)
    r = torch.randn(B, C, H // s, W // s, generator=g)
    y_dev, g_dev = op.apply(x.to(dev)), op.adjoint(r.to(dev))
    assert y_dev.dtype == torch.float32 and y_dev.is_cuda and tuple(y_dev.shape) == (B, C, H // s, W // s)
    assert g_dev.dtype == torch.float32 and tuple(g_dev.shape) == (B, C, H, W)
    e1 = check("dps: afd_linop_apply vs cpu fp64", y_dev.cpu(), op.apply(x), 1e-5, case)
    e2 = check("dps: afd_linop_adjoint vs cpu fp64", g_dev.cpu(), op.adjoint(r), 1e-5, case)
    # <A x, r> = <x, A^T r> with both sides from the device, evaluated in fp64 on the host
    lhs = float((y_dev.cpu().double() * r.double()).sum())
    rhs = float((x.double() * g_dev.cpu().double()).sum())
    scale = float(y_dev.cpu().double().norm() * r.double().norm())
    gap = abs(lhs - rhs) / scale
    note("dps: device adjoint identity / (|Ax| |r|)", gap, case)
    print(f"{case}: apply {e1:.2e}, adjoint {e2:.2e}, identity {gap:.2e}")
    assert gap <= 1e-5
    assert _same_bits(op.apply(x.to(dev)), y_dev) and _same_bits(op.adjoint(r.to(dev)), g_dev)      # the same bits from call to call


# ---- 2. / 3. the step's two launches against fp64 restatements ------------------------------------------------------------------
def _coef(diff, t, like):
    a, b = diff.x0_coefficients(t)
    shape = (-1,) + (1,) * (like.dim() - 1)
    return a.view(shape), b.view(shape)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[2], CASES[4]], ids=[IDS[0], IDS[1], IDS[2], IDS[4]])
def test_dps_residual_equals_the_fp64_restatement(A, case, kind):
    afdm, dev = A
    from afdm import ops
    B, C, H, W, K, s, ms = case
    op = _operator(afdm, case)
    diff = afdm.Diffusion(noise_steps=T, img_size=H, device=dev, prediction=kind)
    g = torch.Generator().manual_seed(3 * K + s)
    x_t, out = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    y = torch.randn(B, C, H // s, W // s, generator=g)
    t = torch.tensor([1, T - 1, 500][:B])                                       # mixed per-row timesteps, both ends
    a, b = _coef(diff, t, x_t)
    r64 = op.apply(a * x_t.double() + b * out.double()) - y.double()
    want_g, want_s = op.adjoint(r64), (r64 * r64).flatten(2).sum(-1)
    call = lambda: ops.dps_residual(x_t.to(dev), out.to(dev), t.to(dev), diff.alpha_hat, kind, y.to(dev), op._taps, s,
                                    op._device_mask(dev))
    got_g, got_s = call()
    assert got_s.dtype == torch.float64 and tuple(got_s.shape) == (B, C)
    eg = check(f"dps: afd_dps_residual g vs fp64 ({kind})", got_g.cpu(), want_g, 1e-5, case)
    es = float(((got_s.cpu() - want_s).abs() / want_s).max())
    note(f"dps: afd_dps_residual sums, max relative ({kind})", es, case)
    print(f"{case} {kind}: g {eg:.2e}, sums {es:.2e}")
    assert es <= 1e-5
    again_g, again_s = call()
    assert _same_bits(again_g, got_g) and _same_bits(again_s, got_s)


@pytest.mark.parametrize("kind", KINDS)
def test_dps_correct_equals_the_fp64_restatement(A, kind):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=T, img_size=8, device=dev, prediction=kind)
    for shape in ((4, 3, 8, 8), (3, 2, 5, 7)):                                   # (a row length that is no multiple of 4 or 256)
        B, C = shape[:2]
        gen = torch.Generator().manual_seed(B)
        x, g, v = (torch.randn(shape, generator=gen) for _ in range(3))
        sums = torch.rand(B, C, generator=gen, dtype=torch.float64) * 50 + 0.1
        sums[1] = 0                                                              # this row's residual vanished: c_row = 0
        t = torch.tensor([1, 700, T - 1, 37][:B])
        a, b = _coef(diff, t, x)
        zeta = 2.5
        c = torch.where(sums.sum(1) > 0, zeta / sums.sum(1).sqrt(), torch.zeros(B, dtype=torch.float64)).view(-1, 1, 1, 1)
        want = x.double() - c * (a * g.double() + b * v.double())
        xd = x.to(dev)
        got = ops.dps_correct(xd, g.to(dev), v.to(dev), sums.to(dev), t.to(dev), diff.alpha_hat, kind, zeta)
        assert got.data_ptr() == xd.data_ptr()                                    # in place
        # fp32 products, sum, scaling and subtraction: a handful of roundings of 6e-8 on terms of the result's size (eps at
        # t = T - 1 scales g and v by 157 and c divides by |r| again)
        check(f"dps: afd_dps_correct vs fp64 ({kind})", got.cpu(), want, 1e-6, shape)
        assert _same_bits(got[1].cpu(), x[1])                                     # untouched, bit for bit
        assert not torch.equal(got[0].cpu(), x[0])
        x0 = x.to(dev)
        ops.dps_correct(x0, g.to(dev), v.to(dev), sums.to(dev), t.to(dev), diff.alpha_hat, kind, 0.0)
        assert _same_bits(x0.cpu(), x)                                            # zeta = 0: nothing moves


def test_ops_refuse_bad_arguments(A):
    afdm, dev = A
    from afdm import ops
    x = torch.zeros(2, 3, 8, 8, device=dev)
    k = _kernel(3, 1)
    with pytest.raises(afdm.AfdError, match="stride"):
        ops.linop_apply(x, k, 3)
    with pytest.raises(afdm.AfdError, match="kernel"):
        ops.linop_apply(x, torch.ones(4, 4))
    with pytest.raises(afdm.AfdError, match="mask"):
        ops.linop_apply(x, k, 1, torch.ones(2, 8, 8, device=dev))
    with pytest.raises(afdm.AfdError, match="multiples of the stride"):
        ops.linop_apply(torch.zeros(1, 1, 6, 8, device=dev), k, 4)
    with pytest.raises(afdm.AfdError, match=r"\[1, 64\]"):
        ops.linop_adjoint(torch.zeros(1, 1, 32, 32, device=dev), k, 4)
    with pytest.raises(afdm.AfdError, match="device tensor"):
        ops.linop_apply(x.cpu(), k)


# ---- 4. the UNet's input vector-Jacobian product -------------------------------------------------------------------------------------
def _pool_gaps(pooled):
    """Per 2 x 2 window of each recorded max-pool input, (largest - second largest) / the tensor's largest magnitude; the smallest."""
    worst = float("inf")
    for inp in pooled:
        B, C, H, W = inp.shape
        w = inp.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        top = w.topk(2, dim=-1).values
        worst = min(worst, float(((top[..., 0] - top[..., 1]) / inp.abs().max()).min()))
    return worst


@pytest.mark.parametrize("variant", [3, 0])
def test_unet_input_vjp_equals_the_cpu_oracle(A, variant, monkeypatch):
    afdm, dev = A
    from oracle import ref_ops as R
    import torch.nn.functional as F
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=variant).to(dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(2, 3, 32, 32, generator=g) * 2 - 1
    seed = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.tensor([500, 37])
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    xc = x.clone().requires_grad_(True)
    pooled, pool = [], F.max_pool2d
    monkeypatch.setattr(F, "max_pool2d", lambda inp, k: (pooled.append(inp.detach()), pool(inp, k))[1])
    ref_out = R.unet_forward(sd, xc, t, variant, dict(F_SET))
    monkeypatch.undo()
    (ref_v,) = torch.autograd.grad(ref_out, xc, seed)
    # Variant 0 pools with a maximum, whose gradient goes to the window's largest element: where the two largest are within
    # rounding of each other the device's forward may pick the other one, and the vector-Jacobian product is then another
    # function's (with the generator seeded 0 one window of image 0 at the 8 x 8 map has a relative gap of 3e-7, a few fp32 ulps, and the
    # device's product is 6.6e-3 off).  The input is chosen away from that: every window's gap is at least 1e-5 of its tensor's
    # largest magnitude, ten times the forward's rel-L2 gate and about 80 ulps.
    assert len(pooled) == (3 if variant == 0 else 0)
    assert _pool_gaps(pooled) >= 1e-5
    # plain autograd on the device, parameters as they are
    xd = x.to(dev).requires_grad_(True)
    (v_plain,) = torch.autograd.grad(model(xd, t.to(dev)), xd, seed.to(dev))
    e_plain = check(f"dps: UNet input VJP vs CPU oracle (variant {variant})", v_plain.cpu(), ref_v, 1e-4, "autograd.grad")
    assert all(p.grad is None for p in model.parameters())
    # the sampler's helper: frozen parameters meanwhile, everything as found afterwards
    first = next(model.parameters())
    first.requires_grad_(False)                                                   # one flag that was off stays off
    found = [p.requires_grad for p in model.parameters()]
    seen = []
    with torch.no_grad():                                                         # (the samplers' scope)
        out, v = diff._output_and_vjp(model, x.to(dev), t.to(dev), None, lambda o: (seen.append(o), seed.to(dev))[1])
    assert not out.requires_grad and not v.requires_grad and len(seen) == 1 and not seen[0].requires_grad
    check(f"dps: UNet forward vs CPU oracle (variant {variant})", out.cpu(), ref_out.detach(), 1e-5, "_output_and_vjp")
    e_frozen = check(f"dps: UNet input VJP vs CPU oracle (variant {variant})", v.cpu(), ref_v, 1e-4, "_output_and_vjp")
    print(f"variant {variant}: input VJP rel-L2 {e_plain:.2e} (autograd.grad), {e_frozen:.2e} (frozen parameters)")
    assert [p.requires_grad for p in model.parameters()] == found
    assert all(p.grad is None for p in model.parameters())


# ---- 5. / 6. trajectories against a loop restated in fp64 ------------------------------------------------------------------------
class _GaussModel(torch.nn.Module):
    """The exact prediction for x0 ~ N(mu, 0.5^2 I) (the _GaussEps of test_gpu_dpm.py), written so that autograd passes through:
    eps(x, t) = sqrt(1 - a) (x - sqrt(a) mu) / (0.25 a + 1 - a), a = alpha_hat[t], evaluated in fp64 and returned in x's dtype;
    "x0" and "v" follow from eps and x."""

    def __init__(self, mu, alpha_hat, prediction="eps"):
        super().__init__()
        self.mu, self.ah, self.prediction = mu.double(), alpha_hat.double(), prediction

    def forward(self, x, t):
        a = self.ah.to(x.device)[t].view(-1, 1, 1, 1)
        xd = x.double()
        eps = (1 - a).sqrt() * (xd - a.sqrt() * self.mu.to(x.device)) / (0.25 * a + 1 - a)
        if self.prediction == "eps":
            out = eps
        else:
            x0 = (xd - (1 - a).sqrt() * eps) / a.sqrt()
            out = x0 if self.prediction == "x0" else a.sqrt() * eps - (1 - a).sqrt() * x0
        return out.to(x.dtype)


def _restated(diff, model, y, op, zeta, moves, eta, n, C, S):
    """posterior_sample's loop in torch fp64 on the cpu with autograd, noise_source="cpu": the same fp32 draws in the same order.
    diff: a cpu Diffusion; model: fp64 in, fp64 out; eta None: the DDPM update."""
    ah, al, be = diff.alpha_hat.double(), diff.alpha.double(), diff.beta.double()
    x = torch.randn(n, C, S, S).double()
    y = y.double()
    for t, tp in moves:
        tt = torch.full((n,), t, dtype=torch.long)
        xg = x.clone().requires_grad_(True)
        out = model(xg, tt)
        a, b = _coef(diff, tt, x)
        norm = (op.apply(a * xg + b * out) - y).flatten(1).norm(dim=1)           # |y - A x0_hat| per row
        (grad,) = torch.autograd.grad(norm.sum(), xg)
        out = out.detach()
        a_t = float(ah[t])
        if diff.prediction == "eps":
            e = out
        elif diff.prediction == "x0":
            e = (x - math.sqrt(a_t) * out) / math.sqrt(1 - a_t)
        else:
            e = math.sqrt(a_t) * out + math.sqrt(1 - a_t) * x
        takes = (eta is None or eta > 0) and tp > 0
        z = torch.randn(n, C, S, S).double() if takes else None
        if eta is None:
            new = (x - (1 - float(al[t])) / math.sqrt(1 - a_t) * e) / math.sqrt(float(al[t]))
            if z is not None:
                new = new + math.sqrt(float(be[t])) * z
        else:
            a_p = float(ah[tp])
            x0 = (x - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
            var = eta * eta * (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
            new = math.sqrt(a_p) * x0 + math.sqrt(max(1 - a_p - var, 0.0)) * e
            if z is not None:
                new = new + math.sqrt(var) * z
        x = new - zeta * grad
    return x


def _consistency(op, x, y):
    """The mean over the images of |A x - y| / |y|, in fp64 on the host."""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    return float(((op.apply(x) - y).flatten(1).norm(dim=1) / y.flatten(1).norm(dim=1)).mean())


def _hole_operator(afdm):
    m = torch.ones(1, 16, 16)
    m[:, 4:12, 4:12] = 0
    return afdm.LinearOperator.inpainting(m)


def _setting(afdm, op, prediction="eps", noise_steps=T, seed=0):
    """mu, the measurement of one draw x0 ~ N(mu, 0.25 I) at sigma = 0.05 (fp32 values), the cpu process and the fp64 model."""
    g = torch.Generator().manual_seed(seed)
    mu = torch.rand(1, 3, 16, 16, generator=g, dtype=torch.float64) * 1.6 - 0.8
    x0 = mu + 0.5 * torch.randn(4, 3, 16, 16, generator=g, dtype=torch.float64)
    y = op.measure(x0, 0.05, generator=g).float()
    host = afdm.Diffusion(noise_steps=noise_steps, img_size=16, device="cpu", prediction=prediction)
    return mu, y, host, _GaussModel(mu, host.alpha_hat, prediction)


RUNS = {
    # name: (operator, prediction, noise_steps, steps, eta, zeta)
    "hole-ddim50-eta1": (_hole_operator, "eps", T, 50, 1.0, 4.0),
    "blur-stride2-ddim10-eta0": (lambda afdm: afdm.LinearOperator(afdm.gaussian_kernel(5, 1.0), 2), "eps", T, 10, 0.0, 4.0),
    "hole-ddpm20-v": (_hole_operator, "v", 20, None, None, 1.0),
}


@pytest.fixture(scope="module")
def trajectories(A):
    """Each run once, on the device and restated: {name: (operator, y, device x, restated x)}; and the zeta = 0 pair of the first."""
    afdm, dev = A
    res = {}
    for name, (make, prediction, steps_T, steps, eta, zeta) in list(RUNS.items()) + [("hole-ddim50-eta1-zeta0", RUNS["hole-ddim50-eta1"][:5] + (0.0,))]:
        op = make(afdm)
        mu, y, host, model64 = _setting(afdm, op, prediction, steps_T)
        diff = afdm.Diffusion(noise_steps=steps_T, img_size=16, device=dev, prediction=prediction)
        moves = [(t, t - 1) for t in range(steps_T - 1, 0, -1)] if steps is None else host._ddim_pairs(steps, eta)
        afdm.set_seed(5)
        want = _restated(host, model64, y, op, zeta, moves, eta, 4, 3, 16)
        afdm.set_seed(5)
        kw = {} if steps is None else {"steps": steps, "eta": eta}
        got = diff.posterior_sample(_GaussModel(mu, diff.alpha_hat, prediction), y.to(dev), op, zeta=zeta, noise_source="cpu",
                                    return_float=True, **kw)
        res[name] = (op, y, got, want)
    return res


@pytest.mark.parametrize("name", list(RUNS))
def test_trajectory_equals_the_fp64_restatement(A, trajectories, name):
    afdm, dev = A
    op, y, (xq, rq, x), want = trajectories[name]
    assert xq.dtype == torch.uint8 and tuple(xq.shape) == (4, 3, 16, 16) and x.dtype == torch.float32
    e = check("dps: posterior_sample vs fp64 restatement loop", x.cpu(), want, 1e-4, name)
    print(f"{name}: trajectory rel-L2 {e:.2e}")
    from afdm import ops
    assert torch.equal(xq, ops.quantize_u8(x))


def test_the_guidance_pulls_the_sample_onto_the_measurement(A, trajectories):
    op, y, (_, _, x), want = trajectories["hole-ddim50-eta1"]
    _, _, (_, _, x_free), want_free = trajectories["hole-ddim50-eta1-zeta0"]
    c = {"restated zeta=4": _consistency(op, want, y), "device zeta=4": _consistency(op, x, y),
         "restated zeta=0": _consistency(op, want_free, y), "device zeta=0": _consistency(op, x_free, y)}
    print("consistency |A x - y| / |y|:", ", ".join(f"{k} {v:.3f}" for k, v in c.items()))
    for k, v in c.items():
        note("dps: consistency " + k, v)
    assert c["restated zeta=4"] <= 0.25 and c["device zeta=4"] <= 0.25
    assert c["restated zeta=0"] >= 0.9 and c["device zeta=0"] >= 0.9


# ---- 7. what a step runs and what the call leaves behind ---------------------------------------------------------------------------
def _unet(afdm, dev, cls=None, **kw):
    afdm.set_seed(42)
    return (cls or afdm.UNet)(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


def test_one_forward_and_one_backward_per_step_and_the_snapshots(A):
    afdm, dev = A

    class Counting(torch.nn.Module):
        def __init__(self, inner):
            super().__init__()
            self.inner, self.forwards, self.backwards, self.grad_modes = inner, 0, 0, []

        def _hook(self, grad):
            self.backwards += 1

        def forward(self, x, t):
            self.forwards += 1
            self.grad_modes.append((torch.is_grad_enabled(), x.requires_grad))
            out = self.inner(x, t)
            out.register_hook(self._hook)
            return out

    op = _hole_operator(afdm)
    mu, y, host, _ = _setting(afdm, op)
    diff = afdm.Diffusion(noise_steps=T, img_size=16, device=dev)
    model = Counting(_GaussModel(mu, diff.alpha_hat))
    steps = [950, 900, 850, 500, 499, 100, 99, 1]                                # five of these moves cross a multiple of 100
    afdm.set_seed(1)
    xq, rq = diff.posterior_sample(model, y.to(dev), op, zeta=1.0, steps=steps, eta=1.0, noise_source="device")
    assert model.forwards == len(steps) and model.backwards == len(steps)
    assert all(mode == (True, True) for mode in model.grad_modes)
    assert len(diff.last_float_snapshots) == 6 and tuple(rq.shape) == (6 * 4, 3, 16, 16) and tuple(xq.shape) == (4, 3, 16, 16)
    assert model.training
    diff.sample(_GaussModel(mu, diff.alpha_hat), n=4, image_channels=3, steps=steps, eta=1.0, noise_source="device")
    assert len(diff.last_float_snapshots) == 6                                   # `sample` keeps the same ones
    # the DDPM chain: T - 1 steps, a snapshot at every i % 100 == 0 and the final x
    d6 = afdm.Diffusion(noise_steps=201, img_size=16, device=dev)
    model = Counting(_GaussModel(mu, d6.alpha_hat))
    d6.posterior_sample(model, y.to(dev), op, zeta=0.5, noise_source="device")
    assert model.forwards == 200 and model.backwards == 200 and len(d6.last_float_snapshots) == 3


def test_unet_runs_with_labels_and_is_left_as_found(A):
    afdm, dev = A
    op = afdm.LinearOperator.super_resolution(4)
    d6 = afdm.Diffusion(noise_steps=6, img_size=32, device=dev)
    g = torch.Generator().manual_seed(2)
    y = op.measure(torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, 0.05, generator=g).float().to(dev)
    model = _unet(afdm, dev, num_classes=10)
    found = [p.requires_grad for p in model.parameters()]

    def run(labels):
        afdm.set_seed(3)
        return d6.posterior_sample(model, y, op, zeta=1.0, labels=labels, noise_source="device", return_float=True)[2]

    x_a, x_b, x_a2 = run(torch.tensor([1, 2])), run(torch.tensor([3, 4])), run(torch.tensor([1, 2]))
    assert bool(torch.isfinite(x_a).all()) and not torch.equal(x_a, x_b)           # the labels reach the model
    assert _same_bits(x_a, x_a2)                                                   # and the call repeats bit for bit
    assert model.training and model._t_range is None
    assert [p.requires_grad for p in model.parameters()] == found and all(p.grad is None for p in model.parameters())


def test_model_is_restored_after_an_exception(A):
    afdm, dev = A

    class Boom(afdm.UNet):
        calls = 0

        def forward(self, *a, **kw):
            Boom.calls += 1
            if Boom.calls == 3:
                raise RuntimeError("boom at forward 3")
            return super().forward(*a, **kw)

    model = _unet(afdm, dev, Boom)
    d6 = afdm.Diffusion(noise_steps=6, img_size=32, device=dev)
    op = afdm.LinearOperator.gaussian_blur(5, 1.0)
    assert model.training and model._t_range is None
    with pytest.raises(RuntimeError, match="boom at forward 3"):
        d6.posterior_sample(model, torch.zeros(2, 3, 32, 32, device=dev), op, noise_source="device")
    torch.cuda.synchronize()
    assert Boom.calls == 3 and model.training and model._t_range is None
    assert all(p.requires_grad for p in model.parameters()) and all(p.grad is None for p in model.parameters())


def test_refusals_on_the_device(A):
    afdm, dev = A

    class Never(afdm.UNet):
        def forward(self, *a, **kw):
            raise AssertionError("the model was called before the checks passed")

    model = _unet(afdm, dev, Never)
    d6 = afdm.Diffusion(noise_steps=6, img_size=32, device=dev)
    op = afdm.LinearOperator.super_resolution(2)
    y = torch.zeros(2, 3, 16, 16, device=dev)
    bad = lambda: pytest.raises(ValueError, match=r"^Diffusion\.posterior_sample: ")
    with bad():
        d6.posterior_sample(model, y, op, zeta=-0.5)
    with bad():
        d6.posterior_sample(model, y, op, zeta=float("nan"))
    with bad():
        d6.posterior_sample(model, torch.zeros(2, 3, 32, 32, device=dev), op)
    with bad():
        d6.posterior_sample(model, y, lambda x: x)
    with bad():
        afdm.Diffusion(noise_steps=6, img_size=32, device=dev, variance="learned").posterior_sample(model, y, op)
    with pytest.raises(ValueError, match="no label embedding"):
        d6.posterior_sample(model, y, op, labels=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match="emits 3 channels"):                    # the model's channels against the measurement's
        d6.posterior_sample(model, torch.zeros(2, 1, 16, 16, device=dev), op)
    with pytest.raises(TypeError):                                               # classifier-free guidance is not offered
        d6.posterior_sample(model, y, op, labels=torch.tensor([0, 1]), cfg_scale=3.0)
    assert model.training and model._t_range is None


# ---- 8. from a checkpoint -----------------------------------------------------------------------------------------------------------
def test_posterior_results_from_a_checkpoint(A, tmp_path):
    afdm, dev = A
    model = _unet(afdm, dev)
    path = tmp_path / "ckpt.pt"
    torch.save(model.state_dict(), path)
    data = {"args": afdm.argument(image_size=32, image_channels=3, device="cuda", noise_steps=T), "unet_v": 3, "seed": 42,
            "f_settings": dict(F_SET), "modelpath": str(path)}
    g = torch.Generator().manual_seed(1)
    pixels = torch.randint(0, 256, (3, 3, 32, 32), generator=g, dtype=torch.uint8)
    op = afdm.LinearOperator.super_resolution(4)
    res = afdm.posterior_results(data, pixels, op, n=2, steps=4)
    assert list(res) == ["n", "steps", "eta", "sigma", "zeta", "psnr", "ssim", "consistency", "baseline"]
    assert (res["n"], res["steps"], res["eta"], res["sigma"], res["zeta"]) == (2, 4, 1.0, 0.05, 1.0)
    assert list(res["baseline"]) == ["psnr", "ssim", "consistency"]
    for scores in (res, res["baseline"]):
        for key in ("psnr", "ssim", "consistency"):
            assert list(scores[key]) == ["mean", "std", "values"] and len(scores[key]["values"]) == 2
            assert all(math.isfinite(v) for v in scores[key]["values"] + [scores[key]["mean"], scores[key]["std"]])
    assert all(v >= 0 for v in res["consistency"]["values"] + res["baseline"]["consistency"]["values"])
    again = afdm.posterior_results(data, afdm.DeviceDataset(pixels, device=dev), op, n=2, steps=4)      # a DeviceDataset: the same numbers
    assert again == res
