"""GPU tests of the probability-flow ODE likelihood: ops.ode_trace_rows against fp64 numpy (bit-identical from call to call,
exact on small integers), ops.ode_heun_step against an fp64 restatement, the ops' refusals, `Diffusion.ode_likelihood` against
`ode_likelihood_reference` on the same probes for an analytic Gaussian model (diagonal Jacobian), a convolution (non-diagonal) and
the UNet against its CPU oracle, against the closed form, what a move runs and what the call leaves behind, and
`likelihood_results` on a checkpoint."""
import math
import os

import numpy as np
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


# ---- 1. ops.ode_trace_rows -----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (3, 3), (1, 64), (3, 255), (2, 256), (3, 257), (5, 1023), (2, 1025), (3, 3072), (1, 12288)]


@pytest.mark.parametrize("with_w", [True, False], ids=["w", "no_w"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_trace_rows_equals_fp64_numpy(A, shape, with_w):
    afdm, dev = A
    from afdm import ops
    rows, per = shape
    g = torch.Generator().manual_seed(rows * 100003 + per)
    v = torch.randn(rows, per, generator=g)
    w = torch.randn(rows, per, generator=g) if with_w else None
    acc0 = torch.randn(rows, generator=g, dtype=torch.float64) * 100                # preloaded, not zero
    cvv, cvw = 0.37, (-1.9 if with_w else 0.0)
    vd, wd = v.to(dev), None if w is None else w.to(dev)
    acc = acc0.to(dev)
    assert ops.ode_trace_rows(vd, wd, cvv, cvw, acc) is acc
    again = acc0.to(dev)
    ops.ode_trace_rows(vd, wd, cvv, cvw, again)
    assert _same_bits(acc, again)                                                   # two calls, the same bits
    v64 = v.double().numpy()
    svv = (v64 * v64).sum(1)
    svw = (v64 * w.double().numpy()).sum(1) if with_w else np.zeros(rows)
    sabs = np.abs(v64 * w.double().numpy()).sum(1) if with_w else np.zeros(rows)
    want = acc0.numpy() + (cvv * svv + cvw * svw)
    got = acc.cpu().numpy()
    # fp64 summation of exact products: at most per * 2^-53 relative to the absolute sum, and the last addition's rounding
    bound = 1e-12 * (abs(cvv) * svv + abs(cvw) * sabs) + np.spacing(np.abs(want))
    worst = float((np.abs(got - want) / bound).max())
    note("likelihood: ode_trace_rows |diff| / bound (absolute)", worst, (shape, with_w))
    assert worst <= 1.0
    # a view that is not 16-byte aligned takes the scalar path and adds alike
    if per % 4 == 0 and per >= 8:
        pad_v = torch.zeros(rows * per + 1, device=dev)
        pad_v[1:] = vd.flatten()
        pad_w = None
        if with_w:
            pad_w = torch.zeros(rows * per + 1, device=dev)
            pad_w[1:] = wd.flatten()
            pad_w = pad_w[1:].view(rows, per)
        shifted = acc0.to(dev)
        ops.ode_trace_rows(pad_v[1:].view(rows, per), pad_w, cvv, cvw, shifted)
        assert _same_bits(acc, shifted)


@pytest.mark.parametrize("shape", [(3, 257), (2, 1024), (1, 12288)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_trace_rows_is_exact_on_small_integers(A, shape):
    afdm, dev = A
    from afdm import ops
    rows, per = shape
    g = torch.Generator().manual_seed(per)
    v = torch.randint(-8, 9, (rows, per), generator=g).float()
    w = torch.randint(-8, 9, (rows, per), generator=g).float()
    acc0 = torch.randint(-1000, 1000, (rows,), generator=g).double()
    acc = acc0.to(dev)
    ops.ode_trace_rows(v.to(dev), w.to(dev), 3.0, -0.5, acc)
    want = acc0 + 3.0 * (v.double() ** 2).sum(1) - 0.5 * (v.double() * w.double()).sum(1)
    assert _same_bits(acc.cpu(), want)
    only = acc0.to(dev)
    ops.ode_trace_rows(v.to(dev), None, -0.5, 0.0, only)                           # the prior's launch
    assert _same_bits(only.cpu(), acc0 - 0.5 * (v.double() ** 2).sum(1))


# ---- 2. ops.ode_heun_step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 4096, 4097])                              # (4096: the 16-byte path)
@pytest.mark.parametrize("move", [(1, 2), (1, 999), (500, 501), (300, 700)], ids=lambda m: f"{m[0]}to{m[1]}")
def test_heun_step_equals_the_fp64_restatement(A, move, n):
    afdm, dev = A
    from afdm import ops
    s, u = move
    diff = afdm.Diffusion(noise_steps=T, img_size=8, device=dev)
    g = torch.Generator().manual_seed(s * 1000 + u + n)
    x, es, eu = (torch.randn(n, generator=g) for _ in range(3))
    ah = diff.alpha_hat.detach().cpu().double()
    a_s, a_u = float(ah[s]), float(ah[u])
    h = math.sqrt((1 - a_u) / a_u) - math.sqrt((1 - a_s) / a_s)
    want = math.sqrt(a_u) * (x.double() / math.sqrt(a_s) + h * (es.double() + eu.double()) / 2)
    xd, esd, eud = x.to(dev), es.to(dev), eu.to(dev)
    out = ops.ode_heun_step(xd, esd, eud, diff.alpha_hat, s, u)
    assert out.data_ptr() != xd.data_ptr() and torch.equal(xd.cpu(), x)            # apart from x: x is not written
    check("likelihood: ode_heun_step vs fp64", out.cpu(), want, 1e-6, (move, n))
    inplace = xd.clone()
    assert ops.ode_heun_step(inplace, esd, eud, diff.alpha_hat, s, u, inplace) is inplace
    assert _same_bits(inplace, out)                                                 # x_out aliasing x: the same bits
    if n > 4:                                                                        # an unaligned view: the scalar path, the same bits
        pad = torch.zeros(n + 1, device=dev)
        pad[1:] = xd
        assert _same_bits(ops.ode_heun_step(pad[1:], esd, eud, diff.alpha_hat, s, u), out)


def test_ops_refuse_bad_arguments(A):
    afdm, dev = A
    from afdm import ops
    E = afdm.AfdError
    v = torch.zeros(2, 3, 8, 8, device=dev)
    acc = torch.zeros(2, device=dev, dtype=torch.float64)
    with pytest.raises(E, match="fp32 only"):
        ops.ode_trace_rows(v.double(), None, 1.0, 0.0, acc)
    with pytest.raises(E, match="HIP device"):
        ops.ode_trace_rows(v.cpu(), None, 1.0, 0.0, acc)
    with pytest.raises(E, match="contiguous"):
        ops.ode_trace_rows(v.transpose(2, 3), None, 1.0, 0.0, acc)
    with pytest.raises(E, match="w must be None or a contiguous tensor of v's shape"):
        ops.ode_trace_rows(v, torch.zeros(2, 3, 8, 4, device=dev), 1.0, 1.0, acc)
    with pytest.raises(E, match="w must be None or a contiguous tensor of v's shape"):
        ops.ode_trace_rows(v, v.transpose(2, 3), 1.0, 1.0, acc)
    with pytest.raises(E, match="w may be None only when cvw == 0"):
        ops.ode_trace_rows(v, None, 1.0, 1.0, acc)
    for bad in (acc.float(), acc.cpu(), torch.zeros(3, device=dev, dtype=torch.float64), torch.zeros(2, 2, device=dev, dtype=torch.float64)[:, 0]):
        with pytest.raises(E, match="acc must be a contiguous"):
            ops.ode_trace_rows(v, None, 1.0, 0.0, bad)
    with pytest.raises(E, match="finite"):
        ops.ode_trace_rows(v, v, float("nan"), 1.0, acc)
    assert float(acc.abs().sum()) == 0.0                                            # nothing was launched
    diff = afdm.Diffusion(noise_steps=T, img_size=8, device=dev)
    x = torch.zeros(2, 3, 8, 8, device=dev)
    with pytest.raises(E, match="fp32 only"):
        ops.ode_heun_step(x.double(), x, x, diff.alpha_hat, 1, 2)
    with pytest.raises(E, match="HIP device"):
        ops.ode_heun_step(x, x.cpu(), x, diff.alpha_hat, 1, 2)
    with pytest.raises(E, match="contiguous"):
        ops.ode_heun_step(x, x, x.transpose(2, 3), diff.alpha_hat, 1, 2)
    with pytest.raises(E, match="elements"):
        ops.ode_heun_step(x, x[:1], x, diff.alpha_hat, 1, 2)
    with pytest.raises(E, match="elements"):
        ops.ode_heun_step(x, x, x[:1], diff.alpha_hat, 1, 2)
    for s, u in ((0, 1), (5, 5), (7, 3), (1, T)):
        with pytest.raises(E, match="needs 1 <= s < u"):
            ops.ode_heun_step(x, x, x, diff.alpha_hat, s, u)
    with pytest.raises(E, match="must not overlap eps_s or eps_u"):
        eps = torch.zeros_like(x)
        ops.ode_heun_step(x, eps, x.clone(), diff.alpha_hat, 1, 2, eps)


# ---- 3. ode_likelihood on an analytic Gaussian model: a diagonal Jacobian -----------------------------------------------------------
class _GaussModel(torch.nn.Module):
    """The exact prediction for x0 ~ N(mu, 0.5^2 I) (test_gpu_dps.py's), written so that autograd passes through:
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


def _gauss_setting(seed=0, n=4, C=3, S=16):
    """mu and images that are draws from the model's own level-0 density, on the host."""
    g = torch.Generator().manual_seed(seed)
    mu = (torch.rand(1, C, S, S, generator=g) - 0.5) * 0.6
    images = (mu + 0.5 * torch.randn(n, C, S, S, generator=g)).clamp(-1, 1).float()
    return mu, images


def _reference(afdm, host, model_cpu, images, steps, method, probes, labels=None):
    """ode_likelihood_reference over the levels of `steps` with host.eps_jacobian_coefficients; model_cpu(x fp64, t (n,))."""
    n = images.shape[0]
    levels = [0] + [u for _, u in host._invert_moves(steps)]
    return afdm.ode_likelihood_reference(lambda x, t: model_cpu(x, torch.full((n,), t, dtype=torch.long)), images, host.alpha_hat, levels,
                                         probes, method, lambda t: host.eps_jacobian_coefficients(t))


@pytest.mark.parametrize("prediction", KINDS)
@pytest.mark.parametrize("method", ["heun", "euler"])
def test_gaussian_model_equals_the_reference_on_the_same_probes(A, method, prediction):
    afdm, dev = A
    mu, images = _gauss_setting()
    diff = afdm.Diffusion(noise_steps=T, img_size=16, device=dev, prediction=prediction)
    host = afdm.Diffusion(noise_steps=T, img_size=16, device="cpu", prediction=prediction)
    model = _GaussModel(mu, diff.alpha_hat, prediction)
    torch.manual_seed(5)
    got = diff.ode_likelihood(model, images, 20, method=method, noise_source="cpu", return_latents=True)
    torch.manual_seed(5)
    probes = (torch.randint(0, 2, (1, 4, 3, 16, 16)) * 2 - 1).float()               # the stated draw
    ref = _reference(afdm, host, _GaussModel(mu, host.alpha_hat, prediction), images, 20, method, probes)
    d = 768
    assert set(got) == {"logp", "bpd", "prior_logp", "trace", "trace_sem", "trace_probes", "latents"}
    for key in ("logp", "bpd", "prior_logp", "trace", "trace_sem"):
        assert got[key].dtype == torch.float64 and got[key].device.type == "cpu" and tuple(got[key].shape) == (4,)
    assert got["latents"].dtype == torch.float32 and got["latents"].device.type == "cuda"
    check(f"likelihood: latents vs reference ({method})", got["latents"].cpu(), ref["latents"], 1e-4, prediction)
    e = float((got["logp"] - ref["logp"]).abs().max())
    note(f"likelihood: |logp - ref| / d, nats ({method}) (absolute)", e / d, prediction)
    assert e <= 1e-4 * d
    te = float(((got["trace"] - ref["trace"]).abs() / ref["trace"].abs()).max())
    note(f"likelihood: trace vs reference, relative ({method}) (absolute)", te, prediction)
    assert te <= 1e-6
    assert float(got["trace_sem"].abs().max()) == 0.0
    want_bpd = -got["logp"] / (d * math.log(2.0)) + math.log2(127.5)
    assert float((got["bpd"] - want_bpd).abs().max()) <= 1e-12
    if method == "euler":                                                           # euler's latents are invert's
        lat = diff.invert(model, images, 20, refine=0)
        assert _same_bits(lat, got["latents"])


def test_heun_at_100_steps_against_the_closed_form(A):
    afdm, dev = A
    mu, images = _gauss_setting(seed=3)
    diff = afdm.Diffusion(noise_steps=T, img_size=16, device=dev)
    model = _GaussModel(mu, diff.alpha_hat)
    torch.manual_seed(1)
    got = diff.ode_likelihood(model, images, 100, noise_source="cpu")
    a0 = float(diff.alpha_hat.detach().cpu().double()[0])
    V = 0.25 * a0 + 1 - a0
    r = images.double() - math.sqrt(a0) * mu.double()
    exact = (-(r * r) / (2 * V) - 0.5 * math.log(2 * math.pi * V)).flatten(1).sum(1)
    err = (got["logp"] - exact) / 768
    print(f"heun S = 100 against the closed form, nats / dim: {err.tolist()}")
    note("likelihood: heun S = 100 vs closed form, nats / dim (absolute)", float(err.abs().max()))
    assert float(err.abs().max()) <= 1e-2


# ---- 4. a non-diagonal Jacobian ------------------------------------------------------------------------------------------------------
class _ConvModel(torch.nn.Module):
    """f(t) Conv2d(3, 3, 3, padding=1)(x), f(t) = 0.5 + t / 1000, in plain torch."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 3, 3, padding=1)

    def forward(self, x, t):
        return (0.5 + t.to(x.dtype) / 1000.0).view(-1, 1, 1, 1) * self.conv(x)


@pytest.mark.parametrize("probe", ["gaussian", "rademacher"])
def test_convolution_model_equals_the_reference_per_probe(A, probe):
    afdm, dev = A
    torch.manual_seed(8)
    cpu_model = _ConvModel().double()
    model = _ConvModel().to(dev)
    model.load_state_dict({k: v.float() for k, v in cpu_model.state_dict().items()})
    cpu_model.load_state_dict({k: v.double() for k, v in model.state_dict().items()})         # the same fp32 weights, widened
    diff = afdm.Diffusion(noise_steps=T, img_size=8, device=dev)
    host = afdm.Diffusion(noise_steps=T, img_size=8, device="cpu")
    images = (torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(2)) * 2 - 1)
    steps = [800, 400, 100, 1]
    torch.manual_seed(6)
    got = diff.ode_likelihood(model, images, steps, probes=3, probe=probe, noise_source="cpu", return_latents=True)
    torch.manual_seed(6)
    probes = torch.randn(3, 2, 3, 8, 8) if probe == "gaussian" else (torch.randint(0, 2, (3, 2, 3, 8, 8)) * 2 - 1).float()
    ref = _reference(afdm, host, cpu_model, images, steps, "heun", probes)
    assert tuple(got["trace_probes"].shape) == (3, 2)
    ratio = float(((got["trace_probes"] - ref["trace_probes"]).abs() / ref["bound_scale"]).max())
    note("likelihood: conv model, per-probe |trace - ref| / sum |weight| |v| |w| (absolute)", ratio, probe)
    assert ratio <= 1e-5
    tol = 1e-5 * float(ref["bound_scale"].max())
    assert float((got["trace"] - ref["trace"]).abs().max()) <= tol
    assert float(ref["trace_sem"].min()) > 0 and float((got["trace_sem"] - ref["trace_sem"]).abs().max()) <= tol
    check("likelihood: conv model latents vs reference", got["latents"].cpu(), ref["latents"], 1e-4, probe)
    assert all(p.requires_grad for p in model.parameters()) and all(p.grad is None for p in model.parameters())


# ---- 5. the UNet (variant 3) ---------------------------------------------------------------------------------------------------------
def _unet(afdm, dev, cls=None, c=1, **kw):
    afdm.set_seed(42)
    return (cls or afdm.UNet)(c_in=c, c_out=c, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


class _Counting(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.forwards, self.backwards = inner, 0, 0

    def _hook(self, grad):
        self.backwards += 1

    def forward(self, x, t):
        self.forwards += 1
        out = self.inner(x, t)
        out.register_hook(self._hook)
        return out


def test_unet_equals_the_loop_on_the_cpu_oracle(A):
    afdm, dev = A
    from oracle import ref_ops as R
    model = _unet(afdm, dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    host = afdm.Diffusion(noise_steps=T, img_size=32, device="cpu")
    images = torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(4)) * 2 - 1
    steps = [700, 300, 1]
    first = next(model.parameters())
    first.requires_grad_(False)                                                     # one flag that was off stays off
    found = [p.requires_grad for p in model.parameters()]
    counting = _Counting(model)
    torch.manual_seed(2)
    got = diff.ode_likelihood(counting, images, steps, noise_source="cpu", return_latents=True)
    assert (counting.forwards, counting.backwards) == (5, 5)                        # (1 + 2 (L - 1)) P for heun over L = 3 moves
    assert [p.requires_grad for p in model.parameters()] == found and all(p.grad is None for p in model.parameters())
    assert counting.training and model._t_range is None
    runs = []
    for _ in range(2):
        torch.manual_seed(2)
        runs.append(diff.ode_likelihood(model, images, steps, noise_source="cpu", return_latents=True))
    assert all(_same_bits(runs[0][k], runs[1][k]) for k in got)                     # the same generator state, the same bits
    assert model.training and model._t_range is None
    counting = _Counting(model)
    diff.ode_likelihood(counting, images, steps, method="euler", probes=2, probe="gaussian")
    assert (counting.forwards, counting.backwards) == (6, 6)                        # L P for euler
    torch.manual_seed(2)
    probes = (torch.randint(0, 2, (1, 2, 1, 32, 32)) * 2 - 1).float()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    oracle = lambda x, t: R.unet_forward(sd, x.float(), t, 3, dict(F_SET)).double()
    ref = _reference(afdm, host, oracle, images, steps, "heun", probes)
    check("likelihood: UNet latents vs the loop on the CPU oracle", got["latents"].cpu(), ref["latents"], 1e-4)
    ratio = float(((got["trace"] - ref["trace"]).abs() / ref["bound_scale"][0]).max())
    note("likelihood: UNet |trace - ref| / sum |weight| |v| |w| (absolute)", ratio)
    assert ratio <= 1e-4
    assert bool(torch.isfinite(got["logp"]).all()) and bool(torch.isfinite(got["bpd"]).all())


def test_labels_reach_a_conditional_unet_and_the_mode_is_left_as_found(A):
    afdm, dev = A
    model = _unet(afdm, dev, num_classes=10)
    model.eval()                                                                    # found in eval mode: stays there
    d6 = afdm.Diffusion(noise_steps=6, img_size=32, device=dev)
    images = torch.rand(2, 1, 32, 32, generator=torch.Generator().manual_seed(4)) * 2 - 1

    def run(labels):
        afdm.set_seed(3)
        return d6.ode_likelihood(model, images, 3, labels=labels, dequantize=True)["logp"]

    a, b, a2 = run(torch.tensor([1, 2])), run(torch.tensor([3, 4])), run(torch.tensor([1, 2]))
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, b) and _same_bits(a, a2)
    assert not model.training and model._t_range is None
    assert all(p.requires_grad for p in model.parameters()) and all(p.grad is None for p in model.parameters())
    with pytest.raises(ValueError, match=r"^Diffusion\.ode_likelihood: "):
        d6.ode_likelihood(_unet(afdm, dev), images, 3, labels=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match="emits 1 channels"):                      # the model's channels against the images'
        d6.ode_likelihood(model, torch.zeros(2, 3, 32, 32), 3)
    with pytest.raises(TypeError):                                                  # classifier-free guidance is not offered
        d6.ode_likelihood(model, images, 3, labels=torch.tensor([1, 2]), cfg_scale=3.0)


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
    assert model.training and model._t_range is None
    with pytest.raises(RuntimeError, match="boom at forward 3"):
        d6.ode_likelihood(model, torch.zeros(2, 1, 32, 32), 4)
    torch.cuda.synchronize()
    assert Boom.calls == 3 and model.training and model._t_range is None
    assert all(p.requires_grad for p in model.parameters()) and all(p.grad is None for p in model.parameters())


def test_basis_probes_give_the_exact_trace_on_the_device(A):
    """d backward passes per evaluation; the Gaussian model's trace is known in closed form: d sqrt(1 - a) / (0.25 a + 1 - a)."""
    afdm, dev = A
    mu, images = _gauss_setting(seed=1, n=2, C=1, S=4)
    diff = afdm.Diffusion(noise_steps=T, img_size=4, device=dev)
    model = _Counting(_GaussModel(mu, diff.alpha_hat))
    state = torch.get_rng_state()
    got = diff.ode_likelihood(model, images, [900, 500, 1], probe="basis", probes=7, noise_source="cpu")
    assert torch.equal(torch.get_rng_state(), state) and model.forwards == 5 * 16  # nothing drawn; `probes` ignored
    ah = diff.alpha_hat.detach().cpu().double()
    levels = [0, 1, 500, 900]
    a = [float(ah[t]) for t in levels]
    sig = [math.sqrt((1 - q) / q) for q in a]
    tr = lambda k: 16 * math.sqrt(1 - a[k]) / (0.25 * a[k] + 1 - a[k])
    want = (sig[1] - sig[0]) * math.sqrt(a[1]) * tr(1)
    for k in (1, 2):
        want += 0.5 * (sig[k + 1] - sig[k]) * (math.sqrt(a[k]) * tr(k) + math.sqrt(a[k + 1]) * tr(k + 1))
    assert float((got["trace"] - want).abs().max()) <= 1e-6 * abs(want)
    assert float(got["trace_sem"].abs().max()) == 0.0 and tuple(got["trace_probes"].shape) == (16, 2)


# ---- 6. from a checkpoint -----------------------------------------------------------------------------------------------------------
def test_likelihood_results_from_a_checkpoint(A, tmp_path):
    afdm, dev = A
    model = _unet(afdm, dev, c=3)
    path = tmp_path / "ckpt.pt"
    torch.save(model.state_dict(), path)
    data = {"args": afdm.argument(image_size=32, image_channels=3, device="cuda", noise_steps=50), "unet_v": 3, "seed": 42,
            "f_settings": dict(F_SET), "modelpath": str(path)}
    pixels = torch.randint(0, 256, (3, 3, 32, 32), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    res = afdm.likelihood_results(data, pixels, n=2, steps=5)
    assert list(res) == ["n", "steps", "method", "probes", "probe", "bpd", "logp", "trace_sem", "bound_bpd"]
    assert (res["n"], res["steps"], res["method"], res["probes"], res["probe"]) == (2, 5, "heun", 1, "rademacher")
    for key in ("bpd", "logp", "trace_sem", "bound_bpd"):
        assert list(res[key]) == ["mean", "std", "values"] and len(res[key]["values"]) == 2
        assert all(math.isfinite(v) for v in res[key]["values"] + [res[key]["mean"], res[key]["std"]])
    assert os.listdir(tmp_path) == ["ckpt.pt"]                                      # no new file beside the checkpoint
    again = afdm.likelihood_results(data, afdm.DeviceDataset(pixels, device=dev), n=2, steps=5)        # a DeviceDataset: the same numbers
    assert again == res
