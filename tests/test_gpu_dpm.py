"""GPU tests of DPM-Solver++(2M) sampling: the two fused update entry points against a per-operation fp32 restatement (bit for
bit) and an fp64 one, the first-order step against DDIM, convergence on a data set whose probability-flow ODE is solved in
closed form, a trajectory against a loop on the CPU oracle, graph replay, guidance, the noise drawn, forwards per step,
snapshots and the model state after an exception."""
import math

import numpy as np
import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10
DPM = "dpmpp_2m"


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42, num_classes=None):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _lerp_restated(u, c, s):
    """ATen's scalar lerp, one device op per step (as in test_gpu_cfg.py)."""
    d = c - u
    if abs(s) < 0.5:
        return u + d * s
    return c - d * float(np.float32(1 - np.float32(s)))


def _dpm_restated(x, e, xp, c):
    """The update as separate fp32 device ops, each a full-tensor operand (no scalar fast path, e.g. no reciprocal)."""
    full = lambda v: torch.full_like(x, float(v))
    x0 = (x - e * full(c[1])) / full(c[0])
    m = x * full(c[2]) + x0 * full(c[3])
    p = xp * full(c[4]) if xp is not None else torch.zeros_like(x)
    return m + p, x0


def _dpm_f64(x, e, xp, c):
    c = [float(v) for v in c]
    x, e = x.double().cpu(), e.double().cpu()
    x0 = (x - c[1] * e) / c[0]
    out = c[2] * x + c[3] * x0
    if xp is not None:
        out = out + c[4] * xp.double().cpu()
    return out, x0


# ---- 1. the two entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("layout", ["vec", "odd", "offset", "inplace"])
@pytest.mark.parametrize("has_prev", [False, True])
def test_dpmpp_update_equals_restatements(A, guided, layout, has_prev):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    table = diff.dpmpp_coefficients(diff.dpmpp_pairs(20)).to(dev)
    s = 3.0
    g = torch.Generator().manual_seed(["vec", "odd", "offset", "inplace"].index(layout) * 4 + 2 * guided + has_prev)
    n = 3 * 5 * 7 if layout == "odd" else 4 * 3 * 8 * 8
    off = 1 if layout == "offset" else 0                          # every operand 4 bytes past a 16-byte boundary
    fam = "DPM++: fused update vs fp64 restatement" + (" (guided)" if guided else "")

    def buf(count):
        return torch.randn(count + off, generator=g).to(dev)[off:]

    for k in (0, 7, 19):
        c = table[k]
        x = buf(n)
        xp = buf(n) if has_prev else None
        if guided:
            eps = buf(2 * n)
            e = _lerp_restated(eps[n:], eps[:n], s)
            e64 = eps[n:].double() + s * (eps[:n].double() - eps[n:].double())
        else:
            eps = e = e64 = buf(n)
        want, want_x0 = _dpm_restated(x, e, xp, c)
        out2 = buf(n).fill_(float("nan"))
        if layout == "inplace":                                   # x_out = x and x0_out = x0_prev, as the sampler runs it
            got = x.clone()
            got_x0 = xp.clone() if has_prev else buf(n)
            prev = got_x0 if has_prev else None
            if guided:
                ops.dpmpp_step_cfg(got, eps, prev, c, s, got, out2, got_x0)
            else:
                ops.dpmpp_step(got, eps, prev, c, got, got_x0)
                out2.copy_(got)
        else:
            got, got_x0 = buf(n), buf(n)
            if guided:
                ops.dpmpp_step_cfg(x, eps, xp, c, s, got, out2, got_x0)
            else:
                ops.dpmpp_step(x, eps, xp, c, got, got_x0)
                out2.copy_(got)
        assert _same_bits(got, want), (layout, k)
        assert _same_bits(got_x0, want_x0), (layout, k)
        assert _same_bits(out2, got)
        w64, x064 = _dpm_f64(x, e64, xp, c)
        check(fam, got.cpu(), w64, 1e-6, (layout, has_prev, k))
        check(fam + ": x0", got_x0.cpu(), x064, 1e-6, (layout, has_prev, k))
    torch.cuda.synchronize()


def test_dpmpp_update_checks_its_arguments(A):
    afdm, dev = A
    from afdm import ops
    x = torch.zeros(2, 3, 4, 4, device=dev)
    c = torch.ones(5, device=dev)
    x0 = torch.zeros_like(x)
    with pytest.raises(afdm.AfdError, match="coef of 5"):
        ops.dpmpp_step(x, x, None, torch.ones(4, device=dev), None, x0)
    with pytest.raises(afdm.AfdError, match="eps2"):
        ops.dpmpp_step_cfg(x, x, None, c, 3.0, None, None, x0)
    with pytest.raises(afdm.AfdError, match="contiguous"):
        ops.dpmpp_step(x, x.transpose(2, 3), None, c)
    with pytest.raises(afdm.AfdError, match="fp32"):
        ops.dpmpp_step(x, x.double(), None, c)
    with pytest.raises(afdm.AfdError, match="x0_out"):
        ops.dpmpp_step(x, x, None, c, None, torch.zeros(5, device=dev))
    with pytest.raises(afdm.AfdError, match="x0_out must not overlap"):
        ops.dpmpp_step(x, x.clone(), None, c, None, x)                        # x0_out = x
    with pytest.raises(afdm.AfdError, match="x0_out must not overlap"):
        big = torch.zeros(2 * x.numel(), device=dev)
        ops.dpmpp_step(x, x.clone(), big[:x.numel()].view_as(x), c, None, big[4:4 + x.numel()].view_as(x))


# ---- 2. a first-order step is DDIM with eta = 0 ---------------------------------------------------------------------------
@pytest.mark.parametrize("t,tp", [(999, 891), (500, 250), (95, 32), (8, 1), (1, 0)])
def test_dpmpp_first_order_step_is_ddim(A, t, tp):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    row = diff.dpmpp_coefficients([(t, tp)]).to(dev)[0]
    assert float(row[4]) == 0.0
    g = torch.Generator().manual_seed(t)
    x = torch.randn(4, 3, 32, 32, generator=g).to(dev)
    e = torch.randn(4, 3, 32, 32, generator=g).to(dev)
    got = ops.dpmpp_step(x, e, None, row)[0]
    want = ops.ddim_step(x, e, None, diff.alpha_hat, t, tp, 0.0)
    check("DPM++: order-1 step vs DDIM eta=0", got, want, 2e-6, (t, tp))


# ---- 3. convergence on Gaussian data, whose probability-flow ODE has a closed-form solution -------------------------------
class _GaussEps(torch.nn.Module):
    """The exact eps of x0 ~ N(mu, 0.5^2 I): eps(x, t) = sqrt(1 - a)(x - sqrt(a) mu) / (0.25 a + 1 - a), a = alpha_hat[t], in
    fp64 and rounded to fp32."""

    def __init__(self, mu, alpha_hat):
        super().__init__()
        self.mu, self.ah = mu, alpha_hat.double()

    def forward(self, x, t):
        a = self.ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (0.25 * a + 1 - a)).float()


def test_dpmpp_converges_on_the_exact_ode(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat.double()
    g = torch.Generator().manual_seed(0)
    mu = (torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 1.6 - 0.8).to(dev)        # 4096 means in [-0.8, 0.8]
    model = _GaussEps(mu, diff.alpha_hat)

    def run(**kw):
        afdm.set_seed(11)
        xf = diff.sample(model, n=1, image_channels=4, noise_source="device", return_float=True, **kw)[2]
        afdm.set_seed(11)
        xT = torch.randn((1, 4, 32, 32), device=dev).double()
        a0, aT = float(ah[0]), float(ah[999])
        exact = math.sqrt(a0) * mu + math.sqrt(0.25 * a0 + 1 - a0) * (xT - math.sqrt(aT) * mu) / math.sqrt(0.25 * aT + 1 - aT)
        return rel_l2(xf, exact)

    e20, e40 = run(steps=20, sampler=DPM), run(steps=40, sampler=DPM)
    d20 = run(steps=diff.logsnr_timesteps(20))                                # DDIM, eta = 0, on the same timesteps
    note("DPM++: exact-ODE endpoint error at S = 20", e20)
    print(f"exact ODE: DPM++ S=20 {e20:.3e}, S=40 {e40:.3e}; DDIM on the same S=20 steps {d20:.3e}")
    assert e20 < 1.5e-2
    assert d20 >= 5 * e20
    assert e20 / e40 >= 3


# ---- 4. a trajectory against the CPU oracle ---------------------------------------------------------------------------------
def test_dpmpp_trajectory_vs_cpu_oracle_loop(A):
    afdm, dev = A
    from oracle import ref_ops as R
    model = _model(afdm, dev)
    T, n, S = 1000, 2, 10
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    afdm.set_seed(13)
    xf = diff.sample(model, n=n, image_channels=3, noise_source="cpu", return_float=True, steps=S, sampler=DPM)[2].cpu()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ah = diff.alpha_hat.cpu().double()
    alpha = lambda t: math.sqrt(float(ah[t]))
    sigma = lambda t: math.sqrt(1 - float(ah[t]))
    lam = lambda t: math.log(alpha(t) / sigma(t))
    taus = diff.logsnr_timesteps(S)
    afdm.set_seed(13)
    x = torch.randn((n, 3, 32, 32)).double()
    x0_prev, h_prev = None, None
    with torch.no_grad():
        for k, (t, tp) in enumerate(zip(taus, taus[1:] + [0])):
            e = R.unet_forward(sd, x.float(), torch.full((n,), t, dtype=torch.long), 3, F_SET).double()
            x0 = (x - sigma(t) * e) / alpha(t)
            h = lam(tp) - lam(t)
            B = -alpha(tp) * math.expm1(-h)
            x = sigma(tp) / sigma(t) * x
            if k == 0 or k == S - 1:                                           # S < 15: the last step is first order too
                x = x + B * x0
            else:
                r = h_prev / h
                x = x + B * (1 + 1 / (2 * r)) * x0 - B / (2 * r) * x0_prev
            x0_prev, h_prev = x0, h
    err = check("DPM++: 10-step trajectory vs a loop on the CPU oracle (fp64 update)", xf, x, 1e-5)
    print(f"DPM++ trajectory (T=1000, S=10) vs oracle loop: rel-L2 {err:.2e}")


# ---- 5. S = 1 and 2 are DDIM with eta = 0 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2])
def test_dpmpp_short_chains_are_ddim(A, S):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    out = []
    for kw in ({"steps": S, "sampler": DPM}, {"steps": diff.logsnr_timesteps(S)}):
        afdm.set_seed(2)
        out.append(diff.sample(model, n=2, image_channels=3, noise_source="device", return_float=True, **kw)[2])
    check("DPM++: S = 1, 2 vs DDIM eta=0", out[0], out[1], 2e-6, S)


# ---- 6. graph replay equals the eager loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("S", [12, 16])
def test_dpmpp_graph_equals_eager(A, guided, S):
    afdm, dev = A
    model = _model(afdm, dev, num_classes=K if guided else None)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    kw = {"labels": torch.tensor([1, afdm.NULL_LABEL, 8], device=dev), "cfg_scale": 3.0} if guided else {}
    outs = []
    for use_graph in (False, True):
        afdm.set_seed(5)
        xq, rq, xf = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True, graph=use_graph,
                                 steps=S, sampler=DPM, **kw)
        outs.append((xq.cpu(), rq.cpu(), xf.cpu(), [s.cpu() for s in diff.last_float_snapshots], torch.randn(8, device=dev).cpu()))
    assert model.training and model._t_range is None
    assert _same_bits(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert len(outs[0][3]) == len(outs[1][3]) and all(_same_bits(a, b) for a, b in zip(outs[0][3], outs[1][3]))
    assert torch.equal(outs[0][4], outs[1][4])                                 # the generator state after the trajectory


# ---- 7. the guided sampler is one 2n forward, the lerp and dpmpp_step per step ------------------------------------------------
def test_dpmpp_guided_sample_equals_hand_loop(A):
    afdm, dev = A
    from afdm import ops
    model = _model(afdm, dev, num_classes=K)
    T, n, s, S = 1000, 3, 3.0, 16
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    labels = [3, afdm.NULL_LABEL, 7]
    afdm.set_seed(5)
    xq, rq, xf = diff.sample(model, n=n, image_channels=3, noise_source="device", return_float=True, labels=labels, cfg_scale=s,
                             steps=S, sampler=DPM)
    afdm.set_seed(5)
    y2 = torch.tensor(labels + [afdm.NULL_LABEL] * n, device=dev)
    pairs = diff.dpmpp_pairs(S)
    table = diff.dpmpp_coefficients(pairs).to(dev)
    model.eval()
    with torch.no_grad():
        x = torch.randn((n, 3, 32, 32), device=dev)
        x0 = torch.zeros_like(x)
        for k, (t, tp) in enumerate(pairs):
            eps2 = model(torch.cat([x, x]), torch.full((2 * n,), t, device=dev, dtype=torch.long), y2)
            e = torch.lerp(eps2[n:], eps2[:n], s)
            note("DPM++: restated lerp vs torch.lerp (guided sampler)", rel_l2(_lerp_restated(eps2[n:], eps2[:n], s), e), t)
            second = k > 0 and (k < S - 1 or S >= 15)                  # S = 16: only the first step is first order
            x = ops.dpmpp_step(x, e, x0 if second else None, table[k], x0_out=x0)[0]
    model.train()
    assert _same_bits(xf, x) and torch.equal(xq, ops.quantize_u8(x))


# ---- 8. no noise after x_T, one forward per step, snapshots, the model state after an exception --------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_dpmpp_draws_nothing_after_x_T(A, graph):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    afdm.set_seed(3)
    diff.sample(model, n=2, image_channels=3, noise_source="device", steps=8, sampler=DPM, graph=graph)
    after_sample = torch.randn(64, device=dev)
    afdm.set_seed(3)
    torch.randn((2, 3, 32, 32), device=dev)                              # x_T alone
    assert torch.equal(after_sample, torch.randn(64, device=dev))


@pytest.mark.parametrize("guided", [False, True])
def test_dpmpp_one_forward_per_step(A, guided):
    afdm, dev = A
    rows = []

    class Counting(afdm.UNet):
        def forward(self, x, *a, **kw):
            rows.append(x.shape[0])
            return super().forward(x, *a, **kw)

    afdm.set_seed(42)
    kw = {"num_classes": K} if guided else {}
    model = Counting(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    kw = {"labels": [1, 2], "cfg_scale": 2.0} if guided else {}
    diff.sample(model, n=2, image_channels=3, noise_source="device", steps=9, sampler=DPM, **kw)
    assert rows == [4 if guided else 2] * 9


@pytest.mark.parametrize("steps", [50, 7, [999, 640, 120, 40, 3]])
def test_dpmpp_snapshot_count(A, steps):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    pairs = diff.dpmpp_pairs(steps)
    want = sum(tp // 100 < t // 100 for t, tp in pairs) + 1
    xq, rq = diff.sample(model, n=1, image_channels=3, noise_source="device", steps=steps, sampler=DPM)
    assert len(diff.last_float_snapshots) == want and rq.shape == (want, 3, 32, 32)
    assert torch.equal(rq[-1], xq[0])
    assert model.training and model._t_range is None
    if steps == 7:
        r = diff.revert(model, n=1, image_channels=3, steps=steps, sampler=DPM, graph=True)
        assert r.shape == (want, 3, 32, 32) and model.training and model._t_range is None


def test_dpmpp_loop_restores_the_model_after_an_exception(A):
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
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    with pytest.raises(RuntimeError, match="third step"):
        diff.sample(model, n=2, image_channels=3, noise_source="device", steps=10, sampler=DPM)
    assert Boom.calls == 3 and model.training and model._t_range is None
