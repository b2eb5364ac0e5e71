"""GPU tests of DDIM sampling over strided timesteps: the four fused update entry points against a per-operation fp32
restatement (bit for bit) and an fp64 one, the DDPM posterior-mean anchor, DDIM trajectories against a loop on the CPU oracle,
the noise the sampler draws, graph replay, classifier-free guidance, concurrent trajectories, snapshots and argument errors."""
import math

import numpy as np
import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10


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


def _taus(T, S):
    """The timestep subsequence of the issue's definition, restated here."""
    return [T - 1] if S == 1 else [1 + (k * (T - 2)) // (S - 1) for k in range(S)][::-1]


# ---- restatements of the update ----------------------------------------------------------------------------------------
def _f32(v):
    return float(np.float32(v))


def _coef32(ah, t, tp, eta):
    """The per-step scalars in fp32, one IEEE rounding per operation (taken in fp64 and rounded once: exact for + - * / sqrt)."""
    a_t, a_p, eta = float(ah[t]), float(ah[tp]), _f32(eta)
    sq = lambda v: _f32(math.sqrt(v))
    r = _f32(_f32(1 - a_p) / _f32(1 - a_t))
    q = _f32(1 - _f32(a_t / a_p))
    var = _f32(_f32(eta * eta) * _f32(r * q))
    return {"sq1m": sq(_f32(1 - a_t)), "sqat": sq(a_t), "sqap": sq(a_p), "sigma": sq(var),
            "dir": sq(max(_f32(_f32(1 - a_p) - var), 0.0))}


def _lerp_restated(u, c, s):
    """ATen's scalar lerp, one device op per step (as in test_gpu_cfg.py)."""
    d = c - u
    if abs(s) < 0.5:
        return u + d * s
    return c - d * _f32(1 - _f32(s))


def _ddim_restated(x, e, z, ah, t, tp, eta):
    """The update as separate fp32 device ops, each a full-tensor operand (no scalar fast path, e.g. no reciprocal)."""
    k = _coef32(ah, t, tp, eta)
    full = lambda v: torch.full_like(x, v)
    pe = e * full(k["sq1m"])
    x0 = (x - pe) / full(k["sqat"])
    mean = x0 * full(k["sqap"]) + e * full(k["dir"])
    nz = z * full(k["sigma"]) if z is not None else torch.zeros_like(x)
    return mean + nz


def _ddim_f64(x, e, z, ah, t, tp, eta):
    x, e = x.double().cpu().numpy(), e.double().cpu().numpy()
    a_t, a_p = float(ah[t]), float(ah[tp])
    x0 = (x - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
    var = eta * eta * (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
    out = math.sqrt(a_p) * x0 + math.sqrt(max(1 - a_p - var, 0.0)) * e
    if z is not None:
        out = out + math.sqrt(var) * z.double().cpu().numpy()
    return torch.from_numpy(out)


# ---- 1. the four entry points --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("t,tp", [(999, 0), (700, 350), (37, 36), (1, 0)])
def test_ddim_update_equals_restatements(A, form, guided, eta, t, tp):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat.cpu()
    s = 3.0
    g = torch.Generator().manual_seed(7 * t + tp)
    fam = "DDIM: fused update vs fp64 restatement" + (" (guided)" if guided else "")
    for shape in ((4, 3, 8, 8), (3, 3, 5, 7)):                           # 16-byte path and scalar path (n % 4 != 0)
        n = shape[0]
        for with_noise in (False, True):
            x = torch.randn(shape, generator=g).to(dev)
            z = torch.randn(shape, generator=g).to(dev) if with_noise else None
            if guided:
                eps2 = torch.randn((2 * n,) + shape[1:], generator=g).to(dev)
                e = _lerp_restated(eps2[n:], eps2[:n], s)
                e64 = eps2[n:].double() + s * (eps2[:n].double() - eps2[n:].double())
            else:
                e = torch.randn(shape, generator=g).to(dev)
                e64 = e
            want = _ddim_restated(x, e, z, ah, t, tp, eta)
            out2 = torch.full_like(x, float("nan"))
            if form == "host":
                if guided:
                    got = ops.ddim_step_cfg(x, eps2, z, diff.alpha_hat, t, tp, eta, s, out2=out2)
                else:
                    got = ops.ddim_step(x, e, z, diff.alpha_hat, t, tp, eta)
                    out2.copy_(got)
            else:
                t_dev = torch.full((2 * n if guided else n,), t, device=dev, dtype=torch.long)
                tp_dev = torch.full((1,), tp, device=dev, dtype=torch.long)
                got = x.clone()                                          # in place, as the captured sampler step runs it
                if guided:
                    ops.ddim_step_cfg_dev(got, eps2, z, diff.alpha_hat, t_dev, tp_dev, eta, s, got, out2)
                else:
                    ops.ddim_step_dev(got, e, z, diff.alpha_hat, t_dev, tp_dev, eta, got)
                    out2.copy_(got)
            assert _same_bits(got, want), (shape, with_noise)
            assert _same_bits(out2, got)
            # the fp32 expression itself loses bits in q = 1 - a_t / a_p at t = 1 (a_t / a_p = 0.99988): with eta = 1 the
            # error reaches the output through dir, ~5e-7 for a unit-variance eps and ~1.5e-6 for the guided eps at s = 3
            tol = 3e-6 if guided and t == 1 and eta == 1.0 else 1e-6
            check(fam, got.cpu(), _ddim_f64(x, e64, z, ah, t, tp, eta), tol, (form, eta, t, tp, shape, with_noise))
    torch.cuda.synchronize()


def test_ddim_update_checks_its_arguments(A):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    x = torch.zeros(2, 3, 4, 4, device=dev)
    with pytest.raises(afdm.AfdError, match="t_prev < t"):
        ops.ddim_step(x, x, None, diff.alpha_hat, 10, 10, 0.0)
    with pytest.raises(afdm.AfdError, match="t_prev < t"):
        ops.ddim_step(x, x, None, diff.alpha_hat, 1000, 10, 0.0)               # t past the schedule
    with pytest.raises(afdm.AfdError, match="eta"):
        ops.ddim_step_cfg(x, torch.cat([x, x]), None, diff.alpha_hat, 10, 5, -1.0, 3.0)
    with pytest.raises(afdm.AfdError, match="eps2"):
        ops.ddim_step_cfg(x, x, None, diff.alpha_hat, 10, 5, 0.0, 3.0)
    with pytest.raises(afdm.AfdError, match="contiguous"):
        ops.ddim_step(x, x.transpose(2, 3), None, diff.alpha_hat, 10, 5, 0.0)
    with pytest.raises(afdm.AfdError, match="fp32"):
        ops.ddim_step(x, x.double(), None, diff.alpha_hat, 10, 5, 0.0)
    with pytest.raises(afdm.AfdError, match="int64"):
        ops.ddim_step_dev(x, x, None, diff.alpha_hat, torch.zeros(1, device=dev), torch.zeros(1, device=dev, dtype=torch.long), 0.0, x)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_dev: eta"):
        t1 = torch.ones(1, device=dev, dtype=torch.long)
        ops.ddim_step_dev(x, x, None, diff.alpha_hat, t1, t1 - 1, -0.5, x)


# ---- 2. the anchor: one eta = 1 step to t - 1 without noise is the DDPM posterior mean ------------------------------------
@pytest.mark.parametrize("t", [1, 2, 500, 999])
def test_ddim_eta1_single_step_is_the_ddpm_posterior_mean(A, t):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    g = torch.Generator().manual_seed(t)
    x = torch.randn(4, 3, 32, 32, generator=g).to(dev)
    e = torch.randn(4, 3, 32, 32, generator=g).to(dev)
    got = ops.ddim_step(x, e, None, diff.alpha_hat, t, t - 1, 1.0)
    want = ops.denoise_step(x, e, None, diff.alpha, diff.alpha_hat, diff.beta, t)
    err = check("DDIM: eta=1 step t -> t-1 vs the DDPM posterior mean", got, want, 1e-5, t)
    print(f"anchor t={t}: rel-L2 {err:.2e}")


# ---- 3. a trajectory against the CPU oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_trajectory_vs_cpu_oracle_loop(A, eta):
    afdm, dev = A
    from oracle import ref_ops as R
    model = _model(afdm, dev)
    T, n, S = 1000, 2, 10
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    afdm.set_seed(13)
    xf = diff.sample(model, n=n, image_channels=3, noise_source="cpu", return_float=True, steps=S, eta=eta)[2].cpu()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ah = diff.alpha_hat.cpu().double()
    taus = _taus(T, S)
    afdm.set_seed(13)
    x = torch.randn((n, 3, 32, 32))
    with torch.no_grad():
        for t, tp in zip(taus, taus[1:] + [0]):
            e = R.unet_forward(sd, x, torch.full((n,), t, dtype=torch.long), 3, F_SET).double()
            a_t, a_p = float(ah[t]), float(ah[tp])
            var = eta * eta * (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
            x0 = (x.double() - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
            xn = math.sqrt(a_p) * x0 + math.sqrt(max(1 - a_p - var, 0.0)) * e
            if eta > 0 and tp > 0:
                xn = xn + math.sqrt(var) * torch.randn((n, 3, 32, 32)).double()
            x = xn.float()
    err = check("DDIM: 10-step trajectory vs a loop on the CPU oracle (fp64 update)", xf, x, 1e-5, eta)
    print(f"DDIM trajectory (T=1000, S=10, eta={eta}) vs oracle loop: rel-L2 {err:.2e}")


# ---- 4. eta = 0 draws no step noise ----------------------------------------------------------------------------------------
def test_ddim_eta0_draws_no_step_noise(A):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    afdm.set_seed(3)
    diff.sample(model, n=2, image_channels=3, noise_source="device", steps=8, eta=0.0)
    after_sample = torch.randn(64, device=dev)
    afdm.set_seed(3)
    torch.randn((2, 3, 32, 32), device=dev)                              # x_T alone
    after_xT = torch.randn(64, device=dev)
    assert torch.equal(after_sample, after_xT)
    afdm.set_seed(3)                                                     # with eta > 0 the steps do draw
    diff.sample(model, n=2, image_channels=3, noise_source="device", steps=8, eta=0.5)
    assert not torch.equal(torch.randn(64, device=dev), after_xT)


# ---- 5. graph replay equals the eager loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_graph_equals_eager(A, guided, eta):
    afdm, dev = A
    model = _model(afdm, dev, num_classes=K if guided else None)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    kw = {"labels": torch.tensor([1, afdm.NULL_LABEL, 8], device=dev), "cfg_scale": 3.0} if guided else {}
    outs = []
    for use_graph in (False, True):
        afdm.set_seed(5)
        xq, rq, xf = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True, graph=use_graph,
                                 steps=12, eta=eta, **kw)
        outs.append((xq.cpu(), rq.cpu(), xf.cpu(), [s.cpu() for s in diff.last_float_snapshots]))
    assert model.training and model._t_range is None
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert len(outs[0][3]) == len(outs[1][3]) and all(torch.equal(a, b) for a, b in zip(outs[0][3], outs[1][3]))


# ---- 6. the guided sampler is one 2n forward, the lerp and ddim_step per step -------------------------------------------------
def test_ddim_guided_sample_equals_hand_loop(A):
    afdm, dev = A
    from afdm import ops
    model = _model(afdm, dev, num_classes=K)
    T, n, s, eta = 1000, 3, 3.0, 0.5
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    labels = [3, afdm.NULL_LABEL, 7]
    afdm.set_seed(5)
    xq, rq, xf = diff.sample(model, n=n, image_channels=3, noise_source="device", return_float=True, labels=labels, cfg_scale=s,
                             steps=9, eta=eta)
    afdm.set_seed(5)
    y2 = torch.tensor(labels + [afdm.NULL_LABEL] * n, device=dev)
    taus = _taus(T, 9)
    model.eval()
    with torch.no_grad():
        x = torch.randn((n, 3, 32, 32), device=dev)
        for t, tp in zip(taus, taus[1:] + [0]):
            eps2 = model(torch.cat([x, x]), torch.full((2 * n,), t, device=dev, dtype=torch.long), y2)
            e = torch.lerp(eps2[n:], eps2[:n], s)
            note("DDIM: restated lerp vs torch.lerp (guided sampler)", rel_l2(_lerp_restated(eps2[n:], eps2[:n], s), e), t)
            noise = torch.randn_like(x) if tp > 0 else None
            x = ops.ddim_step(x, e, noise, diff.alpha_hat, t, tp, eta)
    model.train()
    assert torch.equal(xf, x) and torch.equal(xq, ops.quantize_u8(x))


# ---- 7. concurrent trajectories ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_ddim_sample_concurrent_streams_and_graph(A, eta):
    afdm, dev = A
    model = _model(afdm, dev)
    T, S = 1000, 8
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    calls = []

    def noise_fn(k, i, shape):
        calls.append((k, i))
        g = torch.Generator().manual_seed(1000 * k + i)
        return torch.randn(shape, generator=g).to(dev)

    outs = []
    for streams, graph in ((2, False), (1, False), (2, True), (1, True)):
        calls.clear()
        outs.append(diff.sample_concurrent(model, n=5, image_channels=3, batch=3, streams=streams, noise_fn=noise_fn, graph=graph,
                                           steps=S, eta=eta))
        torch.cuda.synchronize()
        assert model.training and model._t_range is None
        want_i = {T} | (set(_taus(T, S)[:-1]) if eta > 0 else set())
        assert {i for _, i in calls} == want_i and {k for k, _ in calls} == {0, 1}
    n_snaps = sum(diff.ddim_snapshot(t, tp) for t, tp in zip(_taus(T, S), _taus(T, S)[1:] + [0])) + 1
    assert outs[0][0].shape == (5, 3, 32, 32) and outs[0][1].shape[0] == 5 * n_snaps
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])


# ---- 8. snapshots, and the model state after the loop (also after an exception) ------------------------------------------------
@pytest.mark.parametrize("S", [999, 50, 7])
def test_ddim_snapshot_count(A, S):
    afdm, dev = A
    model = _model(afdm, dev)
    T = 1000
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    taus = _taus(T, S)
    want = sum(tp // 100 < t // 100 for t, tp in zip(taus, taus[1:] + [0])) + 1
    if S == T - 1:
        assert want == 10                                                # the DDPM sampler's nine at i = 900 .. 100 + the final x
    xq, rq = diff.sample(model, n=1, image_channels=3, noise_source="device", steps=S)
    assert len(diff.last_float_snapshots) == want and rq.shape == (want, 3, 32, 32)
    assert torch.equal(rq[-1], xq[0])
    assert model.training and model._t_range is None
    if S == 7:
        r = diff.revert(model, n=1, image_channels=3, steps=S, eta=1.0)
        assert r.shape == (want, 3, 32, 32) and model.training and model._t_range is None


def test_ddim_loop_restores_the_model_after_an_exception(A):
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
        diff.sample(model, n=2, image_channels=3, noise_source="device", steps=10)
    assert Boom.calls == 3 and model.training and model._t_range is None


# ---- 9. argument errors --------------------------------------------------------------------------------------------------------
def test_ddim_sampler_argument_errors(A):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    with pytest.raises(NotImplementedError, match="theta"):
        diff.sample(model, n=1, image_channels=3, theta=45, steps=10)
    with pytest.raises(ValueError, match="eta"):
        diff.sample(model, n=1, image_channels=3, steps=10, eta=-0.5)
    with pytest.raises(ValueError):
        diff.sample(model, n=1, image_channels=3, steps=1000)
    with pytest.raises(ValueError):
        diff.sample(model, n=1, image_channels=3, steps=[500, 999])
    with pytest.raises(NotImplementedError):
        diff.sample_sharded(model, n=2, image_channels=3, steps=10)
    assert model.training and model._t_range is None
    # an explicit sequence is the same chain as its int form
    afdm.set_seed(1)
    a = diff.sample(model, n=1, image_channels=3, noise_source="device", return_float=True, steps=5)[2]
    afdm.set_seed(1)
    b = diff.sample(model, n=1, image_channels=3, noise_source="device", return_float=True, steps=_taus(1000, 5))[2]
    assert torch.equal(a, b)
