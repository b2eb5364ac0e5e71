"""GPU tests of UniPC sampling (orders 1-3): the two fused predictor-corrector entry points against a per-operation fp32
restatement (bit for bit) and an fp64 one, a trajectory against `unipc_reference` on the CPU oracle, S = 1 against DDIM, graph
replay, accuracy on a data set whose probability-flow ODE is solved in closed form, forwards per step, the noise drawn,
snapshots, the model state after an exception, and v-prediction / learned-variance models against a hand loop."""
import math

import numpy as np
import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10
LAYOUTS = ["vec", "odd", "offset", "inplace"]


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


def _lerp_restated(u, c, s):
    """ATen's scalar lerp, one device op per step (as in test_gpu_cfg.py)."""
    d = c - u
    if abs(s) < 0.5:
        return u + d * s
    return c - d * float(np.float32(1 - np.float32(s)))


def _unipc_restated(x, e, xc, h1, h2, h3, c):
    """The three lines as separate fp32 device ops, each a full-tensor operand (no scalar fast path, e.g. no reciprocal)."""
    full = lambda v: torch.full_like(x, float(v))
    m = (x - e * full(c[1])) / full(c[0])
    nc = ((((xc * full(c[2])) + (m * full(c[3]))) + (h1 * full(c[4]))) + (h2 * full(c[5]))) + (h3 * full(c[6]))
    xn = (((nc * full(c[7])) + (m * full(c[8]))) + (h1 * full(c[9]))) + (h2 * full(c[10]))
    return m, nc, xn


def _unipc_f64(x, e, xc, h1, h2, h3, c):
    c = [float(v) for v in c]
    x, e, xc, h1, h2, h3 = (v.double().cpu() for v in (x, e, xc, h1, h2, h3))
    m = (x - c[1] * e) / c[0]
    nc = c[2] * xc + c[3] * m + c[4] * h1 + c[5] * h2 + c[6] * h3
    return m, nc, c[7] * nc + c[8] * m + c[9] * h1 + c[10] * h2


# ---- 1. the two entry points ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_unipc_update_equals_restatements(A, guided, layout):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    table = diff.unipc_coefficients(diff.dpmpp_pairs(20), 3).to(dev)
    s = 3.0
    g = torch.Generator().manual_seed(LAYOUTS.index(layout) * 2 + guided)
    n = 1027 if layout == "odd" else 4 * 3 * 8 * 8
    off = 1 if layout == "offset" else 0                          # every operand 4 bytes past a 16-byte boundary
    fam = "UniPC: fused update vs fp64 restatement" + (" (guided)" if guided else "")

    def buf(count):
        return torch.randn(count + off, generator=g).to(dev)[off:]

    # row 0: no corrector, first order (every history weight 0, slot 0); row 1: second order (c2 = c3 = p2 = 0, slot 1); row 2:
    # slot 2; rows 7 and 9: every weight non-zero, slots 1 and 0
    assert [int(table[k, 11]) for k in (0, 1, 2, 7, 9)] == [0, 1, 2, 1, 0]
    assert table[0, 3:7].tolist() == [0.0] * 4 and table[0, 9:11].tolist() == [0.0] * 2 and bool((table[7:10, 2:11] != 0).all())
    for k in (0, 1, 2, 7, 9):
        c = table[k]
        slot = k % 3
        x, xc, hist = buf(n), buf(n), buf(3 * n).view(3, n)
        h1, h2, h3 = (hist[(slot - j) % 3].clone() for j in (1, 2, 3))
        if guided:
            eps = buf(2 * n)
            e = _lerp_restated(eps[n:], eps[:n], s)
            e64 = eps[n:].double() + s * (eps[:n].double() - eps[n:].double())
        else:
            eps = e = e64 = buf(n)
        want_m, want_xc, want = _unipc_restated(x, e, xc, h1, h2, h3, c)
        m64, xc64, w64 = _unipc_f64(x, e64, xc, h1, h2, h3, c)
        out2 = buf(n).fill_(float("nan"))
        got = x.clone() if layout == "inplace" else buf(n)         # in place: x_out = x, as the sampler runs it
        src = got if layout == "inplace" else x
        if guided:
            ops.unipc_step_cfg(src, eps, xc, hist, c, s, got, out2)
        else:
            ops.unipc_step(src, eps, xc, hist, c, got)
            out2.copy_(got)
        assert _same_bits(got, want), (layout, k)
        assert _same_bits(xc, want_xc), (layout, k)
        assert _same_bits(hist[slot], want_m), (layout, k)
        assert _same_bits(hist[(slot - 1) % 3], h1) and _same_bits(hist[(slot - 2) % 3], h2)       # the other planes are not written
        assert _same_bits(out2, got)
        check(fam, got.cpu(), w64, 1e-6, (layout, k))
        check(fam + ": xc", xc.cpu(), xc64, 1e-6, (layout, k))
        check(fam + ": m", hist[slot].cpu(), m64, 1e-6, (layout, k))
    torch.cuda.synchronize()


def test_unipc_update_clamps_the_slot_and_checks_its_arguments(A):
    afdm, dev = A
    from afdm import ops
    x = torch.zeros(2, 3, 4, 4, device=dev)
    e = torch.ones_like(x)
    c = torch.tensor([1.0, 1.0, 1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0.0], device=dev)
    for slot, plane in ((-3.0, 0), (7.0, 2), (float("nan"), 0)):   # out of range: clamped, never an address outside hist
        c[11] = slot
        xc, hist = torch.zeros_like(x), torch.zeros((3,) + tuple(x.shape), device=dev)
        ops.unipc_step(x, e, xc, hist, c)
        assert [bool((hist[j] == (-1.0 if j == plane else 0.0)).all()) for j in range(3)] == [True] * 3
    c[11] = 0.0
    xc, hist = torch.zeros_like(x), torch.zeros((3,) + tuple(x.shape), device=dev)
    with pytest.raises(afdm.AfdError, match="coef of 12"):
        ops.unipc_step(x, e, xc, hist, torch.ones(5, device=dev))
    with pytest.raises(afdm.AfdError, match="eps2"):
        ops.unipc_step_cfg(x, e, xc, hist, c, 3.0)
    with pytest.raises(afdm.AfdError, match="contiguous"):
        ops.unipc_step(x, e.transpose(2, 3), xc, hist, c)
    with pytest.raises(afdm.AfdError, match="fp32"):
        ops.unipc_step(x, e.double(), xc, hist, c)
    with pytest.raises(afdm.AfdError, match="hist"):
        ops.unipc_step(x, e, xc, hist[:2], c)
    with pytest.raises(afdm.AfdError, match="must not overlap"):
        ops.unipc_step(x, e, x, hist, c)                                        # xc = x
    with pytest.raises(afdm.AfdError, match="must not overlap"):
        ops.unipc_step(x, e, hist[1], hist, c)                                  # xc inside hist


# ---- 2. a trajectory against the CPU oracle ---------------------------------------------------------------------------------
def test_unipc_trajectory_vs_reference_on_the_cpu_oracle(A):
    afdm, dev = A
    from oracle import ref_ops as R
    model = _model(afdm, dev)
    n, S = 2, 10
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    afdm.set_seed(13)
    xf = diff.sample(model, n=n, image_channels=3, noise_source="cpu", return_float=True, steps=S, sampler="unipc_3")[2].cpu()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    afdm.set_seed(13)
    x_T = torch.randn((n, 3, 32, 32))
    want = afdm.unipc_reference(lambda x, t: R.unet_forward(sd, x.float(), t, 3, F_SET), x_T, diff.dpmpp_pairs(S), 3, diff)
    err = check("UniPC-3: 10-step trajectory vs unipc_reference on the CPU oracle", xf, want, 1e-5)
    print(f"UniPC-3 trajectory (T=1000, S=10) vs reference loop: rel-L2 {err:.2e}")


# ---- 3. S = 1 is DDIM with eta = 0 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unipc", "unipc_1", "unipc_3"])
def test_unipc_single_step_is_ddim(A, name):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    out = []
    for kw in ({"steps": 1, "sampler": name}, {"steps": [999]}):
        afdm.set_seed(2)
        out.append(diff.sample(model, n=2, image_channels=3, noise_source="device", return_float=True, **kw)[2])
    check("UniPC: S = 1 vs DDIM eta=0", out[0], out[1], 2e-6, name)


def test_unipc_is_unipc_2(A):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    out = []
    for name in ("unipc", "unipc_2", "unipc_3"):
        afdm.set_seed(2)
        out.append(diff.sample(model, n=1, image_channels=3, noise_source="device", return_float=True, steps=5, sampler=name)[2])
    assert _same_bits(out[0], out[1]) and not _same_bits(out[0], out[2])


# ---- 4. graph replay equals the eager loop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("S", [12, 16])
@pytest.mark.parametrize("order", [2, 3])
def test_unipc_graph_equals_eager(A, guided, S, order):
    afdm, dev = A
    model = _model(afdm, dev, num_classes=K if guided else None)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    kw = {"labels": torch.tensor([1, afdm.NULL_LABEL, 8], device=dev), "cfg_scale": 3.0} if guided else {}
    outs = []
    for use_graph in (False, True):
        afdm.set_seed(5)
        xq, rq, xf = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True, graph=use_graph,
                                 steps=S, sampler=f"unipc_{order}", **kw)
        outs.append((xq.cpu(), rq.cpu(), xf.cpu(), [s.cpu() for s in diff.last_float_snapshots], torch.randn(8, device=dev).cpu()))
    assert model.training and model._t_range is None
    assert bool(torch.isfinite(outs[0][2]).all())
    assert _same_bits(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert len(outs[0][3]) == len(outs[1][3]) and all(_same_bits(a, b) for a, b in zip(outs[0][3], outs[1][3]))
    assert torch.equal(outs[0][4], outs[1][4])                                 # the generator state after the trajectory


# ---- 5. accuracy on Gaussian data, whose probability-flow ODE has a closed-form solution -------------------------------------
class _GaussEps(torch.nn.Module):
    """The exact eps of x0 ~ N(mu, 0.5^2 I): eps(x, t) = sqrt(1 - a)(x - sqrt(a) mu) / (0.25 a + 1 - a), a = alpha_hat[t], in
    fp64 and rounded to fp32 (the model of test_gpu_dpm.py)."""

    def __init__(self, mu, alpha_hat):
        super().__init__()
        self.mu, self.ah = mu, alpha_hat.double()

    def forward(self, x, t):
        a = self.ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (0.25 * a + 1 - a)).float()


def test_unipc_beats_2m_on_the_exact_ode(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat.double()
    g = torch.Generator().manual_seed(0)
    mu = (torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 1.6 - 0.8).to(dev)        # 4096 means in [-0.8, 0.8]
    model = _GaussEps(mu, diff.alpha_hat)
    afdm.set_seed(11)
    xT = torch.randn((1, 4, 32, 32), device=dev).double()
    a0, aT = float(ah[0]), float(ah[999])
    exact = math.sqrt(a0) * mu + math.sqrt(0.25 * a0 + 1 - a0) * (xT - math.sqrt(aT) * mu) / math.sqrt(0.25 * aT + 1 - aT)

    def run(S, sampler):
        afdm.set_seed(11)
        xf = diff.sample(model, n=1, image_channels=4, noise_source="device", return_float=True, steps=S, sampler=sampler)[2]
        err = rel_l2(xf, exact)
        note(f"UniPC: exact-ODE endpoint error, {sampler}", err, f"S = {S}")
        return err

    e2m = {S: run(S, "dpmpp_2m") for S in (20, 40)}
    u2 = {S: run(S, "unipc_2") for S in (20, 40)}
    u3 = {S: run(S, "unipc_3") for S in (16, 20, 40)}
    print(f"exact ODE: 2M {e2m}; UniPC-2 {u2}; UniPC-3 {u3}")
    assert e2m[20] / u3[20] >= 10
    assert e2m[40] / u3[40] >= 10
    assert e2m[20] / u2[20] >= 1.3
    assert e2m[40] / u2[40] >= 2
    assert u3[16] <= e2m[40]


# ---- 6. one forward per step, no noise after x_T, snapshots, the model state after an exception --------------------------------
@pytest.mark.parametrize("guided", [False, True])
def test_unipc_one_forward_per_step(A, guided):
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
    diff.sample(model, n=2, image_channels=3, noise_source="device", steps=9, sampler="unipc_3", **kw)
    assert rows == [4 if guided else 2] * 9


@pytest.mark.parametrize("graph", [False, True])
def test_unipc_draws_nothing_after_x_T(A, graph):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    afdm.set_seed(3)
    diff.sample(model, n=2, image_channels=3, noise_source="device", steps=8, sampler="unipc_3", graph=graph)
    after_sample = torch.randn(64, device=dev)
    afdm.set_seed(3)
    torch.randn((2, 3, 32, 32), device=dev)                              # x_T alone
    assert torch.equal(after_sample, torch.randn(64, device=dev))


@pytest.mark.parametrize("steps", [7, [999, 640, 120, 40, 3]])
def test_unipc_snapshot_count_and_revert(A, steps):
    afdm, dev = A
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    pairs = diff.dpmpp_pairs(steps)
    want = sum(diff.ddim_snapshot(t, tp) for t, tp in pairs) + 1
    afdm.set_seed(4)
    xq, rq = diff.sample(model, n=1, image_channels=3, noise_source="device", steps=steps, sampler="unipc_3")
    assert len(diff.last_float_snapshots) == want and rq.shape == (want, 3, 32, 32)
    assert torch.equal(rq[-1], xq[0])
    assert model.training and model._t_range is None
    for graph in (False, True):
        afdm.set_seed(4)
        r = diff.revert(model, n=1, image_channels=3, noise_source="device", steps=steps, sampler="unipc_3", graph=graph)
        assert r.shape == (want, 3, 32, 32) and torch.equal(r, rq) and model.training and model._t_range is None


def test_unipc_loop_restores_the_model_after_an_exception(A):
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
        diff.sample(model, n=2, image_channels=3, noise_source="device", steps=10, sampler="unipc_3")
    assert Boom.calls == 3 and model.training and model._t_range is None


# ---- 7. v-prediction and learned variances go through predict_eps ----------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v", "learned"])
def test_unipc_on_other_model_kinds_equals_a_hand_loop(A, kind):
    afdm, dev = A
    from afdm import ops
    learned = kind == "learned"
    model = _model(afdm, dev, c_out=6 if learned else 3)
    kw = {"variance": "learned"} if learned else {"prediction": "v"}
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **kw)
    n, S = 2, 4
    afdm.set_seed(6)
    xf = diff.sample(model, n=n, image_channels=3, noise_source="device", return_float=True, steps=S, sampler="unipc_3")[2]
    afdm.set_seed(6)
    pairs = diff.dpmpp_pairs(S)
    table = diff.unipc_coefficients(pairs, 3).to(dev)
    model.eval()
    with torch.no_grad():
        x = torch.randn((n, 3, 32, 32), device=dev)
        xc, hist = x.clone(), torch.zeros((3,) + tuple(x.shape), device=dev)
        for k, (t, _) in enumerate(pairs):
            eps = diff.predict_eps(model, x, torch.full((n,), t, device=dev, dtype=torch.long))
            x = ops.unipc_step(x, eps, xc, hist, table[k])
    model.train()
    assert bool(torch.isfinite(xf).all()) and _same_bits(xf, x)
