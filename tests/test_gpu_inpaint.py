"""GPU tests of inpainting (RePaint): the eight masked update entry points and afd_renoise bit for bit against restatements,
inpaint == sample under an all-zero mask, the known region under an all-one mask, graph replay, the forward count, an analytic
two-image model on which the mask must condition the result, and the model's state after an exception."""
import math

import numpy as np
import pytest
import torch

from conftest import check

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


def _f32(v):
    return float(np.float32(v))


def _slot(shape, dev, g, offset):
    """A standard-normal tensor of `shape`; offset > 0 places it `offset` elements into a larger buffer (unaligned)."""
    n = int(np.prod(shape))
    buf = torch.randn(n + offset, generator=g).to(dev)
    return buf[offset:].view(shape)


# ---- 1. the masked entry points and renoise, bit for bit ---------------------------------------------------------------------
def _masked_restated(ops, diff, kind, guided, x, e, z, x0, m, t, tp, eta, s):
    """gen: the unmasked entry point; known: ops.noise_images(x0, full(t_prev), z), or x0 at t_prev == 0."""
    n = x.shape[0]
    gz = None if tp == 0 or (kind == "ddim" and eta == 0) else z
    if kind == "ddpm":
        gen = (ops.denoise_step_cfg(x, e, gz, diff.alpha, diff.alpha_hat, diff.beta, t, s) if guided
               else ops.denoise_step(x, e, gz, diff.alpha, diff.alpha_hat, diff.beta, t))
    else:
        gen = (ops.ddim_step_cfg(x, e, gz, diff.alpha_hat, t, tp, eta, s) if guided
               else ops.ddim_step(x, e, gz, diff.alpha_hat, t, tp, eta))
    if tp == 0:
        known = x0
    else:
        known = ops.noise_images(x0.contiguous(), z.contiguous(), torch.full((n,), tp, dtype=torch.long, device=x.device),
                                 diff.alpha_hat)
    return torch.where(m.bool(), known, gen)


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("kind,eta,t,tp", [("ddpm", 0.0, 999, 998), ("ddpm", 0.0, 37, 36), ("ddpm", 0.0, 1, 0),
                                           ("ddim", 0.0, 700, 350), ("ddim", 1.0, 700, 350), ("ddim", 0.5, 37, 36),
                                           ("ddim", 1.0, 20, 0), ("ddim", 0.0, 1, 0)])
def test_masked_update_equals_restatement(A, form, guided, kind, eta, t, tp):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    s = 3.0
    g = torch.Generator().manual_seed(7 * t + tp + (1 if guided else 0))
    for shape, off in (((4, 3, 8, 8), 0), ((3, 3, 5, 7), 0), ((4, 3, 8, 8), 1)):    # 16-byte path, odd n, unaligned
        n = shape[0]
        x = _slot(shape, dev, g, off)
        e = _slot((2 * n,) + shape[1:] if guided else shape, dev, g, off)
        z = _slot(shape, dev, g, off)
        x0 = _slot(shape, dev, g, off)
        mfull = (torch.rand(shape, generator=g) < 0.5).to(torch.uint8)
        m = torch.zeros(mfull.numel() + off, dtype=torch.uint8, device=dev)[off:].view(shape)
        m.copy_(mfull.to(dev))
        with_noise = [True] if tp > 0 else [False, True]          # the noise may be NULL only at t_prev == 0 (host forms)
        for use_z in with_noise:
            zz = z if use_z else None
            if form == "dev" and zz is None:
                continue
            want = _masked_restated(ops, diff, kind, guided, x, e, z, x0, m, t, tp, eta, s)
            out2 = torch.full_like(x, float("nan"))
            if form == "host":
                if kind == "ddpm":
                    got = (ops.denoise_step_masked_cfg(x, e, zz, x0, m, diff.alpha, diff.alpha_hat, diff.beta, t, s, out2=out2)
                           if guided else ops.denoise_step_masked(x, e, zz, x0, m, diff.alpha, diff.alpha_hat, diff.beta, t))
                else:
                    got = (ops.ddim_step_masked_cfg(x, e, zz, x0, m, diff.alpha_hat, t, tp, eta, s, out2=out2)
                           if guided else ops.ddim_step_masked(x, e, zz, x0, m, diff.alpha_hat, t, tp, eta))
                if not guided:
                    out2.copy_(got)
            else:
                t_dev = torch.full((2 * n if guided else n,), t, device=dev, dtype=torch.long)
                tp_dev = torch.full((1,), tp, device=dev, dtype=torch.long)
                got = x.clone()                                           # in place, as the captured sampler step runs it
                if kind == "ddpm":
                    if guided:
                        ops.denoise_step_masked_cfg_dev(got, e, zz, x0, m, diff.alpha, diff.alpha_hat, diff.beta, t_dev, s, got, out2)
                    else:
                        ops.denoise_step_masked_dev(got, e, zz, x0, m, diff.alpha, diff.alpha_hat, diff.beta, t_dev, got)
                else:
                    if guided:
                        ops.ddim_step_masked_cfg_dev(got, e, zz, x0, m, diff.alpha_hat, t_dev, tp_dev, eta, s, got, out2)
                    else:
                        ops.ddim_step_masked_dev(got, e, zz, x0, m, diff.alpha_hat, t_dev, tp_dev, eta, got)
                if not guided:
                    out2.copy_(got)
            assert _same_bits(got, want), (shape, off, use_z)
            assert _same_bits(out2, got)
            assert 0 < int(m.sum()) < m.numel()
    torch.cuda.synchronize()


@pytest.mark.parametrize("t_from,t_to", [(0, 1), (1, 11), (36, 37), (240, 999), (500, 998)])
def test_renoise_equals_restatements(A, t_from, t_to):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat.cpu()
    a = _f32(float(ah[t_to]) / float(ah[t_from]))
    sa, sb = _f32(math.sqrt(a)), _f32(math.sqrt(_f32(1 - a)))
    g = torch.Generator().manual_seed(t_from + 1000 * t_to)
    for shape, off in (((4, 3, 8, 8), 0), ((3, 3, 5, 7), 0), ((4, 3, 8, 8), 3)):
        x, z = _slot(shape, dev, g, off), _slot(shape, dev, g, off)
        want = x * torch.full_like(x, sa) + z * torch.full_like(x, sb)
        got = ops.renoise(x, z, diff.alpha_hat, t_from, t_to)
        assert _same_bits(got, want), (shape, off)
        inplace = x.clone()
        ops.renoise(inplace, z, diff.alpha_hat, t_from, t_to, out=inplace)
        assert _same_bits(inplace, want)
        a64 = float(ah[t_to]) / float(ah[t_from])
        ref = math.sqrt(a64) * x.double().cpu() + math.sqrt(1 - a64) * z.double().cpu()
        check("inpaint: renoise vs fp64", got.cpu(), ref, 1e-6, (t_from, t_to, shape, off))
    with pytest.raises(afdm.AfdError, match="t_from < t_to"):
        ops.renoise(x, z, diff.alpha_hat, 5, 5)
    with pytest.raises(afdm.AfdError, match="t_from < t_to"):
        ops.renoise(x, z, diff.alpha_hat, 5, 1000)


def test_masked_update_checks_its_arguments(A):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    x = torch.zeros(2, 3, 4, 4, device=dev)
    m = torch.ones(2, 3, 4, 4, device=dev, dtype=torch.uint8)
    with pytest.raises(afdm.AfdError, match="mask must be"):
        ops.ddim_step_masked(x, x, x, x.clone(), m.float(), diff.alpha_hat, 10, 5, 0.0)
    with pytest.raises(afdm.AfdError, match="mask must be"):
        ops.denoise_step_masked(x, x, x, x.clone(), m[:1], diff.alpha, diff.alpha_hat, diff.beta, 10)
    with pytest.raises(afdm.AfdError, match="x0 must be"):
        ops.denoise_step_masked(x, x, x, x[:1], m, diff.alpha, diff.alpha_hat, diff.beta, 10)
    with pytest.raises(afdm.AfdError, match="noise must not be NULL"):
        ops.ddim_step_masked(x, x, None, x.clone(), m, diff.alpha_hat, 10, 5, 0.0)
    with pytest.raises(afdm.AfdError, match="must not overlap"):
        ops.ddim_step_masked(x, x, x, x, m, diff.alpha_hat, 10, 5, 0.0, out=x)
    with pytest.raises(afdm.AfdError, match="t_prev < t"):
        ops.ddim_step_masked(x, x, x, x.clone(), m, diff.alpha_hat, 10, 10, 0.0)


# ---- 2. an all-zero mask is `sample`, bit for bit ---------------------------------------------------------------------------
def _run(diff, fn, seed, **kw):
    import afdm
    afdm.set_seed(seed)
    xq, rq, xf = fn(return_float=True, **kw)
    snaps = [s.cpu() for s in diff.last_float_snapshots]
    after = torch.randn(4, device=xf.device).cpu()           # where the device generator stands afterwards
    return xq.cpu(), rq.cpu(), xf.cpu(), snaps, after


@pytest.mark.parametrize("cfg", ["ddpm", "ddpm-graph", "ddim0", "ddim1", "ddim1-graph", "ddim0-graph", "ddpm-guided",
                                 "ddim1-guided-graph"])
def test_all_zero_mask_is_sample(A, cfg):
    afdm, dev = A
    guided = "guided" in cfg
    model = _model(afdm, dev, num_classes=K if guided else None)
    T = 1000 if cfg.startswith("ddim") else 130
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    n = 3
    kw = {"graph": "graph" in cfg}
    if cfg.startswith("ddim"):
        kw.update(steps=12, eta=float(cfg[4]))
    if guided:
        kw.update(labels=torch.tensor([1, afdm.NULL_LABEL, 8], device=dev), cfg_scale=3.0)
    images = torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
    s = _run(diff, lambda **k: diff.sample(model, n=n, image_channels=3, **k), 9, **kw)
    p = _run(diff, lambda **k: diff.inpaint(model, images, torch.zeros(1, 1, 32, 32), **k), 9, **kw)
    assert torch.equal(s[0], p[0]) and torch.equal(s[1], p[1]) and _same_bits(s[2], p[2])
    assert len(s[3]) == len(p[3]) >= 2 and all(_same_bits(a, b) for a, b in zip(s[3], p[3]))
    if not cfg.startswith("ddim0"):
        assert torch.equal(s[4], p[4])                        # the same noise stream consumed
    assert model.training and model._t_range is None


# ---- 3. an all-one mask: the known region is images noised to each level, and images at the end --------------------------
@pytest.mark.parametrize("steps,eta,jumps", [(None, 0.0, 1), (20, 0.5, 3)])
def test_all_one_mask_keeps_the_images(A, steps, eta, jumps):
    afdm, dev = A
    from afdm import ops
    model = _model(afdm, dev)
    T = 250 if steps is None else 1000
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    n, shape = 2, (2, 3, 32, 32)
    images = torch.rand(shape, generator=torch.Generator().manual_seed(2)) * 2 - 1
    afdm.set_seed(4)
    xq, rq, xf = diff.inpaint(model, images, torch.ones(1), steps=steps, eta=eta, jump_length=2, jump_n_sample=jumps,
                              noise_source="cpu", return_float=True)
    snaps = diff.last_float_snapshots
    assert _same_bits(xf.cpu(), images) and _same_bits(snaps[-1].cpu(), images)
    # replay the CPU generator: x_T, then one draw per up-move and per down-move with t_prev > 0
    chain = list(range(T - 1, 0, -1)) if steps is None else diff.ddim_timesteps(steps)
    afdm.set_seed(4)
    torch.randn(shape)
    x0 = images.to(dev)
    want = []
    for t, tp in diff.repaint_moves(chain, 2, jumps):
        if tp > t:
            torch.randn(shape)
            continue
        if tp > 0:
            z = torch.randn(shape).to(dev)
            known = ops.noise_images(x0, z, torch.full((n,), tp, dtype=torch.long, device=dev), diff.alpha_hat)
        else:
            known = x0
        if diff.ddim_snapshot(t, tp):
            want.append(known.cpu())
    assert len(want) == len(snaps) - 1 >= 2
    assert all(_same_bits(a.cpu(), b) for a, b in zip(snaps, want))


# ---- 4. graph replay equals the eager loop, with and without jumps ----------------------------------------------------------
@pytest.mark.parametrize("cfg", ["ddpm", "ddim1-guided", "ddim0"])
@pytest.mark.parametrize("jumps", [1, 3])
def test_inpaint_graph_equals_eager(A, cfg, jumps):
    afdm, dev = A
    guided = "guided" in cfg
    model = _model(afdm, dev, num_classes=K if guided else None)
    T = 30 if cfg == "ddpm" else 1000
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    kw = {"jump_length": 2, "jump_n_sample": jumps, "noise_source": "device"}
    if cfg.startswith("ddim"):
        kw.update(steps=8, eta=float(cfg[4]))
    if guided:
        kw.update(labels=torch.tensor([1, 8], device=dev), cfg_scale=3.0)
    images = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1
    mask = torch.zeros(2, 1, 32, 32)
    mask[:, :, :, :16] = 1
    outs = [_run(diff, lambda **k: diff.inpaint(model, images, mask, **k), 11, graph=g, **kw) for g in (False, True)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and _same_bits(outs[0][2], outs[1][2])
    assert len(outs[0][3]) == len(outs[1][3]) and all(_same_bits(a, b) for a, b in zip(outs[0][3], outs[1][3]))
    assert torch.equal(outs[0][4], outs[1][4])
    known = mask.bool().expand(2, 3, 32, 32)
    assert _same_bits(outs[0][2][known], images[known])
    assert model.training and model._t_range is None


# ---- 5. one forward per down-move -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,jumps", [(10, 1), (10, 3), (None, 2)])
def test_inpaint_forward_count(A, steps, jumps):
    afdm, dev = A
    inner = _model(afdm, dev)

    class Counting(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inner, self.calls = inner, 0

        def forward(self, *a):
            self.calls += 1
            return self.inner(*a)

    model = Counting()
    T = 40 if steps is None else 1000
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    images = torch.zeros(2, 3, 32, 32)
    diff.inpaint(model, images, torch.ones(1, 1, 1, 32), steps=steps, jump_length=3, jump_n_sample=jumps)
    chain = list(range(T - 1, 0, -1)) if steps is None else diff.ddim_timesteps(steps)
    down = [m for m in diff.repaint_moves(chain, 3, jumps) if m[0] > m[1]]
    assert model.calls == len(down)
    if jumps == 1:
        assert model.calls == len(chain)
    else:
        assert model.calls > len(chain)


# ---- 6. conditioning works: the exact denoiser of a two-image data set -------------------------------------------------------
class TwoImages(torch.nn.Module):
    """eps(x_t, t) = (x_t - sqrt(ah_t) E[x0 | x_t]) / sqrt(1 - ah_t) for data that are x_a or x_b with equal weight: the
    posterior weights are the softmax of the two Gaussian log-likelihoods -|x_t - sqrt(ah_t) x_k|^2 / (2 (1 - ah_t))."""

    def __init__(self, xa, xb, alpha_hat):
        super().__init__()
        self.xs = torch.stack([xa, xb]).double()                 # (2, C, H, W)
        self.ah = alpha_hat.double()

    def forward(self, x, t):
        ah = self.ah[t].view(-1, 1, 1, 1)
        xd = x.double()
        d = xd[:, None] - ah.sqrt()[:, None] * self.xs[None]      # (n, 2, C, H, W)
        logp = -(d * d).flatten(2).sum(-1) / (2 * (1 - ah.view(-1, 1)))
        w = torch.softmax(logp, dim=1)
        ex0 = (w[:, :, None, None, None] * self.xs[None]).sum(1)
        return ((xd - ah.sqrt() * ex0) / (1 - ah).sqrt()).float()


def test_inpaint_conditions_on_the_known_region(A):
    afdm, dev = A
    g = torch.Generator().manual_seed(17)
    xa = (torch.rand(1, 8, 8, generator=g) * 2 - 1).to(dev)
    xb = (torch.rand(1, 8, 8, generator=g) * 2 - 1).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=8, device=dev)
    model = TwoImages(xa, xb, diff.alpha_hat)
    n = 64

    def nearest_a(x):
        da = (x - xa).flatten(1).norm(dim=1)
        db = (x - xb).flatten(1).norm(dim=1)
        return da < db

    afdm.set_seed(1)
    _, _, free = diff.sample(model, n=n, image_channels=1, steps=50, return_float=True)
    k = int(nearest_a(free).sum())
    assert 0 < k < n, k                                           # unconditional: both images appear
    mask = torch.zeros(1, 1, 8, 8)
    mask[..., :4] = 1                                             # the left half is known, from x_a
    images = xa.cpu().expand(n, 1, 8, 8).contiguous()
    ra = (xa[..., 4:]).flatten()
    for kw in ({"steps": 50, "eta": 0.0}, {"steps": 50, "eta": 1.0, "jump_length": 10, "jump_n_sample": 5}, {}):
        afdm.set_seed(2)
        _, _, x = diff.inpaint(model, images, mask, return_float=True, **kw)
        right = x[..., 4:].flatten(1)
        rel = (right - ra).norm(dim=1) / ra.norm()
        good = int((rel < 0.05).sum())
        assert good >= math.ceil(0.95 * n), (kw, good, rel.max().item())
        assert _same_bits(x[..., :4].cpu(), images[..., :4])


# ---- 7. the model's state after an exception ----------------------------------------------------------------------------------
def test_inpaint_restores_the_model_after_an_exception(A):
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
        diff.inpaint(model, torch.zeros(2, 3, 32, 32), torch.ones(1), steps=10, jump_length=2, jump_n_sample=2)
    assert Boom.calls == 3 and model.training and model._t_range is None
