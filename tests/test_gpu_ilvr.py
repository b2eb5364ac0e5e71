"""GPU tests of reference-guided sampling (ILVR): the fused low-pass refinement against the fp64 composition of the oracle's
resamplers and against the project's own resamplers on the device, its bit-level identities, ilvr == sample when no move is
refined, graph replay, a loop restated from the public ops, the forward count, an analytic two-image model on which the
reference must select the image, `reference_from_lowres`, and the model's state after an exception.

The graph test's chains: the DDIM chains (T = 1000) run with t_stop in {0, 300}.  The 30-step DDPM process cannot take
t_stop = 300 (t_stop lies in [0, T]): it runs with t_stop in {0, 10}, and a 330-step DDPM process runs with t_stop = 300."""
import math

import numpy as np
import pytest
import torch

from conftest import check

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10
GATE = 1e-5                      # the project's per-op gate on rel-L2 against fp64


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


def _slot(shape, dev, g, offset):
    """A standard-normal tensor of `shape`; offset > 0 places it `offset` elements into a larger buffer (unaligned)."""
    n = int(np.prod(shape))
    buf = torch.randn(n + offset, generator=g).to(dev)
    return buf[offset:].view(shape)


def _phi64(v, k, levels):
    """4^L U^L(D^L(v)) in fp64 on the CPU with the oracle's resamplers."""
    from oracle import ref_ops as R
    for _ in range(levels):
        v = R.filt_down2(v, k)
    for _ in range(levels):
        v = 4.0 * R.filt_up2(v, k)
    return v


def _phi_dev(ops, v, taps, levels):
    """The same composition from the project's own resamplers on the device."""
    for _ in range(levels):
        v = ops.FiltDown2.apply(v, taps)
    for _ in range(levels):
        v = ops.FiltUp2.apply(v, taps)
    return v * float(4 ** levels)


# ---- 1. the kernel against fp64 -------------------------------------------------------------------------------------------------
T_CASES = ((0, False), (0, True), (1, True), (998, True))        # (t_prev, whether the noise is passed)


@pytest.mark.parametrize("S,levels,N", [(8, 1, 3), (8, 2, 9), (16, 3, 5), (32, 2, 9), (64, 1, 15), (64, 5, 3)])
def test_refine_equals_the_fp64_composition(A, S, levels, N):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat.cpu().double()
    g = torch.Generator().manual_seed(1000 * S + 10 * levels + N)
    k = torch.randn(N, N, generator=g) / N                       # random and asymmetric: a transposed or flipped index fails
    assert not torch.equal(k, k.T) and not torch.equal(k, k.flip(0)) and not torch.equal(k, k.flip(1))
    taps = ops.Taps(k)
    for planes in (1, 3, 7):
        for off in (0, 1):
            shape = (planes, 1, S, S)
            x, ref, z = (_slot(shape, dev, g, off) for _ in range(3))
            zero = _slot(shape, dev, g, off).zero_()
            x64, r64, z64 = x.cpu().double(), ref.cpu().double(), z.cpu().double()
            known64 = [r64 if tp == 0 else math.sqrt(ah[tp]) * r64 + math.sqrt(1.0 - ah[tp]) * z64 for tp, _ in T_CASES]
            # one batched fp64 composition for the eight (t_prev, x) variants: phi acts per plane
            want = _phi64(torch.cat([kn - xx for kn in known64 for xx in (x64, torch.zeros_like(x64))]), k.double(), levels)
            want = want.reshape(len(T_CASES), 2, *shape)
            for ti, (tp, with_noise) in enumerate(T_CASES):
                for xi, xin in enumerate((x, zero)):
                    detail = (S, levels, N, planes, off, tp, with_noise, "x" if xi == 0 else "x=0")
                    out2 = _slot(shape, dev, g, off)
                    out = ops.lowpass_refine(xin, ref, z if with_noise else None, diff.alpha_hat, tp, taps, levels, out2=out2)
                    got = out.cpu().double() - xin.cpu().double()
                    check("ilvr: refine vs fp64 composition", got, want[ti, xi], GATE, detail)
                    assert _same_bits(out2, out), detail
                    known = ref if tp == 0 else ops.noise_images(ref.contiguous(), z.contiguous(),
                                                                  torch.full((planes,), tp, dtype=torch.long, device=dev),
                                                                  diff.alpha_hat)
                    comp = _phi_dev(ops, known - xin, taps, levels)
                    check("ilvr: device composition vs refine", comp.cpu().double(), got, GATE, detail)
                    if xi == 1 and tp == 0:                      # x = 0, known = ref: phi itself
                        assert _same_bits(ops.lowpass_project(ref, taps, levels), out), detail
    torch.cuda.synchronize()


# ---- 2. bit-level identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,levels,N", [((2, 3, 32, 32), 2, 9), ((7, 1, 16, 16), 3, 3), ((1, 2, 64, 64), 1, 15)])
def test_refine_bit_identities(A, shape, levels, N):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    g = torch.Generator().manual_seed(N + levels)
    taps = ops.Taps(torch.randn(N, N, generator=g) / N)
    x, ref, z = (_slot(shape, dev, g, 0) for _ in range(3))
    for tp in (0, 1, 500):
        zz = z if tp > 0 else None
        out2 = torch.full_like(x, float("nan"))
        out = ops.lowpass_refine(x, ref, zz, diff.alpha_hat, tp, taps, levels, out2=out2)
        assert _same_bits(out2, out)                                                        # out2 equals out
        assert _same_bits(ops.lowpass_refine(x, ref, zz, diff.alpha_hat, tp, taps, levels), out)   # two calls, the same bits
        inplace = x.clone()
        assert ops.lowpass_refine(inplace, ref, zz, diff.alpha_hat, tp, taps, levels, out=inplace) is inplace
        assert _same_bits(inplace, out)                                                     # in place equals out of place
        tp_dev = torch.full((1,), tp, device=dev, dtype=torch.long)
        got = x.clone()
        out2.fill_(float("nan"))
        ops.lowpass_refine_dev(got, ref, z, diff.alpha_hat, tp_dev, taps, levels, got, out2)   # (t_prev = 0: the noise is ignored)
        assert _same_bits(got, out) and _same_bits(out2, out)
    with pytest.raises(afdm.AfdError, match="t_prev"):
        ops.lowpass_refine(x, ref, z, diff.alpha_hat, 1000, taps, levels)
    with pytest.raises(afdm.AfdError, match="noise must not be NULL"):
        ops.lowpass_refine(x, ref, None, diff.alpha_hat, 3, taps, levels)
    with pytest.raises(afdm.AfdError, match="must not overlap"):
        ops.lowpass_refine(x, ref, z, diff.alpha_hat, 3, taps, levels, out=ref)
    with pytest.raises(afdm.AfdError, match="N odd"):
        ops.lowpass_refine(x, ref, z, diff.alpha_hat, 3, torch.ones(4, 4), levels)
    with pytest.raises(afdm.AfdError, match="levels"):
        ops.lowpass_refine(x, ref, z, diff.alpha_hat, 3, taps, 6)
    with pytest.raises(afdm.AfdError, match="square planes"):
        ops.lowpass_refine(x.view(-1, shape[-1] * shape[-2]), ref, z, diff.alpha_hat, 3, taps, levels)
    torch.cuda.synchronize()


# ---- 3. without a refined move ilvr is `sample`, bit for bit ----------------------------------------------------------------------
def _run(diff, fn, seed, **kw):
    import afdm
    afdm.set_seed(seed)
    xq, rq, xf = fn(return_float=True, **kw)
    snaps = [s.cpu() for s in diff.last_float_snapshots]
    after = torch.randn(4, device=xf.device).cpu()           # where the device generator stands afterwards
    after_cpu = torch.randn(4)                               # and the CPU generator
    return xq.cpu(), rq.cpu(), xf.cpu(), snaps, after, after_cpu


def _equal_runs(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and _same_bits(a[2], b[2]) and len(a[3]) == len(b[3]) >= 1
            and all(_same_bits(p, q) for p, q in zip(a[3], b[3])) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5]))


@pytest.mark.parametrize("cfg", ["ddpm", "ddpm-graph", "ddim0", "ddim1", "ddim1-graph", "ddim0-graph", "ddpm-guided",
                                 "ddim1-guided-graph"])
def test_no_refined_move_is_sample(A, cfg):
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
    reference = torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
    s = _run(diff, lambda **k: diff.sample(model, n=n, image_channels=3, **k), 9, **kw)
    for t_stop in (T, T - 1):
        p = _run(diff, lambda **k: diff.ilvr(model, reference, t_stop=t_stop, **k), 9, **kw)
        assert _equal_runs(s, p) and len(p[3]) >= 2, t_stop
    assert model.training and model._t_range is None


# ---- 4. graph replay equals the eager loop ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,T,t_stop", [("ddpm", 30, 0), ("ddpm", 30, 10), ("ddpm", 330, 300),
                                          ("ddim1-guided", 1000, 0), ("ddim1-guided", 1000, 300),
                                          ("ddim0", 1000, 0), ("ddim0", 1000, 300)])
def test_ilvr_graph_equals_eager(A, cfg, T, t_stop):
    afdm, dev = A
    guided = "guided" in cfg
    model = _model(afdm, dev, num_classes=K if guided else None)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    kw = {"t_stop": t_stop, "noise_source": "device"}
    if cfg.startswith("ddim"):
        kw.update(steps=8, eta=float(cfg[4]))
    if guided:
        kw.update(labels=torch.tensor([1, 8], device=dev), cfg_scale=3.0)
    reference = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 2 - 1
    outs = [_run(diff, lambda **k: diff.ilvr(model, reference, **k), 11, graph=g, **kw) for g in (False, True)]
    assert _equal_runs(outs[0], outs[1])
    free = _run(diff, lambda **k: diff.ilvr(model, reference, **k), 11, graph=False, **dict(kw, t_stop=T))
    assert not _same_bits(free[2], outs[0][2])                    # (the refinement did act)
    assert model.training and model._t_range is None


# ---- 5. the loop restated from the public ops -----------------------------------------------------------------------------------
def test_ilvr_equals_the_restated_ddim_loop(A):
    afdm, dev = A
    from afdm import ops
    model = _model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    n, shape = 2, (2, 3, 32, 32)
    reference = torch.rand(shape, generator=torch.Generator().manual_seed(5)) * 2 - 1
    taps = afdm.circularLowpassKernel(math.pi / 2, 9, beta=8)
    afdm.set_seed(21)
    _, _, got = diff.ilvr(model, reference, factor=4, steps=4, eta=1.0, noise_source="cpu", return_float=True)
    after = torch.randn(4)
    afdm.set_seed(21)
    ref = reference.to(dev)
    x = torch.randn(shape).to(dev)                               # x_T, then per move the step noise, then the reference noise
    with diff._model_scope(model):                               # eval mode, no_grad, the timestep hint: as the samplers run
        for t, tp in diff._ddim_pairs(4, 1.0):
            eps = diff.predict_eps(model, x, torch.full((n,), t, device=dev, dtype=torch.long))
            z = torch.randn(shape).to(dev) if tp > 0 else None
            x = ops.ddim_step(x, eps, z, diff.alpha_hat, t, tp, 1.0)
            zr = torch.randn(shape).to(dev) if tp > 0 else None
            x = ops.lowpass_refine(x, ref, zr, diff.alpha_hat, tp, taps, 2)
    assert _same_bits(got, x)
    assert torch.equal(after, torch.randn(4))


def test_ilvr_equals_the_restated_learned_variance_loop(A):
    afdm, dev = A
    from afdm import ops
    model = _model(afdm, dev, c_out=6)
    T = 12
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, variance="learned")
    n, shape = 2, (2, 3, 32, 32)
    reference = torch.rand(shape, generator=torch.Generator().manual_seed(6)) * 2 - 1
    taps = afdm.circularLowpassKernel(math.pi / 2, 9, beta=8)
    afdm.set_seed(22)
    _, _, got = diff.ilvr(model, reference, factor=2, t_stop=3, noise_source="cpu", return_float=True)
    after = torch.randn(4)
    afdm.set_seed(22)
    ref = reference.to(dev)
    x = torch.randn(shape).to(dev)
    with diff._model_scope(model):
        for i in range(T - 1, 0, -1):
            out2 = model(x, torch.full((n,), i, device=dev, dtype=torch.long)).contiguous()
            z = torch.randn(shape).to(dev) if i > 1 else None
            x = ops.denoise_step_lvar(x, out2, z, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), "eps", i)
            if i - 1 >= 3:                                       # t_stop = 3
                x = ops.lowpass_refine(x, ref, torch.randn(shape).to(dev), diff.alpha_hat, i - 1, taps, 1)
    assert _same_bits(got, x)
    assert torch.equal(after, torch.randn(4))


# ---- 6. one forward per move ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,graph", [(10, False), (10, True), (None, False)])
def test_ilvr_forward_count(A, steps, graph):
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
    diff.ilvr(model, torch.zeros(2, 3, 32, 32), steps=steps, t_stop=0 if graph else 5, graph=graph)
    moves = T - 1 if steps is None else steps
    # graph: one warm-up and one capture instead of the replayed moves' calls (every move but the last is replayed)
    assert model.calls == (2 + 1 if graph else moves)


# ---- 7. conditioning works: the exact denoiser of a two-image data set ---------------------------------------------------------
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


@pytest.fixture(scope="module")
def two_images(A):
    """x_a = 0.6 pat + 0.3 u_a, x_b = -0.6 pat + 0.3 u_b on 16 x 16: the images differ in their coarse content."""
    afdm, dev = A
    g = torch.Generator().manual_seed(17)
    i = torch.arange(16, dtype=torch.float32)
    pat = torch.cos(math.pi * (i + 0.5) / 16)[:, None].expand(16, 16)
    xa = (0.6 * pat + 0.3 * (torch.rand(1, 16, 16, generator=g) * 2 - 1)).to(dev)
    xb = (-0.6 * pat + 0.3 * (torch.rand(1, 16, 16, generator=g) * 2 - 1)).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=16, device=dev)
    return xa, xb, diff, TwoImages(xa, xb, diff.alpha_hat)


def _nearest_a(x, xa, xb):
    return (x - xa).flatten(1).norm(dim=1) < (x - xb).flatten(1).norm(dim=1)


def test_free_sampling_lands_on_both_images(A, two_images):
    afdm, dev = A
    xa, xb, diff, model = two_images
    afdm.set_seed(1)
    _, _, free = diff.sample(model, n=64, image_channels=1, steps=50, return_float=True)
    k = int(_nearest_a(free, xa, xb).sum())
    print(f"free sampling: {k} of 64 nearest x_a")
    assert 0 < k < 64, k


@pytest.mark.parametrize("filt", ["default", "n3"])
@pytest.mark.parametrize("steps,eta", [(50, 0.0), (20, 1.0)])
@pytest.mark.parametrize("factor", [2, 4])
def test_ilvr_conditions_on_the_reference(A, two_images, factor, steps, eta, filt):
    afdm, dev = A
    from afdm import ops
    xa, xb, diff, model = two_images
    n = 64
    taps = None if filt == "default" else afdm.circularLowpassKernel(F_SET["omega_c_down"], F_SET["kernel_size"], F_SET["kaiser_beta"])
    k, levels = diff._ilvr_operator("ilvr", factor, taps)
    for target, is_a in ((xa, True), (xb, False)):
        reference = ops.lowpass_project(target[None], k, levels).expand(n, 1, 16, 16).contiguous()
        afdm.set_seed(2)
        _, _, x = diff.ilvr(model, reference, factor=factor, taps=taps, steps=steps, eta=eta, return_float=True)
        hits = int((_nearest_a(x, xa, xb) == is_a).sum())
        print(f"ilvr factor {factor} steps {steps} eta {eta} filter {filt} towards {'x_a' if is_a else 'x_b'}: {hits} of {n}")
        assert hits >= 61, (factor, steps, eta, filt, is_a, hits)


# ---- 8. a reference from low-resolution images ----------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,filt", [(2, "default"), (4, "default"), (8, "n3")])
def test_reference_from_lowres(A, factor, filt):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    taps = None if filt == "default" else afdm.circularLowpassKernel(math.pi / 2, 3, 2)
    k, levels = diff._ilvr_operator("ilvr", factor, taps)
    v = (torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(8)) * 2 - 1).to(dev)
    low = v
    for _ in range(levels):
        low = ops.FiltDown2.apply(low, k)
    assert tuple(low.shape) == (2, 3, 32 // factor, 32 // factor)
    got = diff.reference_from_lowres(low.cpu(), factor, taps)
    assert got.device.type == "cuda" and tuple(got.shape) == (2, 3, 32, 32)
    check("ilvr: reference_from_lowres vs lowpass_project", got.cpu(), ops.lowpass_project(v, k, levels).cpu(), GATE, (factor, filt))
    if factor == 4:
        model = _model(afdm, dev)
        afdm.set_seed(3)
        xq, rq, xf = diff.ilvr(model, got, factor=factor, taps=taps, steps=4, return_float=True)
        assert xq.dtype == torch.uint8 and tuple(xq.shape) == (2, 3, 32, 32) and bool(torch.isfinite(xf).all())
        assert model.training and model._t_range is None


# ---- 9. the model's state after an exception --------------------------------------------------------------------------------------
def test_ilvr_restores_the_model_after_an_exception(A):
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
        diff.ilvr(model, torch.zeros(2, 3, 32, 32), steps=10)
    assert Boom.calls == 3 and model.training and model._t_range is None
