"""GPU tests of the real-image methods: the ascending DDIM step's four entry points against a per-operation fp32 restatement (bit
for bit) and an fp64 one, ops.slerp against a numpy fp64 restatement, `invert` against a loop on the CPU oracle and against fp64
chains on Gaussian data (where the probability-flow map is closed form and the refinement's contraction can be measured), what
`invert` draws and how many forwards it runs, graph replay, guidance, `decode` against `sample`, `sdedit` and `interpolate` against
the same public calls made by hand, the model's state after an exception, and `reconstruct_results` on a checkpoint."""
import math

import numpy as np
import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10
T = 1000


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42, num_classes=None):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


@pytest.fixture(scope="module")
def M(A):
    """The tiny model, its guided sibling and the process, built once."""
    afdm, dev = A
    return _model(afdm, dev), _model(afdm, dev, num_classes=K), afdm.Diffusion(noise_steps=T, img_size=32, device=dev)


def _images(n, seed, dev, c=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, c, 32, 32, generator=g) * 2 - 1).to(dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _f32(v):
    return float(np.float32(v))


# ---- restatements of the ascending step ------------------------------------------------------------------------------------------
def _lerp_restated(u, c, s):
    """ATen's scalar lerp, one device op per step (as in test_gpu_ddim.py)."""
    d = c - u
    if abs(s) < 0.5:
        return u + d * s
    return c - d * _f32(1 - _f32(s))


def _invert_restated(x, e, ah, s, u):
    """The step as separate fp32 device ops, each a full-tensor operand; the scalars in fp32, one IEEE rounding per operation
    (taken in fp64 and rounded once: exact for + - * / sqrt)."""
    a_s, a_u = float(ah[s]), float(ah[u])
    sq = lambda v: _f32(math.sqrt(v))
    full = lambda v: torch.full_like(x, v)
    pe = e * full(sq(_f32(1 - a_s)))
    x0 = (x - pe) / full(sq(a_s))
    return x0 * full(sq(a_u)) + e * full(sq(_f32(1 - a_u)))


def _up64(x, e, ah, s, u):
    """The step in fp64 (numpy arrays or fp64 tensors)."""
    a_s, a_u = float(ah[s]), float(ah[u])
    return math.sqrt(a_u) * ((x - math.sqrt(1 - a_s) * e) / math.sqrt(a_s)) + math.sqrt(1 - a_u) * e


# ---- 1. the four entry points ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("s,u", [(0, 1), (0, 999), (36, 37), (350, 700), (998, 999)])
def test_invert_step_equals_restatements(A, M, form, guided, s, u):
    afdm, dev = A
    from afdm import ops
    diff = M[2]
    ah = diff.alpha_hat.cpu()
    scale = 3.0
    g = torch.Generator().manual_seed(7 * u + s)
    fam = "invert: fused ascending step vs fp64 restatement" + (" (guided)" if guided else "")
    for shape in ((4, 3, 8, 8), (3, 3, 5, 7)):                           # 16-byte path and scalar path (n % 4 != 0)
        n = shape[0]
        for in_place in (False, True):
            x = torch.randn(shape, generator=g).to(dev)
            if guided:
                eps = torch.randn((2 * n,) + shape[1:], generator=g).to(dev)
                e = _lerp_restated(eps[n:], eps[:n], scale)
                e64 = eps[n:].double() + scale * (eps[:n].double() - eps[n:].double())
            else:
                eps = e = e64 = torch.randn(shape, generator=g).to(dev)
            want = _invert_restated(x, e, ah, s, u)
            want64 = _up64(x.double(), e64.double(), ah.double(), s, u)
            keep = x.clone()
            out = x if in_place else torch.full_like(x, float("nan"))
            out2 = torch.full_like(x, float("nan"))
            if form == "host":
                index = (s, u)
            else:
                index = (torch.full((1,), s, device=dev, dtype=torch.long), torch.full((2 * n,), u, device=dev, dtype=torch.long))
            name = "ddim_invert_step" + "_cfg" * guided + "_dev" * (form == "dev")
            if guided:
                got = getattr(ops, name)(x, eps, diff.alpha_hat, *index, scale, out, out2)
            else:
                got = getattr(ops, name)(x, eps, diff.alpha_hat, *index, out)
                out2.copy_(got)
            assert got.data_ptr() == out.data_ptr()
            assert in_place or _same_bits(x, keep)                      # x is only read
            assert _same_bits(got, want), (shape, in_place, int((got != want).sum()))
            assert _same_bits(out2, got)
            check(fam, got.cpu(), want64.cpu(), 1e-6, (form, s, u, shape, in_place))
    if form == "host" and not guided:                                    # `out` defaults to a new tensor
        got = ops.ddim_invert_step(x, e, diff.alpha_hat, s, u)
        assert got.data_ptr() != x.data_ptr() and _same_bits(got, _invert_restated(x, e, ah, s, u))
    torch.cuda.synchronize()


def test_invert_step_is_the_inverse_of_the_samplers_step(A, M):
    """For the same eps, up (s -> u) then ops.ddim_step (u -> s, eta = 0) returns x up to fp32 rounding."""
    afdm, dev = A
    from afdm import ops
    diff = M[2]
    g = torch.Generator().manual_seed(3)
    x, e = torch.randn(2, 3, 32, 32, generator=g).to(dev), torch.randn(2, 3, 32, 32, generator=g).to(dev)
    for s, u in ((0, 1), (36, 37), (350, 700), (0, 999)):
        back = ops.ddim_step(ops.ddim_invert_step(x, e, diff.alpha_hat, s, u), e, None, diff.alpha_hat, u, s, 0.0)
        # the worst case (0, 999): x_u - sqrt(1 - a_u) e cancels down to sqrt(a_u) x0 and is divided by sqrt(a_999) = 6.4e-3, so
        # half an ulp each of x_u and of the product, 2 * 6e-8 of values near |x|, becomes at most 1.9e-5 of x
        check("invert: ascending step then the sampler's step, same eps", back, x, 2e-5, (s, u))


def test_invert_step_checks_its_arguments(A, M):
    afdm, dev = A
    from afdm import ops
    diff = M[2]
    x = torch.zeros(2, 3, 4, 4, device=dev)
    x2 = torch.cat([x, x])
    i64 = lambda v: torch.full((1,), v, device=dev, dtype=torch.long)
    for s, u in ((10, 10), (11, 10), (-1, 5)):
        with pytest.raises(afdm.AfdError, match="s < u"):
            ops.ddim_invert_step(x, x.clone(), diff.alpha_hat, s, u)
        with pytest.raises(afdm.AfdError, match="s < u"):
            ops.ddim_invert_step_cfg(x, x2, diff.alpha_hat, s, u, 3.0)
    with pytest.raises(afdm.AfdError, match="s < u < 1000"):
        ops.ddim_invert_step(x, x.clone(), diff.alpha_hat, 10, 1000)                  # u past the table
    with pytest.raises(afdm.AfdError, match="s < u < 1000"):
        ops.ddim_invert_step_cfg(x, x2, diff.alpha_hat, 999, 1000, 3.0)
    with pytest.raises(afdm.AfdError, match="contiguous"):
        ops.ddim_invert_step(x, x.transpose(2, 3), diff.alpha_hat, 5, 10)
    with pytest.raises(afdm.AfdError, match="contiguous"):
        ops.ddim_invert_step(x, x.clone(), diff.alpha_hat, 5, 10, out=torch.zeros(2, 3, 4, 8, device=dev)[..., ::2])
    with pytest.raises(afdm.AfdError, match="fp32"):
        ops.ddim_invert_step(x, x.double(), diff.alpha_hat, 5, 10)
    with pytest.raises(afdm.AfdError, match="eps2"):
        ops.ddim_invert_step_cfg(x, x.clone(), diff.alpha_hat, 5, 10, 3.0)
    with pytest.raises(afdm.AfdError, match="eps2"):
        ops.ddim_invert_step_cfg_dev(x, x.clone(), diff.alpha_hat, i64(5), i64(10), 3.0, x)
    with pytest.raises(afdm.AfdError, match="96 elements"):
        ops.ddim_invert_step(x, x.clone(), diff.alpha_hat, 5, 10, out=torch.zeros(95, device=dev))
    for bad in (torch.zeros(1, device=dev), torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(1, dtype=torch.long), 5):
        with pytest.raises(afdm.AfdError, match="int64"):
            ops.ddim_invert_step_dev(x, x.clone(), diff.alpha_hat, bad, i64(10), x)
        with pytest.raises(afdm.AfdError, match="int64"):
            ops.ddim_invert_step_cfg_dev(x, x2, diff.alpha_hat, i64(5), bad, 3.0, x)
    with pytest.raises(afdm.AfdError, match="afd_ddim_invert_step: x_out and x_out2 must not overlap eps"):
        e = x.clone()
        ops.ddim_invert_step(x, e, diff.alpha_hat, 5, 10, out=e)


# ---- 2. slerp ----------------------------------------------------------------------------------------------------------------------
def _slerp64(a, b, w):
    """numpy fp64 restatement: a, b (pairs, row) fp32 arrays, w fp32 weights -> (pairs, W, row) fp32."""
    a, b, w = a.astype(np.float64), b.astype(np.float64), np.asarray(w, dtype=np.float32).astype(np.float64)
    out = np.empty((a.shape[0], w.size, a.shape[1]), dtype=np.float32)
    for i in range(a.shape[0]):
        d, na, nb = float(a[i] @ b[i]), float(a[i] @ a[i]), float(b[i] @ b[i])
        lerp = na == 0 or nb == 0
        if not lerp:
            omega = math.acos(min(max(d / math.sqrt(na * nb), -1.0), 1.0))
            so = math.sin(omega)
            lerp = so < 1e-6
        for k, wk in enumerate(w):
            ca, cb = (1 - wk, wk) if lerp else (math.sin((1 - wk) * omega) / so, math.sin(wk * omega) / so)
            out[i, k] = (ca * a[i] + cb * b[i]).astype(np.float32)
    return out


WEIGHTS = {1: [0.3], 3: [0.0, 0.5, 1.0], 5: [0.0, 0.25, 0.5, 0.9, 1.0]}


@pytest.mark.parametrize("pairs,W,row,off", [(1, 1, 105, 0), (3, 5, 192, 0), (2, 3, 12288, 0), (3, 5, 192, 1)])
def test_slerp_equals_fp64_restatement(A, pairs, W, row, off):
    afdm, dev = A
    from afdm import ops
    g = torch.Generator().manual_seed(100 * pairs + row)
    a_h, b_h = torch.randn(pairs, row, generator=g), torch.randn(pairs, row, generator=g)
    a = torch.zeros(pairs * row + off, device=dev)[off:].view(pairs, row)           # off = 1: misaligned, the scalar path
    a.copy_(a_h)
    b = b_h.to(dev)
    assert a.data_ptr() % 16 == 4 * off and a.is_contiguous()
    w = WEIGHTS[W]
    got = ops.slerp(a, b, w)
    assert got.shape == (pairs, W, row) and got.dtype == torch.float32
    check("slerp: kernel vs numpy fp64 restatement", got.cpu(), torch.from_numpy(_slerp64(a_h.numpy(), b_h.numpy(), w)), 1e-6,
          (pairs, W, row, off))
    assert _same_bits(got, ops.slerp(a, b, torch.tensor(w)))                       # a tensor of weights; and the same bits again
    assert _same_bits(got, ops.slerp(a, b, torch.tensor(w, dtype=torch.float64, device=dev)))
    if off:                                                                        # alignment does not change a bit
        assert _same_bits(got, ops.slerp(a_h.to(dev), b, w))
    if W > 1:                                                                      # the end points are the inputs
        assert _same_bits(got[:, 0], a) and _same_bits(got[:, -1], b)
    shaped = ops.slerp(a.contiguous().view(pairs, 3, row // 3), b.view(pairs, 3, row // 3), w)
    assert shaped.shape == (pairs, W, 3, row // 3) and _same_bits(shaped.view(pairs, W, row), got)


def test_slerp_degenerate_rows_fall_back_to_lerp_and_unit_rows_stay_unit(A):
    afdm, dev = A
    from afdm import ops
    g = torch.Generator().manual_seed(5)
    row, w = 3 * 16 * 16, [0.0, 0.25, 0.5, 1.0]
    a = torch.randn(4, row, generator=g)
    b = torch.stack([a[0], -a[1], torch.zeros(row), torch.randn(row, generator=g)])    # parallel, antiparallel, zero, generic
    got = ops.slerp(a.to(dev), b.to(dev), w).cpu()
    w64 = torch.tensor(w, dtype=torch.float64).view(1, -1, 1)
    lerp = ((1 - w64) * a.double()[:, None] + w64 * b.double()[:, None]).float()
    for i in range(3):
        assert _same_bits(got[i], lerp[i]), i
    assert _same_bits(got[0], a[0].expand(4, row))                    # b = a: every weight returns a
    assert not _same_bits(got[3], lerp[3])
    check("slerp: kernel vs numpy fp64 restatement", got, torch.from_numpy(_slerp64(a.numpy(), b.numpy(), w)), 1e-6, "degenerate rows")
    z = torch.zeros(2, row, device=dev)
    assert _same_bits(ops.slerp(z, z, w), torch.zeros(2, 4, row, device=dev))
    # unit rows: |ca a + cb b|^2 = (sin^2((1-w) o) + sin^2(w o) + 2 sin((1-w) o) sin(w o) cos o) / sin^2 o = 1
    ua, ub = a / a.norm(dim=1, keepdim=True), torch.randn(4, row, generator=g)
    ub = ub / ub.norm(dim=1, keepdim=True)
    norms = ops.slerp(ua.to(dev), ub.to(dev), [0.1, 0.37, 0.5, 0.8]).double().norm(dim=2).cpu()
    dev_norm = float((norms - 1).abs().max())
    note("slerp: | |out| - 1 | for unit rows", dev_norm)
    assert dev_norm < 1e-5


def test_slerp_checks_its_arguments(A):
    afdm, dev = A
    from afdm import ops
    a = torch.zeros(2, 3, 8, 8, device=dev)
    E = afdm.AfdError
    with pytest.raises(E, match="fp32"):
        ops.slerp(a, a.double(), [0.5])
    with pytest.raises(E, match="HIP device"):
        ops.slerp(a, a.cpu(), [0.5])
    with pytest.raises(E, match="one shape"):
        ops.slerp(a, a[:1], [0.5])
    with pytest.raises(E, match="one shape"):
        ops.slerp(a.view(2, 192), a, [0.5])
    with pytest.raises(E, match="one shape"):
        ops.slerp(a.view(-1), a.view(-1), [0.5])
    with pytest.raises(E, match="contiguous"):
        ops.slerp(a, a.transpose(2, 3), [0.5])
    with pytest.raises(E, match="between 1 and 12288"):
        ops.slerp(torch.zeros(1, 12289, device=dev), torch.zeros(1, 12289, device=dev), [0.5])
    with pytest.raises(E, match="tensors"):
        ops.slerp(a, a.cpu().numpy(), [0.5])
    for w in ([], [[0.5]], 0.5, [float("nan")], [0.5, float("inf")], ["x"], torch.zeros(2, 2), torch.tensor([True])):
        with pytest.raises(E, match="weights"):
            ops.slerp(a, a, w)


# ---- 3. invert: a trajectory against the CPU oracle ---------------------------------------------------------------------------------
def test_invert_trajectory_vs_cpu_oracle_loop(A, M):
    afdm, dev = A
    from oracle import ref_ops as R
    model, _, diff = M
    n, S, refine = 2, 5, 1
    images = _images(n, 21, dev)
    lat = diff.invert(model, images, S, refine=refine)
    assert lat.shape == images.shape and lat.dtype == torch.float32 and lat.device == images.device
    assert model.training and model._t_range is None
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ah = diff.alpha_hat.cpu().double()
    taus = diff.ddim_timesteps(S)
    levels = [0] + taus[::-1]
    x = images.cpu().double()
    with torch.no_grad():
        for s, u in zip(levels, levels[1:]):
            z = x
            for _ in range(refine + 1):
                e = R.unet_forward(sd, z.float(), torch.full((n,), u, dtype=torch.long), 3, F_SET).double()
                z = _up64(x, e, ah, s, u)
            x = z
    err = check("invert: 5 levels, refine 1 vs a loop on the CPU oracle (fp64 step)", lat.cpu(), x, 1e-5)
    print(f"invert trajectory (T=1000, S=5, refine=1, ten forwards) vs oracle loop: rel-L2 {err:.2e}")


# ---- 4. Gaussian data: everything closed form ----------------------------------------------------------------------------------------
class _GaussEps(torch.nn.Module):
    """The exact eps of x0 ~ N(mu, 0.5^2 I): eps(x, t) = sqrt(1 - a)(x - sqrt(a) mu) / (0.25 a + 1 - a), a = alpha_hat[t], in
    fp64 and rounded to fp32 (the construction of test_gpu_dpm.py)."""

    def __init__(self, mu, alpha_hat):
        super().__init__()
        self.mu, self.ah = mu, alpha_hat.double()

    def forward(self, x, t):
        a = self.ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (0.25 * a + 1 - a)).float()


def test_invert_on_gaussian_data_refinement_contracts_and_error_falls_with_steps(A, M):
    """Round-trip rel-L2 of decode(invert(x0, 50, refine), 50) in an fp64 run of this setting: 5.3e-2, 4.8e-3, 4.6e-4, 4.8e-5 for
    refine 0 .. 3 (a factor 115 at refine 2 and 1100 at 3: the bounds below leave 2x and 10x for the seed and fp32); latent error
    of refine 0 against the exact probability-flow map: 5.0e-2, 1.18e-1, 2.18e-1 at S = 50, 20, 10."""
    afdm, dev = A
    diff = M[2]
    ah = diff.alpha_hat.cpu().double().numpy()
    g = torch.Generator().manual_seed(0)
    mu_t = torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 1.6 - 0.8               # 4096 means in [-0.8, 0.8]
    x0_t = (mu_t + 0.5 * torch.randn(1, 4, 32, 32, generator=g, dtype=torch.float64)).float()
    model = _GaussEps(mu_t.to(dev), diff.alpha_hat)
    mu, x0 = mu_t.numpy(), x0_t.double().numpy()

    def eps64(x, t):
        return math.sqrt(1 - ah[t]) * (x - math.sqrt(ah[t]) * mu) / (0.25 * ah[t] + 1 - ah[t])

    def invert64(taus, refine):
        levels, x = [0] + taus[::-1], x0
        for s, u in zip(levels, levels[1:]):
            z = x
            for _ in range(refine + 1):
                z = _up64(x, eps64(z, u), ah, s, u)
            x = z
        return x

    var = lambda t: 0.25 * ah[t] + 1 - ah[t]
    exact = math.sqrt(ah[T - 1]) * mu + math.sqrt(var(T - 1) / var(0)) * (x0 - math.sqrt(ah[0]) * mu)     # level 0 -> T - 1
    rt, err = {}, {}
    for S, refine in ((50, 0), (50, 1), (50, 2), (50, 3), (20, 0), (10, 0)):
        lat = diff.invert(model, x0_t.to(dev), S, refine=refine)
        check("invert: Gaussian data, GPU latent vs its fp64 chain", lat.cpu(), invert64(diff.ddim_timesteps(S), refine), 1e-5, (S, refine))
        if refine == 0:
            err[S] = rel_l2(lat.cpu(), exact)
            note(f"invert: Gaussian data, latent error of refine 0 at S = {S}", err[S])
        if S == 50:
            back = diff.decode(model, lat, S, return_float=True)[2]
            rt[refine] = rel_l2(back.cpu(), x0)
            note(f"invert: Gaussian data, round trip at S = 50, refine {refine}", rt[refine])
    print("round trip rel-L2 by refine:", {k: f"{v:.3e}" for k, v in rt.items()}, "latent error by S:", {k: f"{v:.3e}" for k, v in err.items()})
    assert rt[2] <= rt[0] / 50
    assert rt[3] <= rt[0] / 100
    assert err[50] < err[20] < err[10]


# ---- 5. what invert draws and runs ---------------------------------------------------------------------------------------------------
def test_invert_draws_nothing_and_runs_refine_plus_one_forwards_per_level(A, M):
    afdm, dev = A
    model, _, diff = M
    images = _images(2, 4, dev)
    calls = []
    hook = model.register_forward_hook(lambda *a: calls.append(1))
    try:
        for S, refine in ((4, 0), (4, 2), ([900, 500, 20], 1)):
            afdm.set_seed(9)
            cpu, gpu_state = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
            calls.clear()
            diff.invert(model, images, S, refine=refine)
            assert len(calls) == (refine + 1) * (S if isinstance(S, int) else len(S))
            assert torch.equal(torch.get_rng_state(), cpu) and torch.equal(torch.cuda.get_rng_state(dev), gpu_state)
    finally:
        hook.remove()
    a = diff.invert(model, images, 4)
    assert _same_bits(a, diff.invert(model, images, diff.ddim_timesteps(4)))          # an explicit sequence is the same chain
    assert _same_bits(images, _images(2, 4, dev))                                      # the images are not written


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("refine", [0, 2])
def test_invert_graph_equals_eager(A, M, guided, refine):
    afdm, dev = A
    model, diff = M[1 if guided else 0], M[2]
    kw = {"labels": torch.tensor([1, afdm.NULL_LABEL, 8], device=dev), "cfg_scale": 3.0} if guided else {}
    images = _images(3, 6, dev)
    eager = diff.invert(model, images, 4, refine=refine, **kw)
    graph = diff.invert(model, images, 4, refine=refine, graph=True, **kw)
    assert model.training and model._t_range is None
    assert _same_bits(eager, graph)


def test_guided_invert_equals_hand_loop(A, M):
    afdm, dev = A
    from afdm import ops
    _, model, diff = M
    n, s, S, refine = 3, 3.0, 4, 1
    labels = [3, afdm.NULL_LABEL, 7]
    images = _images(n, 8, dev)
    got = diff.invert(model, images, S, refine=refine, labels=labels, cfg_scale=s)
    y2 = torch.tensor(labels + [afdm.NULL_LABEL] * n, device=dev)
    levels = [0] + diff.ddim_timesteps(S)[::-1]
    model.eval()
    with torch.no_grad():
        x = images.clone()
        for lo, hi in zip(levels, levels[1:]):
            z = x
            for _ in range(refine + 1):
                eps2 = diff.predict_eps(model, torch.cat([z, z]), torch.full((2 * n,), hi, device=dev, dtype=torch.long), y2)
                z = ops.ddim_invert_step_cfg(x, eps2, diff.alpha_hat, lo, hi, s)
            x = z
    model.train()
    assert _same_bits(got, x)
    assert not _same_bits(got, diff.invert(model, images, S, refine=refine, labels=labels))      # the guidance does something


# ---- 6. decode, sdedit, interpolate against the same calls made by hand -----------------------------------------------------------
@pytest.mark.parametrize("steps", [6, [950, 610, 333, 40]])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_decode_from_drawn_noise_is_sample(A, M, eta, steps):
    afdm, dev = A
    model, _, diff = M
    shape = (2, 3, 32, 32)
    afdm.set_seed(17)
    xq, rq, xf = diff.sample(model, n=2, image_channels=3, noise_source="device", return_float=True, steps=steps, eta=eta)
    snaps = [s.clone() for s in diff.last_float_snapshots]
    afdm.set_seed(17)
    xT = torch.randn(shape, device=dev)
    keep = xT.clone()
    dq, dr, df = diff.decode(model, xT, steps=steps, eta=eta, noise_source="device", return_float=True)
    assert _same_bits(df, xf) and torch.equal(dq, xq) and torch.equal(dr, rq)
    assert len(diff.last_float_snapshots) == len(snaps) and all(_same_bits(a, b) for a, b in zip(diff.last_float_snapshots, snaps))
    assert _same_bits(xT, keep)                                                     # the latents are not written
    assert model.training and model._t_range is None
    assert len(diff.decode(model, xT, steps=steps, eta=eta, noise_source="device")) == 2


def test_decode_graph_and_guidance_follow_sample(A, M):
    afdm, dev = A
    _, model, diff = M
    kw = {"labels": torch.tensor([1, afdm.NULL_LABEL], device=dev), "cfg_scale": 3.0, "steps": 5, "eta": 0.5, "noise_source": "device",
          "return_float": True}
    afdm.set_seed(2)
    want = diff.sample(model, n=2, image_channels=3, **kw)[2]
    for graph in (None, True):
        afdm.set_seed(2)
        xT = torch.randn((2, 3, 32, 32), device=dev)
        assert _same_bits(diff.decode(model, xT, graph=graph, **kw)[2], want)


@pytest.mark.parametrize("steps", [5, [400, 250, 90, 3]])
def test_sdedit_is_noise_images_then_decode(A, M, steps):
    afdm, dev = A
    from afdm import ops
    model, _, diff = M
    n, t0, eta = 2, 400, 0.5
    images = _images(n, 12, dev)
    afdm.set_seed(23)
    gq, gr, gf = diff.sdedit(model, images, t0, steps, eta=eta, noise_source="device", return_float=True)
    afdm.set_seed(23)
    z = torch.randn((n, 3, 32, 32), device=dev)
    x = ops.noise_images(images, z, torch.full((n,), t0, device=dev, dtype=torch.long), diff.alpha_hat)
    taus = diff.ddim_timesteps_from(t0, steps) if isinstance(steps, int) else steps
    wq, wr, wf = diff.decode(model, x, taus, eta=eta, noise_source="device", return_float=True)
    assert _same_bits(gf, wf) and torch.equal(gq, wq) and torch.equal(gr, wr)
    assert model.training and model._t_range is None
    with pytest.raises(ValueError, match="must start at t0 = 400"):
        diff.sdedit(model, images, t0, [399, 100])
    # the default noise source draws z on the CPU, as `sample` draws x_T
    afdm.set_seed(23)
    rf = diff.sdedit(model, images, t0, steps, return_float=True)[2]
    afdm.set_seed(23)
    x = ops.noise_images(images, torch.randn((n, 3, 32, 32)).to(dev), torch.full((n,), t0, device=dev, dtype=torch.long), diff.alpha_hat)
    assert _same_bits(rf, diff.decode(model, x, taus, return_float=True)[2])


def test_interpolate_is_invert_slerp_decode(A, M):
    afdm, dev = A
    from afdm import ops
    model, _, diff = M
    n, S, w = 2, 5, [0.0, 0.5, 1.0]
    a, b = _images(n, 31, dev), _images(n, 32, dev)
    gq, gr, gf = diff.interpolate(model, a, b, w, S, return_float=True)
    assert gq.shape == (n * 3, 3, 32, 32) and gq.dtype == torch.uint8
    lat = diff.invert(model, torch.cat([a, b]), S)
    mid = ops.slerp(lat[:n], lat[n:], w)
    assert mid.shape == (n, 3, 3, 32, 32)
    wq, wr, wf = diff.decode(model, mid.reshape(n * 3, 3, 32, 32), S, return_float=True)
    assert _same_bits(gf, wf) and torch.equal(gq, wq) and torch.equal(gr, wr)
    # rows are ordered (pair, weight): row i W + 0 decodes a's latent, row i W + 2 b's
    ends = diff.decode(model, lat, S, return_float=True)[2]
    rows = gf.view(n, 3, 3, 32, 32)
    # (another batch size may take other kernels: each side is within the trajectory gate, 1e-5, of the exact chain)
    check("interpolate: weight 0 / 1 rows vs the decoded latents of a / b", torch.cat([rows[:, 0], rows[:, 2]]), ends, 2e-5)
    assert rel_l2(rows[:, 1], rows[:, 0]) > 1e-3
    assert len(diff.interpolate(model, a, b, torch.tensor(w), S)) == 2
    assert model.training and model._t_range is None


def test_interpolate_with_labels_repeats_them_per_weight(A, M):
    afdm, dev = A
    from afdm import ops
    _, model, diff = M
    n, S, w, s = 2, 3, [0.25, 0.75], 3.0
    labels = [4, afdm.NULL_LABEL]
    a, b = _images(n, 41, dev), _images(n, 42, dev)
    gf = diff.interpolate(model, a, b, w, S, refine=1, labels=labels, cfg_scale=s, return_float=True)[2]
    lat = diff.invert(model, torch.cat([a, b]), S, refine=1, labels=labels + labels, cfg_scale=s)
    mid = ops.slerp(lat[:n], lat[n:], w).reshape(n * 2, 3, 32, 32)
    wf = diff.decode(model, mid, S, labels=[4, 4, afdm.NULL_LABEL, afdm.NULL_LABEL], cfg_scale=s, return_float=True)[2]
    assert _same_bits(gf, wf)


# ---- 7. the model's state after an exception ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["invert", "decode", "sdedit", "interpolate"])
def test_methods_restore_the_model_after_an_exception(A, name):
    afdm, dev = A

    class Boom(afdm.UNet):
        calls = 0

        def forward(self, *a, **kw):
            Boom.calls += 1
            if Boom.calls == 3:
                raise RuntimeError("boom at the third forward")
            return super().forward(*a, **kw)

    afdm.set_seed(42)
    model = Boom(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    x = _images(2, 3, dev)
    call = {"invert": lambda: diff.invert(model, x, 3, refine=1), "decode": lambda: diff.decode(model, x, 4),
            "sdedit": lambda: diff.sdedit(model, x, 300, 4), "interpolate": lambda: diff.interpolate(model, x, x.flip(0), [0.5], 2, refine=1)}
    with pytest.raises(RuntimeError, match="third forward"):
        call[name]()
    torch.cuda.synchronize()
    assert Boom.calls == 3 and model.training and model._t_range is None


# ---- 8. from a checkpoint -----------------------------------------------------------------------------------------------------------------
def test_reconstruct_and_edit_results_from_a_checkpoint(A, M, tmp_path):
    afdm, dev = A
    model, _, diff = M
    path = tmp_path / "ckpt.pt"
    torch.save(model.state_dict(), path)
    data = {"args": afdm.argument(image_size=32, image_channels=3, device="cuda", noise_steps=T), "unet_v": 3, "seed": 42,
            "f_settings": dict(F_SET), "modelpath": str(path)}
    g = torch.Generator().manual_seed(1)
    pixels = torch.randint(0, 256, (3, 3, 32, 32), generator=g, dtype=torch.uint8)
    res = afdm.reconstruct_results(data, pixels, 2, steps=4)
    assert list(res) == ["n", "steps", "refine", "psnr", "ssim", "latent_std"]
    assert res["n"] == 2 and res["steps"] == 4 and res["refine"] == 0
    for key in ("psnr", "ssim"):
        assert list(res[key]) == ["mean", "std", "values"] and len(res[key]["values"]) == 2
        assert all(math.isfinite(v) for v in res[key]["values"] + [res[key]["mean"], res[key]["std"]])
    assert len(res["latent_std"]) == 2 and all(math.isfinite(v) and v > 0 for v in res["latent_std"])
    # the same numbers by hand, and through a DeviceDataset
    from afdm.data import normalisation_table
    x0 = normalisation_table(3)[torch.arange(3).view(1, 3, 1, 1), pixels[:2].long()].to(dev)            # as the loader maps pixels
    lat = diff.invert(model, x0, 4)
    q = afdm.image_quality(diff.decode(model, lat, 4)[0], pixels[:2].to(dev))
    assert res["psnr"]["values"] == q["psnr"].tolist() and res["ssim"]["values"] == q["ssim"].tolist()
    ds = afdm.DeviceDataset(pixels, device=dev)
    assert afdm.reconstruct_results(data, ds, 2, steps=[700, 300, 50, 2], refine=1)["steps"] == [700, 300, 50, 2]
    # edit_results is sdedit after the checkpoint's seed
    eq = afdm.edit_results(data, x0, 300, steps=3, noise_source="device")[0]
    afdm.set_seed(42)
    assert torch.equal(eq, diff.sdedit(model, x0, 300, 3, noise_source="device")[0])
