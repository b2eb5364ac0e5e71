"""GPU tests of consistency distillation: the three kernels against an fp64 restatement of the math (every element), the
defining property of the target, the boundary t = 0, the VEC and element-wise forms, the fused sampling step against its two
parts, self-consistency and the sampler on Gaussian data with a closed-form probability-flow ODE, a perfect student of a real
UNet teacher, ConsistencyStep against the inner TrainStep fed by hand in every launch mode, the models' state, a short training
run, the loop and ddpm_run."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
PAIRS = [(999, 998), (999, 500), (500, 499), (2, 1), (1, 0), (143, 0)]
KINDS = ("eps", "v", "x0")
LAYOUTS = ("vec", "odd", "offset", "inplace")


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


@pytest.fixture(scope="module", autouse=True)
def _leave_the_stream_pool_as_found(gpu):
    """torch.cuda.Stream() hands out a pool of 32 streams per device round-robin, and the steps and captures of this file take
    many.  Whether a later TrainStep's side stream happens to BE the stream torch captures on decides the fourth figure of its
    `lanes_counts` (14 or 26 for the same launches), which tests elsewhere compare between two steps.  So this
    file puts the pool's turn back where it found it: one full turn on the way in, and on the way out as many streams as it
    takes to come round to that turn's last one."""
    turn = [torch.cuda.Stream() for _ in range(32)]
    yield
    last = turn[-1].cuda_stream
    for _ in range(32):
        if torch.cuda.Stream().cuda_stream == last:
            break


def _model(afdm, dev, seed=42):
    afdm.set_seed(seed)
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _flat_of(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


# ---- the math of DESIGN.md 6zb, verbatim, in fp64 on the CPU -----------------------------------------------------------------------
def _level64(alpha_hat, t):
    """alpha_t, sigma_t of the rows t, (B, 1) fp64, from the fp32 table; the level t = 0 is alpha_hat[0], as afd_ddim_step reads it."""
    a = alpha_hat.double().cpu()[t]
    return torch.sqrt(a)[:, None], torch.sqrt(1.0 - a)[:, None]


def _coef64(coef, t):
    c = coef.double().cpu()[t]
    return c[:, 0:1], c[:, 1:2]


def _split64(kind, p, z, al, sg):
    """(x_hat, eps_hat) of the raw output p at z."""
    if kind == "eps":
        return (z - sg * p) / al, p
    if kind == "x0":
        return p, (z - al * p) / sg
    return al * z - sg * p, sg * z + al * p


def _fn64(kind, out, z, t, alpha_hat, coef):
    """f = c_skip z + c_out x_hat; z itself where c_out == 0, whatever `out` holds there."""
    al, sg = _level64(alpha_hat, t)
    cs, co = _coef64(coef, t)
    z = z.double().cpu()
    x, _ = _split64(kind, out.double().cpu(), z, al, sg)
    return torch.where(co == 0, z, cs * z + co * x)


def _target64(kind, out_tgt, z_prev, z_t, t, t_prev, alpha_hat, coef):
    al, sg = _level64(alpha_hat, t)
    cs, co = _coef64(coef, t)
    z = z_t.double().cpu()
    f = _fn64(kind, out_tgt, z_prev, t_prev, alpha_hat, coef)
    x = (f - cs * z) / co
    return x, (z - al * x) / sg, f


def _assert_every_element(fam, got, want, detail):
    """|got - want| <= 2^-23 |want| + 1e-9 for every element: both sides are fp64 evaluations of exact fp32 inputs, rounded once."""
    got = got.double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()), (fam, detail)
    excess = (got - want).abs() / (2.0 ** -23 * want.abs() + 1e-9)
    worst = float(excess.max())
    note(fam + " (worst |err| / gate, per element)", worst, detail)
    print(fam, detail, "worst |err| / (2^-23 |want| + 1e-9) =", worst, "max |want| =", float(want.abs().max()))
    assert worst <= 1.0, (fam, detail, worst, int(excess.argmax()))


def _rows(dev, pairs=PAIRS):
    tt = torch.tensor(pairs, dtype=torch.long)
    host = tuple(tt[:, i].contiguous() for i in range(2))
    return host, tuple(v.to(dev) for v in host)


def _setup(afdm, dev, **kw):
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **kw)
    return diff, diff.alpha_hat, diff.consistency_coefficients().to(dev)


# ---- 1 + 2. the kernels against the fp64 restatement, and the target's defining property ------------------------------------------
@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_consistency_kernels_equal_the_fp64_restatement(A, kind, layout, schedule):
    afdm, dev = A
    from afdm import ops
    diff, ah, coef = _setup(afdm, dev, schedule=schedule)
    (t, tp), (td, tpd) = _rows(dev)
    B = len(PAIRS)
    shape = (B, 3, 5, 7) if layout == "odd" else (B, 3, 32, 32)
    n = int(np.prod(shape))
    off = 1 if layout == "offset" else 0                              # every float operand 4 bytes past a 16-byte boundary
    g = torch.Generator().manual_seed(1000 + 100 * KINDS.index(kind) + 10 * LAYOUTS.index(layout) + (schedule == "cosine"))
    detail = (kind, layout, schedule)

    def buf(fill=None):
        v = torch.randn(n + off, generator=g) if fill is None else torch.full((n + off,), fill)
        return v.to(dev)[off:].view(shape)

    out, z_t, out_tgt, z_prev = buf(), buf(), buf(), buf()
    # consistency_fn at the rows' t and at their t_prev (two of those are the boundary 0)
    for rows, rows_dev, tag in ((t, td, "t"), (tp, tpd, "t_prev")):
        want = _fn64(kind, out.view(B, -1), z_t.view(B, -1), rows, ah, coef)
        if layout == "inplace":                                       # over out, then over z
            got = out.clone()
            assert ops.consistency_fn(got, z_t, rows_dev, ah, coef, kind, f_out=got) is got
            got_z = z_t.clone()
            ops.consistency_fn(out, got_z, rows_dev, ah, coef, kind, f_out=got_z)
            assert _same_bits(got, got_z), detail
        else:
            got = ops.consistency_fn(out, z_t, rows_dev, ah, coef, kind, f_out=buf(float("nan")))
        _assert_every_element(f"consistency_fn at {tag} vs fp64", got, want, detail)
    want_x, want_e, f_tgt = _target64(kind, out_tgt.view(B, -1), z_prev.view(B, -1), z_t.view(B, -1), t, tp, ah, coef)
    if layout == "inplace":                                           # eps_tilde over out_tgt, x_tilde over z_prev
        got_e, got_x = out_tgt.clone(), z_prev.clone()
        ops.consistency_target(got_e, got_x, z_t, td, tpd, ah, coef, kind, x_out=got_x, eps_out=got_e)
        got_x2 = z_t.clone()                                          # and x_tilde over z_t
        ops.consistency_target(out_tgt, z_prev, got_x2, td, tpd, ah, coef, kind, x_out=got_x2)
        assert _same_bits(got_x, got_x2), detail
    else:
        got_x, got_e = ops.consistency_target(out_tgt, z_prev, z_t, td, tpd, ah, coef, kind, x_out=buf(float("nan")),
                                              eps_out=buf(float("nan")))
    _assert_every_element("consistency_target x_tilde vs fp64", got_x, want_x, detail)
    _assert_every_element("consistency_target eps_tilde vs fp64", got_e, want_e, detail)
    # the defining property, in fp64 with the fp32 outputs: a student predicting x_tilde has f(z_t, t) = f_tgt, within the rounding
    # of x_tilde alone, 2^-24 c_out |x~| (+ 1e-9); and (x_tilde, eps_tilde) re-form z_t within 2^-24 (al |x~| + sg |eps~|) (+ 1e-9)
    al, sg = _level64(ah, t)
    cs, co = _coef64(coef, t)
    gx, ge, z = got_x.double().cpu().view(B, -1), got_e.double().cpu().view(B, -1), z_t.double().cpu().view(B, -1)
    miss_f = ((cs * z + co * gx) - f_tgt).abs() / (2.0 ** -24 * co * gx.abs() + 1e-9)
    miss_z = ((al * gx + sg * ge) - z).abs() / (2.0 ** -24 * (al * gx.abs() + sg * ge.abs()) + 1e-9)
    note("consistency_target: c_skip z_t + c_out x~ equals f_tgt (worst |err| / bound)", float(miss_f.max()), detail)
    note("consistency_target: al x~ + sg eps~ equals z_t (worst |err| / bound)", float(miss_z.max()), detail)
    print("defining property", detail, "f:", float(miss_f.max()), "z_t:", float(miss_z.max()))
    assert float(miss_f.max()) <= 1.0 and float(miss_z.max()) <= 1.0, (detail, float(miss_f.max()), float(miss_z.max()))
    torch.cuda.synchronize()


# ---- 3. the boundary ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 3, 32, 32), (6, 3, 5, 7)])
@pytest.mark.parametrize("kind", KINDS)
def test_boundary_rows_do_not_read_the_output(A, kind, shape):
    afdm, dev = A
    from afdm import ops
    diff, ah, coef = _setup(afdm, dev)
    (t, tp), (td, tpd) = _rows(dev)
    B = shape[0]
    g = torch.Generator().manual_seed(31 + KINDS.index(kind))
    out_tgt, z_prev, z_t = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
    at0 = (tp == 0).to(dev)
    assert int(at0.sum()) == 2
    poisoned = out_tgt.clone()
    poisoned[at0] = float("nan")
    poisoned[at0, 0] = float("inf")
    # consistency_fn at t = 0 returns z's bits, NaN / Inf in `out` or not; the other rows are what they are without the poison
    f = ops.consistency_fn(poisoned, z_prev, tpd, ah, coef, kind)
    assert _same_bits(f[at0], z_prev[at0]) and _same_bits(f, ops.consistency_fn(out_tgt, z_prev, tpd, ah, coef, kind))
    zeros = torch.zeros(B, device=dev, dtype=torch.long)
    assert _same_bits(ops.consistency_fn(torch.full_like(z_prev, float("nan")), z_prev, zeros, ah, coef, kind), z_prev)
    # the target: rows with t_prev == 0 take f_tgt = z_prev bit for bit, so x_tilde there is the fp64 expression of z_prev alone
    x, e = ops.consistency_target(poisoned, z_prev, z_t, td, tpd, ah, coef, kind)
    x_clean, e_clean = ops.consistency_target(out_tgt, z_prev, z_t, td, tpd, ah, coef, kind)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(e).all())
    assert _same_bits(x, x_clean) and _same_bits(e, e_clean)
    cs, co = _coef64(coef, t)
    want = (z_prev.double().cpu().view(B, -1) - cs * z_t.double().cpu().view(B, -1)) / co
    rows = at0.cpu()
    _assert_every_element("consistency_target at t_prev = 0: f_tgt is z_prev", x.view(B, -1)[at0], want[rows], (kind, shape))
    torch.cuda.synchronize()


# ---- 4. the VEC and element-wise forms ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_consistency_vec_and_elementwise_forms_agree_bit_for_bit(A, kind):
    afdm, dev = A
    from afdm import ops
    diff, ah, coef = _setup(afdm, dev)
    _, (td, tpd) = _rows(dev)
    shape = (len(PAIRS), 3, 32, 32)                                   # three segments of 256 quads per row
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(70 + KINDS.index(kind))
    data = [torch.randn(n, generator=g) for _ in range(5)]
    res = {}
    for off in (0, 1):                                                # aligned: 128-bit accesses; 4 bytes off: element by element
        out, z_t, out_tgt, z_prev, noise = (torch.cat([torch.zeros(off), v]).to(dev)[off:].view(shape) for v in data)
        assert out.data_ptr() % 16 == 4 * off
        fresh = lambda: torch.empty(n + off, device=dev)[off:].view(shape)
        f = ops.consistency_fn(out, z_t, td, ah, coef, kind, f_out=fresh())
        f0 = ops.consistency_fn(out, z_t, tpd, ah, coef, kind, f_out=fresh())
        x, e = ops.consistency_target(out_tgt, z_prev, z_t, td, tpd, ah, coef, kind, x_out=fresh(), eps_out=fresh())
        s = ops.consistency_step(out, z_t, noise, ah, coef, kind, 500, 143, x_out=fresh())
        s0 = ops.consistency_step(out, z_t, None, ah, coef, kind, 143, 0, x_out=fresh())
        res[off] = (f, f0, x, e, s, s0)
    for a, b, tag in zip(res[0], res[1], ("f", "f at t_prev", "x_tilde", "eps_tilde", "step", "last step")):
        assert _same_bits(a, b), (kind, tag)
    torch.cuda.synchronize()


# ---- 5. the fused step is consistency_fn followed by noise_images ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(6, 3, 32, 32), (3, 3, 5, 7)])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_step_has_the_bits_of_its_two_parts(A, kind, shape):
    afdm, dev = A
    from afdm import ops
    diff, ah, coef = _setup(afdm, dev, schedule="cosine" if kind == "v" else "linear")
    g = torch.Generator().manual_seed(50 + KINDS.index(kind) + shape[0])
    out, z, noise = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
    rows = lambda v: torch.full((shape[0],), v, device=dev, dtype=torch.long)
    for t, tn in PAIRS:
        f = ops.consistency_fn(out, z, rows(t), ah, coef, kind)
        if tn > 0:
            want = ops.noise_images(f, noise, rows(tn), ah)
            got = ops.consistency_step(out, z, noise, ah, coef, kind, t, tn)
        else:
            want = f
            got = ops.consistency_step(out, z, None, ah, coef, kind, t, tn)
            assert _same_bits(ops.consistency_step(out, z, noise, ah, coef, kind, t, tn), want)      # a noise given is not used
        assert _same_bits(got, want), (kind, shape, t, tn)
        for over in ("z", "out"):                                     # in place over z, as the sampler runs it, and over out
            o2, z2 = out.clone(), z.clone()
            dst = z2 if over == "z" else o2
            assert ops.consistency_step(o2, z2, noise if tn > 0 else None, ah, coef, kind, t, tn, x_out=dst) is dst
            assert _same_bits(dst, want), (kind, shape, t, tn, over)
        # the levels read on the device (what a captured step replays)
        got_dev = ops.consistency_step_dev(out, z, noise, ah, coef, kind, rows(t)[:1], rows(tn)[:1], torch.empty_like(z))
        assert _same_bits(got_dev, want), (kind, shape, t, tn, "dev")
    torch.cuda.synchronize()


# ---- 6 + 7. Gaussian data: x0 ~ N(mu, 0.5^2 I) has a closed-form probability-flow ODE ---------------------------------------------------
class _GaussEps(torch.nn.Module):
    """The exact eps of x0 ~ N(mu, 0.5^2 I) (test_gpu_dpm._GaussEps): sqrt(1 - a)(x - sqrt(a) mu) / (0.25 a + 1 - a), fp64 -> fp32."""

    def __init__(self, mu, alpha_hat):
        super().__init__()
        self.mu, self.ah = mu, alpha_hat.double()

    def forward(self, x, t):
        a = self.ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * self.mu) / (0.25 * a + 1 - a)).float()


def _f_star(mu, ah64, z, t):
    """The exact consistency function: the ODE's solution through (z, t) at level 0 (alpha_hat[0]), with v = 0.25 a + 1 - a:
    f*(z, t) = sqrt(a_0) mu + sqrt(v_0 / v_t) (z - sqrt(a_t) mu).  t: (B,) tensor; fp64."""
    a0, at = ah64[0], ah64[t].view(-1, 1, 1, 1)
    v0, vt = 0.25 * a0 + 1 - a0, 0.25 * at + 1 - at
    return a0.sqrt() * mu + (v0 / vt).sqrt() * (z.double() - at.sqrt() * mu)


class _ExactConsistency(torch.nn.Module):
    """The raw output of `kind` whose consistency function is f*: x_hat = (f* - c_skip z) / c_out in fp64, rounded once (zeros
    at t = 0, where the output is not read).  No host value in it: it captures into a graph."""

    def __init__(self, mu, alpha_hat, coef, kind):
        super().__init__()
        self.mu, self.ah, self.coef, self.kind = mu, alpha_hat.double(), coef, kind

    def forward(self, z, t):
        c = self.coef[t]
        cs, co = c[:, 0].view(-1, 1, 1, 1), c[:, 1].view(-1, 1, 1, 1)
        a = self.ah[t].view(-1, 1, 1, 1)
        al, sg = a.sqrt(), (1 - a).sqrt()
        z = z.double()
        x = (_f_star(self.mu, self.ah, z, t) - cs * z) / torch.where(co == 0, torch.ones_like(co), co)
        e = (z - al * x) / sg
        p = {"eps": e, "x0": x, "v": al * e - sg * x}[self.kind]
        return torch.where(co == 0, torch.zeros_like(p), p).float()


def _gauss(afdm, dev, kind="eps"):
    diff, ah, coef = _setup(afdm, dev, prediction=kind)
    g = torch.Generator().manual_seed(0)
    mu = (torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 1.6 - 0.8).to(dev)        # 4096 means in [-0.8, 0.8]
    return diff, ah, coef, mu


def test_self_consistency_error_is_second_order_in_the_gap(A):
    """The one test of the mathematics: with the exact teacher and the exact target network, f of the student's target x_tilde
    misses f*(z_t, t) by the one-step DDIM truncation error of t -> t_prev alone, second order in the gap.  In fp64 on the CPU
    (linear schedule) the ratios (gap 20) / (gap 10) are 4.15-4.23 and the residuals 5e-5 .. 3.5e-3, far above fp32 rounding."""
    afdm, dev = A
    from afdm import ops
    diff, ah, coef, mu = _gauss(afdm, dev)
    teacher, target = _GaussEps(mu, ah), _ExactConsistency(mu, ah, coef, "eps")
    B = 4
    g = torch.Generator().manual_seed(5)
    x0 = (mu.float().cpu() + 0.5 * torch.randn(B, 4, 32, 32, generator=g)).to(dev)
    eps = torch.randn(B, 4, 32, 32, generator=g).to(dev)
    for t in (400, 200, 100):
        res = {}
        for gap in (20, 10):
            td, tpd = (torch.full((B,), v, device=dev, dtype=torch.long) for v in (t, t - gap))
            z_t = ops.noise_images(x0, eps, td, ah)
            z_prev = ops.distill_mid(teacher(z_t, td), z_t, td, tpd, ah, "eps")
            x_tilde, _ = ops.consistency_target(target(z_prev, tpd), z_prev, z_t, td, tpd, ah, coef, "eps")
            c = coef[t].double()
            f = c[0] * z_t.double() + c[1] * x_tilde.double()
            res[gap] = rel_l2(f.cpu(), _f_star(mu, ah.double(), z_t, td).cpu())
        ratio = res[20] / res[10]
        note("self-consistency: truncation error ratio gap 20 / gap 10 (>= 3)", -ratio, t)
        print(f"self-consistency at t = {t}: residual gap 20 {res[20]:.3e}, gap 10 {res[10]:.3e}, ratio {ratio:.3f}")
        assert ratio >= 3, (t, res)
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ("v", "x0"))
def test_sampler_with_the_exact_model(A, kind):
    """(Not "eps": at t = 999 x_hat = (z - sg p) / al multiplies the fp32 rounding of the model's OUTPUT p by sg / al = 156, so
    2^-24 * 156 = 9.3e-6 of |p| is already in x_hat before the kernel runs -- the model's rounding, not the sampler's, and it
    leaves no room under the 1e-5 gate.  It is the instability ConsistencyStep warns about.)"""
    afdm, dev = A
    diff, ah, coef, mu = _gauss(afdm, dev, kind)
    model = _ExactConsistency(mu, ah, coef, kind)
    ah64 = ah.double()
    n, shape = 2, (2, 4, 32, 32)
    rows = lambda v: torch.full((n,), v, device=dev, dtype=torch.long)
    # one step: f* of the same x_T
    afdm.set_seed(11)
    xq, _, got = diff.consistency_sample(model, n, 4, [999], noise_source="device", return_float=True)
    afdm.set_seed(11)
    xT = torch.randn(shape, device=dev)
    check("consistency_sample, one step, exact model vs f*(x_T)", got.cpu(), _f_star(mu, ah64, xT, rows(999)).cpu(), 1e-5, kind)
    assert xq.dtype == torch.uint8 and tuple(xq.shape) == shape
    # three steps against a hand loop in fp64 fed the same noise
    steps = [999, 500, 100]
    afdm.set_seed(12)
    _, snaps, got3 = diff.consistency_sample(model, n, 4, steps, noise_source="device", return_float=True)
    afdm.set_seed(12)
    x = torch.randn(shape, device=dev).double()
    for t, tn in zip(steps, steps[1:] + [0]):
        x = _f_star(mu, ah64, x, rows(t))
        if tn > 0:
            x = ah64[tn].sqrt() * x + (1 - ah64[tn]).sqrt() * torch.randn(shape, device=dev).double()
    check("consistency_sample, three steps, exact model vs an fp64 hand loop", got3.cpu(), x.cpu(), 1e-5, kind)
    assert snaps.shape[0] == n * 4                                   # 999 -> 500, 500 -> 100 and 100 -> 0 cross a hundred; the final x
    # graph=True replays one captured step: the eager bits
    afdm.set_seed(12)
    _, _, got_g = diff.consistency_sample(model, n, 4, steps, noise_source="device", return_float=True, graph=True)
    assert _same_bits(got_g, got3), kind
    # an int S means ddim_timesteps(S)
    afdm.set_seed(13)
    a = diff.consistency_sample(model, n, 4, 3, noise_source="device", return_float=True)[2]
    afdm.set_seed(13)
    b = diff.consistency_sample(model, n, 4, diff.ddim_timesteps(3), noise_source="device", return_float=True)[2]
    assert _same_bits(a, b)
    torch.cuda.synchronize()


# ---- 8. a perfect student of a real teacher --------------------------------------------------------------------------------------------
class _PerfectStudent(torch.nn.Module):
    """At (z, t) of the teacher's chain: the teacher's whole remaining deterministic DDIM chain down to 0 with the sampler's own
    steps, then the raw output whose consistency function is that endpoint."""

    def __init__(self, teacher, diff, chain, coef):
        super().__init__()
        self.refs = (teacher, diff)                                   # (a tuple: the teacher is not a submodule)
        self.chain, self.coef = list(chain), coef
        self.calls = 0

    def forward(self, z, t):
        from afdm import ops
        teacher, diff = self.refs
        k = self.chain.index(int(t[0]))
        teacher.eval()
        x = z.clone()
        for ti, tn in zip(self.chain[k:], self.chain[k + 1:] + [0]):
            eps = diff.predict_eps(teacher, x, torch.full_like(t, ti))
            x = ops.ddim_step(x, eps, None, diff.alpha_hat, ti, tn, 0.0)
        c = self.coef[t].view(-1, 2, 1, 1, 1)
        a = diff.alpha_hat.double()[t].view(-1, 1, 1, 1)
        al, sg, z64 = a.sqrt(), (1 - a).sqrt(), z.double()
        x_hat = (x.double() - c[:, 0] * z64) / c[:, 1]
        e_hat = (z64 - al * x_hat) / sg
        self.calls += 1
        return {"eps": e_hat, "x0": x_hat, "v": al * e_hat - sg * x_hat}[diff.prediction].float()


@pytest.mark.parametrize("prediction", ("v", "x0"))
def test_perfect_student_reproduces_the_teacher_in_one_step(A, prediction):
    afdm, dev = A
    diff, ah, coef = _setup(afdm, dev, prediction=prediction)
    teacher = _model(afdm, dev)
    chain = diff.ddim_timesteps(8)
    afdm.set_seed(3)
    _, _, want = diff.sample(teacher, n=2, image_channels=3, steps=chain, noise_source="cpu", return_float=True)
    student = _PerfectStudent(teacher, diff, chain, coef)
    afdm.set_seed(3)
    _, _, got = diff.consistency_sample(student, 2, 3, [chain[0]], noise_source="cpu", return_float=True)
    assert student.calls == 1 and bool(torch.isfinite(want).all())
    e = rel_l2(got.cpu(), want.cpu())
    print("perfect student, 1 consistency step vs the teacher's 8 DDIM steps:", prediction, "rel-L2", e, "max |x|", float(want.abs().max()))
    check("perfect 1-step consistency student vs the teacher's 8-step sample", got.cpu(), want.cpu(), 1e-5, prediction)


# ---- 9. ConsistencyStep is the inner step on the distilled batch ---------------------------------------------------------------------
_K = torch.tensor([0, 7, 3, 5])                                      # position 7 is the chain's last: t_prev = 0
_DIFF_KW = dict(schedule="cosine", prediction="v")
_eager = {}


def _step_inputs(dev):
    g = torch.Generator().manual_seed(11)
    images = (torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    eps = [torch.randn(4, 3, 32, 32, generator=g).to(dev) for _ in range(3)]
    return images, eps


def _run_consistency_step(afdm, dev, mode):
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **_DIFF_KW)
    teacher = _model(afdm, dev)
    student = copy.deepcopy(teacher)
    images, eps = _step_inputs(dev)
    before = [p.detach().clone() for p in teacher.parameters()]
    step = afdm.ConsistencyStep(student, teacher, diff, diff.ddim_timesteps(8), lr=1e-4, graph=mode)
    assert isinstance(step.step, afdm.TrainStep) and step.step.loss_weighting == "truncated_snr"
    assert step.target is not student and step.target is not teacher and step.step.ema.beta == 0.95 and step.n_steps == 8
    losses = [step(images, k=_K, eps=e).clone() for e in eps]
    torch.cuda.synchronize()
    assert all(_same_bits(a, b.detach()) for a, b in zip(before, teacher.parameters()))      # the teacher is frozen
    assert all(p.grad is None for p in teacher.parameters())
    return torch.stack(losses), step.step.opt.fp.flat.clone(), _flat_of(step.target).clone()


def test_consistency_step_is_the_inner_step_on_the_distilled_batch(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **_DIFF_KW)
    chain = diff.ddim_timesteps(8)
    coef = diff.consistency_coefficients().to(dev)
    teacher = _model(afdm, dev)
    hand = copy.deepcopy(teacher)
    hand_target = copy.deepcopy(hand)
    images, eps = _step_inputs(dev)
    # the first call's loss, restated in fp64 from the student's own prediction
    x, e, t = diff.consistency_targets(teacher, hand_target, images, _K, chain, coef, eps[0])
    assert t.tolist() == [chain[int(k)] for k in _K] and not x.requires_grad and not e.requires_grad
    with torch.no_grad():
        pred = hand(diff.noise_images(x, t, e)[0], t).double().cpu()
    w = diff.snr_weights("truncated_snr").float().double()[t.cpu()]
    target = diff.training_target(x.double().cpu(), e.double().cpu(), t.cpu())
    want0 = float((w[:, None, None, None] * (pred - target) ** 2).mean())
    ref = afdm.TrainStep(hand, diff, 1e-4, loss_weighting="truncated_snr", ema=afdm.EMA(0.95), ema_model=hand_target, ema_start=0)
    want = []
    for ep in eps:
        x, e, t = diff.consistency_targets(teacher, hand_target, images, _K, chain, coef, ep)
        want.append(ref(x, t, e).clone())
    torch.cuda.synchronize()
    got_losses, got_flat, got_target = _eager["run"] = _run_consistency_step(afdm, dev, False)
    rel = abs(float(got_losses[0]) - want0) / want0
    note("ConsistencyStep: first loss vs fp64 restatement (rel)", rel)
    print("ConsistencyStep losses", got_losses.tolist(), "fp64 restatement of the first", want0, "rel", rel)
    assert rel < 1e-5, (float(got_losses[0]), want0)
    assert _same_bits(got_losses, torch.stack(want)) and _same_bits(got_flat, ref.opt.fp.flat)
    assert _same_bits(got_target, _flat_of(hand_target))
    assert not _same_bits(got_flat[:1000], _flat_of(teacher)[:1000])                          # it did train,
    assert not _same_bits(got_target[:1000], _flat_of(teacher)[:1000])                        # the target network follows
    assert not _same_bits(got_target[:1000], got_flat[:1000])                                 # at its own rate


@pytest.mark.parametrize("mode", (True, "lanes"))
def test_consistency_step_in_every_launch_mode(A, mode):
    afdm, dev = A
    if "run" not in _eager:
        _eager["run"] = _run_consistency_step(afdm, dev, False)
    got = _run_consistency_step(afdm, dev, mode)
    for a, b, tag in zip(got, _eager["run"], ("losses", "parameters", "target network")):
        assert _same_bits(a, b), (mode, tag)


# ---- 10. state ---------------------------------------------------------------------------------------------------------------------------
def test_consistency_targets_restore_both_models(A):
    afdm, dev = A
    diff, ah, coef = _setup(afdm, dev, prediction="x0")
    teacher = _model(afdm, dev)
    target = copy.deepcopy(teacher)
    chain = diff.ddim_timesteps(8)
    images = torch.zeros(2, 3, 32, 32, device=dev)
    k = torch.tensor([0, 7])
    seen = []
    hooks = [m.register_forward_pre_hook(lambda m, a, tag=tag: seen.append((tag, m.training, m._t_range)))
             for tag, m in (("teacher", teacher), ("target", target))]
    for tr_teacher, tr_target in ((True, False), (False, True)):
        teacher.train(tr_teacher)
        target.train(tr_target)
        x, e, t = diff.consistency_targets(teacher, target, images, k, chain, coef)
        assert teacher.training is tr_teacher and target.training is tr_target
        assert teacher._t_range is None and target._t_range is None
        assert not x.requires_grad and not e.requires_grad and t.tolist() == [999, 1]
    assert seen == [("teacher", False, 1000), ("target", False, 1000)] * 2      # one forward each per call: eval mode, hinted
    for h in hooks:
        h.remove()

    def boom(*a, **kw):
        raise RuntimeError("forward failed")

    for broken in (teacher, target):
        teacher.train(True)
        target.train(False)
        broken.forward = boom
        with pytest.raises(RuntimeError, match="forward failed"):
            diff.consistency_targets(teacher, target, images, k, chain, coef)
        assert teacher.training is True and target.training is False
        assert teacher._t_range is None and target._t_range is None
        del broken.forward
    # a step leaves its models as it found them, too
    step = afdm.ConsistencyStep(copy.deepcopy(teacher), teacher, diff, chain, 1e-4)
    step.target.train(False)
    assert math.isfinite(float(step(images + 0.1, k=k)))
    assert teacher.training is True and step.target.training is False and teacher._t_range is None
    torch.cuda.synchronize()


def test_eps_prediction_logs_one_warning(A, caplog):
    afdm, dev = A
    teacher = _model(afdm, dev)
    for prediction, n in (("eps", 1), ("v", 0)):
        diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction=prediction)
        caplog.clear()
        with caplog.at_level("WARNING"):
            afdm.ConsistencyStep(copy.deepcopy(teacher), teacher, diff, diff.ddim_timesteps(4), 1e-4)
        assert sum("prediction='eps' is unstable" in r.getMessage() for r in caplog.records) == n


# ---- 11. it trains ----------------------------------------------------------------------------------------------------------------------
def test_consistency_distillation_lowers_the_loss_on_a_fixed_batch(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="v")
    teacher = _model(afdm, dev)
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(8, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    eps = torch.randn(8, 3, 32, 32, generator=g).to(dev)
    chain = diff.ddim_timesteps(8)
    # every row at the chain's last position: t_prev = 0, so the target is the teacher's z_prev and does not move with the target network
    step = afdm.ConsistencyStep(copy.deepcopy(teacher), teacher, diff, chain, lr=1e-4)
    k = torch.full((8,), len(chain) - 1)
    losses = [float(step(images, k=k, eps=eps)) for _ in range(30)]
    print("consistency distillation at the last position, one fixed batch, 30 steps at lr 1e-4: first loss", losses[0], "last", losses[-1])
    note("consistency distillation on a fixed batch: last / first loss", losses[-1] / losses[0])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    mixed = afdm.ConsistencyStep(copy.deepcopy(teacher), teacher, diff, chain, lr=1e-4)
    km = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7])
    lm = [float(mixed(images, k=km, eps=eps)) for _ in range(6)]
    print("mixed positions, 6 steps:", lm)
    assert all(math.isfinite(v) for v in lm), lm
    assert bool(torch.isfinite(_flat_of(mixed.target)).all())


# ---- 12. the loop and ddpm_run ------------------------------------------------------------------------------------------------------------
def test_consistency_distill_returns_the_target_network(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="v")
    model = _model(afdm, dev)
    before = _flat_of(model).clone()
    g = torch.Generator().manual_seed(9)
    loader = [(torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, torch.zeros(2)) for _ in range(3)]       # 3 batches, cycled
    seen = []
    afdm.set_seed(1)
    net, info = afdm.consistency_distill(model, diff, loader, 8, 4, 1e-4, dev, target_beta=0.5,
                                         on_done=lambda info, s, tgt: seen.append((info, s, tgt)))
    torch.cuda.synchronize()
    assert info["chain"] == diff.ddim_timesteps(8) and math.isfinite(info["mean_loss"]) and info["mean_loss"] > 0
    assert len(seen) == 1 and seen[0][0] is info and seen[0][2] is net and seen[0][1] is not net
    assert net is not model and seen[0][1] is not model
    assert _same_bits(_flat_of(model), before)                        # the teacher is left as it was
    assert not _same_bits(_flat_of(net), before) and not _same_bits(_flat_of(net), _flat_of(seen[0][1]))
    for steps in ([999], 2):
        xq, _ = diff.consistency_sample(net, 2, 3, steps)
        assert xq.dtype == torch.uint8 and tuple(xq.shape) == (2, 3, 32, 32)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_ddpm_run_with_consistency(A, tmp_path, monkeypatch):
    afdm, dev = A
    rng = np.random.default_rng(0)
    csvp = tmp_path / "mnist.csv"
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    np.savetxt(csvp, arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
    params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
              "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(csvp),
              "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
              "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42, "prediction": "v"}
    runs = {}
    for key, extra in (("plain", {}), ("consistency", {"consistency": {"steps": 4, "iters": 2, "sample_steps": 2}})):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        runs[key] = (afdm.ddpm_run(dict(params, **extra)), _files(wd))
    (plain, plain_files), (out, files) = runs["plain"], runs["consistency"]
    assert "consistency" not in plain and not any("consistency" in f for f in plain_files)
    new = "models/DDPM_Uncondtional_MNIST_3/ckpt_MNIST_3_consistency4.pt"
    assert files == sorted(plain_files + [new])                       # the same file set, plus the consistency model
    c = out["consistency"]
    assert c["modelpath"] == str(tmp_path / "consistency" / new) and c["sample_steps"] == 2
    assert c["chain"] == [11, 7, 4, 1] and math.isfinite(c["mean_loss"])
    sd = torch.load(c["modelpath"], weights_only=True)
    ck = torch.load(out["modelpath"], weights_only=True)
    assert sd.keys() == ck.keys() and any(not torch.equal(sd[k], ck[k]) for k in sd)
    assert len([f for f in files if f.startswith("images/generated/MNIST_3/")]) == len(
        [f for f in plain_files if f.startswith("images/generated/MNIST_3/")])
