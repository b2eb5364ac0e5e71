"""GPU tests of progressive distillation: the two target kernels against an fp64 restatement of the math (every element), their
VEC and element-wise forms, the existing sampler's steps, a student that reproduces its teacher exactly, DistillStep against the
inner TrainStep fed by hand in every launch mode, the teacher's state, a short training run, the loop and ddpm_run."""
import copy
import math
import os

import numpy as np
import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
TRIPLES = [(999, 998, 997), (999, 500, 1), (500, 499, 498), (3, 2, 1), (2, 1, 0)]
KINDS = ("eps", "v", "x0")
LAYOUTS = ("vec", "odd", "offset", "inplace")
# test_perfect_student_reproduces_the_teacher: 10 x the worst rel-L2 of the first run on an MI355X (PERFECT_MEASURED)
PERFECT_MEASURED = 8.52e-7           # x0; 6.53e-7 for v
PERFECT_GATE = 10 * PERFECT_MEASURED


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42):
    afdm.set_seed(seed)
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the math of DESIGN.md 6l, verbatim, in fp64 on the CPU ---------------------------------------------------------------------------
def _level64(alpha_hat, t):
    """alpha_t, sigma_t of the rows t, (B, 1) fp64, from the fp32 table.  The level t = 0 follows the DDIM sampler's convention:
    afd_ddim_step reads alpha_hat[0] for t_prev = 0 (not a := 1), and the student is sampled with that step."""
    a = alpha_hat.double().cpu()[t]
    return torch.sqrt(a)[:, None], torch.sqrt(1.0 - a)[:, None]


def _split64(kind, p, z, al, sg):
    """(x_hat, eps_hat) of the raw output p at z."""
    if kind == "eps":
        return (z - sg * p) / al, p
    if kind == "x0":
        return p, (z - al * p) / sg
    return al * z - sg * p, sg * z + al * p


def _mid64(kind, out1, z_t, t, t_mid, alpha_hat):
    al, sg = _level64(alpha_hat, t)
    al1, sg1 = _level64(alpha_hat, t_mid)
    x1, e1 = _split64(kind, out1.double().cpu(), z_t.double().cpu(), al, sg)
    return al1 * x1 + sg1 * e1


def _target64(kind, out2, z_mid, z_t, t, t_mid, t_prev, alpha_hat):
    al, sg = _level64(alpha_hat, t)
    al1, sg1 = _level64(alpha_hat, t_mid)
    al2, sg2 = _level64(alpha_hat, t_prev)
    z = z_t.double().cpu()
    x2, e2 = _split64(kind, out2.double().cpu(), z_mid.double().cpu(), al1, sg1)
    z2 = al2 * x2 + sg2 * e2
    r = sg2 / sg
    x = (z2 - r * z) / (al2 - r * al)
    return x, (z - al * x) / sg


def _assert_every_element(fam, got, want, detail):
    """|got - want| <= 2^-23 |want| + 1e-9 for every element: both sides are fp64 evaluations of exact fp32 inputs, rounded once."""
    got = got.double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all()), (fam, detail)
    excess = (got - want).abs() / (2.0 ** -23 * want.abs() + 1e-9)
    worst = float(excess.max())
    note(fam + " (worst |err| / gate, per element)", worst, detail)
    print(fam, detail, "worst |err| / (2^-23 |want| + 1e-9) =", worst, "max |want| =", float(want.abs().max()))
    assert worst <= 1.0, (fam, detail, worst, int(excess.argmax()))


def _rows(dev, triples=TRIPLES):
    tt = torch.tensor(triples, dtype=torch.long)
    host = tuple(tt[:, i].contiguous() for i in range(3))
    return host, tuple(v.to(dev) for v in host)


# ---- 1. the kernels against the fp64 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", KINDS)
def test_distill_kernels_equal_the_fp64_restatement(A, kind, layout, schedule):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule)
    ah = diff.alpha_hat
    (t, tm, tp), (td, tmd, tpd) = _rows(dev)
    B = len(TRIPLES)
    shape = (B, 3, 5, 7) if layout == "odd" else (B, 3, 32, 32)
    n = int(np.prod(shape))
    off = 1 if layout == "offset" else 0                              # every float operand 4 bytes past a 16-byte boundary
    g = torch.Generator().manual_seed(100 * KINDS.index(kind) + 10 * LAYOUTS.index(layout) + (schedule == "cosine"))

    def buf(fill=None):
        v = torch.randn(n + off, generator=g) if fill is None else torch.full((n + off,), fill)
        return v.to(dev)[off:].view(shape)

    out1, z_t, out2 = buf(), buf(), buf()
    want_mid = _mid64(kind, out1.view(B, -1), z_t.view(B, -1), t, tm, ah)
    if layout == "inplace":                                           # z_mid over out1
        z_mid = out1.clone()
        assert ops.distill_mid(z_mid, z_t, td, tmd, ah, kind, out=z_mid) is z_mid
    else:
        z_mid = ops.distill_mid(out1, z_t, td, tmd, ah, kind, out=buf(float("nan")))
    _assert_every_element("distill_mid vs fp64", z_mid, want_mid, (kind, layout, schedule))
    # the second kernel takes the first one's fp32 z_mid, as the step does
    want_x, want_e = _target64(kind, out2.view(B, -1), z_mid.view(B, -1), z_t.view(B, -1), t, tm, tp, ah)
    if layout == "inplace":                                           # eps_tilde over out2, x_tilde over z_mid
        got_e, got_x = out2.clone(), z_mid.clone()
        ops.distill_target(got_e, got_x, z_t, td, tmd, tpd, ah, kind, x_out=got_x, eps_out=got_e)
    else:
        got_x, got_e = ops.distill_target(out2, z_mid, z_t, td, tmd, tpd, ah, kind, x_out=buf(float("nan")), eps_out=buf(float("nan")))
    _assert_every_element("distill_target x_tilde vs fp64", got_x, want_x, (kind, layout, schedule))
    _assert_every_element("distill_target eps_tilde vs fp64", got_e, want_e, (kind, layout, schedule))
    # and in fp64 one DDIM step from z_t with the fp32 (x_tilde, eps_tilde) lands on the teacher's z_prev
    al2, sg2 = _level64(ah, tp)
    al1, sg1 = _level64(ah, tm)
    x2, e2 = _split64(kind, out2.double().cpu().view(B, -1), z_mid.double().cpu().view(B, -1), al1, sg1)
    # within what rounding x_tilde and eps_tilde to fp32 allows: 2^-24 (al'' |x~| + sg'' |eps~|) per element (+ 1e-9 for fp64)
    gx, ge = got_x.double().cpu().view(B, -1), got_e.double().cpu().view(B, -1)
    miss = ((al2 * gx + sg2 * ge) - (al2 * x2 + sg2 * e2)).abs() / (2.0 ** -24 * (al2 * gx.abs() + sg2 * ge.abs()) + 1e-9)
    note("distill_target: one DDIM step of (x~, eps~) lands on z_prev (worst |err| / bound)", float(miss.max()), (kind, layout, schedule))
    assert float(miss.max()) <= 1.0, (kind, layout, schedule, float(miss.max()))
    torch.cuda.synchronize()


# ---- 2. the VEC and element-wise forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_distill_vec_and_elementwise_forms_agree_bit_for_bit(A, kind):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat
    _, (td, tmd, tpd) = _rows(dev)
    B, shape = len(TRIPLES), (len(TRIPLES), 3, 32, 32)
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(7 + KINDS.index(kind))
    data = [torch.randn(n, generator=g) for _ in range(3)]
    res = {}
    for off in (0, 1):                                                # aligned: 128-bit accesses; 4 bytes off: element by element
        out1, z_t, out2 = (torch.cat([torch.zeros(off), v]).to(dev)[off:].view(shape) for v in data)
        assert out1.data_ptr() % 16 == 4 * off
        z_mid = ops.distill_mid(out1, z_t, td, tmd, ah, kind, out=torch.empty(n + off, device=dev)[off:].view(shape))
        x, e = ops.distill_target(out2, z_mid, z_t, td, tmd, tpd, ah, kind, x_out=torch.empty(n + off, device=dev)[off:].view(shape),
                                  eps_out=torch.empty(n + off, device=dev)[off:].view(shape))
        res[off] = (z_mid, x, e)
    for a, b, tag in zip(res[0], res[1], ("z_mid", "x_tilde", "eps_tilde")):
        assert _same_bits(a, b), (kind, tag)
    # a ragged row (chw = 105: 26 quads and one float) against the same rows cut out of a longer, aligned run is not expressible
    # (the row stride differs), so the odd size is covered against fp64 above; here: several segments per row and more than one
    # workgroup per row (chw = 3 * 32 * 32 = 3 segments of 256 quads)
    torch.cuda.synchronize()


# ---- 3. against the existing sampler's fp32 steps ----------------------------------------------------------------------------------------
def _parent_ddim(afdm, diff, kind, out, z, t, t_prev):
    """One deterministic DDIM step of the raw output `out` at z with the parent's fp32 code: pred_to_eps + ddim_step."""
    from afdm import ops
    tt = torch.full((z.shape[0],), t, device=z.device, dtype=torch.long)
    eps = out if kind == "eps" else ops.pred_to_eps(out.clone(), z, tt, diff.alpha_hat, kind)
    return ops.ddim_step(z, eps, None, diff.alpha_hat, t, t_prev, 0.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("group", [(999, 856, 713), (500, 499, 498), (143, 1, 0), (2, 1, 0)])
def test_distill_kernels_against_the_existing_sampler(A, kind, group):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat
    t, tm, tp = group
    B, shape = 3, (3, 3, 8, 8)
    g = torch.Generator().manual_seed(sum(group) + KINDS.index(kind))
    out1, z_t, out2 = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
    td, tmd, tpd = (torch.full((B,), v, device=dev, dtype=torch.long) for v in group)
    z_mid = ops.distill_mid(out1, z_t, td, tmd, ah, kind)
    want_mid = _parent_ddim(afdm, diff, kind, out1, z_t, t, tm)
    check("distill_mid vs pred_to_eps + ddim_step (fp32)", z_mid.cpu(), want_mid.cpu(), 1e-5, (kind, group))
    # the defining property, with the sampler's own step: from z_t with eps_tilde it lands on the hand-composed z_prev
    x, e = ops.distill_target(out2, z_mid, z_t, td, tmd, tpd, ah, kind)
    z_prev = _parent_ddim(afdm, diff, kind, out2, want_mid, tm, tp)
    landed = ops.ddim_step(z_t, e, None, ah, t, tp, 0.0)
    check("ddim_step(z_t, eps_tilde) vs two hand-composed steps", landed.cpu(), z_prev.cpu(), 1e-5, (kind, group))
    assert bool(torch.isfinite(x).all())
    torch.cuda.synchronize()


# ---- 4. a perfect student reproduces the teacher ---------------------------------------------------------------------------------------
class _PerfectStudent(torch.nn.Module):
    """At (z, t) of the student's chain: the teacher's two steps and both kernels -> training_target(x_tilde, eps_tilde, t)."""

    def __init__(self, teacher, diff, chain):
        super().__init__()
        self.refs = (teacher, diff)                                   # (a tuple: the teacher is not a submodule)
        self.levels = diff.distill_levels(chain)
        self.calls = 0

    def forward(self, z, t):
        from afdm import ops
        teacher, diff = self.refs
        k = self.levels[0].tolist().index(int(t[0]))
        tm, tp = (torch.full_like(t, int(tab[k])) for tab in self.levels[1:])
        teacher.eval()
        out1 = teacher(z, t)
        z_mid = ops.distill_mid(out1, z, t, tm, diff.alpha_hat, diff.prediction)
        out2 = teacher(z_mid, tm)
        x, e = ops.distill_target(out2, z_mid, z, t, tm, tp, diff.alpha_hat, diff.prediction)
        self.calls += 1
        return diff.training_target(x, e, t)


@pytest.mark.parametrize("prediction", ("v", "x0"))
def test_perfect_student_reproduces_the_teacher(A, prediction):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction=prediction)
    teacher = _model(afdm, dev)
    chain = diff.ddim_timesteps(8)
    afdm.set_seed(3)
    _, _, want = diff.sample(teacher, n=2, image_channels=3, steps=chain, noise_source="cpu", return_float=True)
    student = _PerfectStudent(teacher, diff, chain)
    afdm.set_seed(3)
    _, _, got = diff.sample(student, n=2, image_channels=3, steps=diff.halve_chain(chain), noise_source="cpu", return_float=True)
    assert student.calls == 4 and bool(torch.isfinite(want).all())
    e = rel_l2(got.cpu(), want.cpu())
    print("perfect student, 4 steps vs the teacher's 8:", prediction, "rel-L2", e, "max |x|", float(want.abs().max()))
    check("perfect 4-step student vs the teacher's 8-step sample", got.cpu(), want.cpu(), PERFECT_GATE, prediction)


# ---- 5. DistillStep is the inner step on the distilled batch ---------------------------------------------------------------------------
_K = torch.tensor([0, 3, 1, 2])
_DIFF_KW = dict(schedule="cosine", prediction="v")
_eager = {}


def _step_inputs(dev):
    g = torch.Generator().manual_seed(11)
    images = (torch.rand(4, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    eps = [torch.randn(4, 3, 32, 32, generator=g).to(dev) for _ in range(3)]
    return images, eps


def _run_distill_step(afdm, dev, mode):
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **_DIFF_KW)
    teacher = _model(afdm, dev)
    student = copy.deepcopy(teacher)
    images, eps = _step_inputs(dev)
    before = [p.detach().clone() for p in teacher.parameters()]
    step = afdm.DistillStep(student, teacher, diff, diff.ddim_timesteps(8), lr=1e-4, graph=mode)
    assert isinstance(step.step, afdm.TrainStep) and step.step.loss_weighting == "truncated_snr"
    losses = [step(images, k=_K, eps=e).clone() for e in eps]
    torch.cuda.synchronize()
    assert all(_same_bits(a, b.detach()) for a, b in zip(before, teacher.parameters()))      # the teacher is frozen
    assert all(p.grad is None for p in teacher.parameters())
    return torch.stack(losses), step.step.opt.fp.flat.clone()


def test_distill_step_is_the_inner_step_on_the_distilled_batch(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **_DIFF_KW)
    chain = diff.ddim_timesteps(8)
    teacher = _model(afdm, dev)
    hand = copy.deepcopy(teacher)
    images, eps = _step_inputs(dev)
    # the first call's loss, restated in fp64 from the student's own prediction
    x, e, t = diff.distill_targets(teacher, images, _K, chain, eps[0])
    assert t.tolist() == [chain[2 * int(k)] for k in _K]
    with torch.no_grad():
        pred = hand(diff.noise_images(x, t, e)[0], t).double().cpu()
    w = diff.snr_weights("truncated_snr").float().double()[t.cpu()]
    target = diff.training_target(x.double().cpu(), e.double().cpu(), t.cpu())
    want0 = float((w[:, None, None, None] * (pred - target) ** 2).mean())
    ref = afdm.TrainStep(hand, diff, 1e-4, loss_weighting="truncated_snr")
    want = []
    for ep in eps:
        x, e, t = diff.distill_targets(teacher, images, _K, chain, ep)
        want.append(ref(x, t, e).clone())
    torch.cuda.synchronize()
    got_losses, got_flat = _eager["run"] = _run_distill_step(afdm, dev, False)
    rel = abs(float(got_losses[0]) - want0) / want0
    note("DistillStep: first loss vs fp64 restatement (rel)", rel)
    print("DistillStep losses", got_losses.tolist(), "fp64 restatement of the first", want0, "rel", rel)
    assert rel < 1e-5, (float(got_losses[0]), want0)
    assert _same_bits(got_losses, torch.stack(want)) and _same_bits(got_flat, ref.opt.fp.flat)
    assert not _same_bits(got_flat[:1000], _flat_of(teacher)[:1000])                          # and it did train


def _flat_of(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


@pytest.mark.parametrize("mode", (True, "lanes"))
def test_distill_step_in_every_launch_mode(A, mode):
    afdm, dev = A
    if "run" not in _eager:
        _eager["run"] = _run_distill_step(afdm, dev, False)
    losses, flat = _run_distill_step(afdm, dev, mode)
    assert _same_bits(losses, _eager["run"][0]) and _same_bits(flat, _eager["run"][1]), mode


# ---- 6. state ---------------------------------------------------------------------------------------------------------------------------
def test_distill_targets_restore_the_teacher(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="x0")
    teacher = _model(afdm, dev)
    chain = diff.ddim_timesteps(8)
    images = torch.zeros(2, 3, 32, 32, device=dev)
    k = torch.tensor([0, 3])
    seen = []
    hook = teacher.register_forward_pre_hook(lambda m, a: seen.append((m.training, m._t_range)))
    for training in (True, False):
        teacher.train(training)
        x, e, t = diff.distill_targets(teacher, images, k, chain)
        assert teacher.training is training and teacher._t_range is None
        assert not x.requires_grad and not e.requires_grad and t.tolist() == [999, 143]
    assert seen == [(False, 1000)] * 4                                # both forwards of both calls: eval mode, hinted
    hook.remove()

    def boom(*a, **kw):
        raise RuntimeError("forward failed")

    teacher.train(True)
    teacher.forward = boom
    with pytest.raises(RuntimeError, match="forward failed"):
        diff.distill_targets(teacher, images, k, chain)
    assert teacher.training is True and teacher._t_range is None
    del teacher.forward
    # argument errors
    with pytest.raises(ValueError, match="student is teacher"):
        afdm.DistillStep(teacher, teacher, diff, chain, 1e-4)
    with pytest.raises(ValueError, match="even number of steps"):
        afdm.DistillStep(copy.deepcopy(teacher), teacher, diff, diff.ddim_timesteps(7), 1e-4)
    lv = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="x0", variance="learned")
    with pytest.raises(ValueError, match="variance='learned'"):
        afdm.DistillStep(copy.deepcopy(teacher), teacher, lv, chain, 1e-4)
    with pytest.raises(ValueError, match="variance='learned'"):
        lv.distill_targets(teacher, images, k, chain)
    torch.cuda.synchronize()


def test_eps_prediction_logs_one_warning(A, caplog):
    afdm, dev = A
    teacher = _model(afdm, dev)
    for prediction, n in (("eps", 1), ("v", 0)):
        diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction=prediction)
        caplog.clear()
        with caplog.at_level("WARNING"):
            afdm.DistillStep(copy.deepcopy(teacher), teacher, diff, diff.ddim_timesteps(4), 1e-4)
        assert sum("prediction='eps' is unstable" in r.getMessage() for r in caplog.records) == n


# ---- 7. it trains -----------------------------------------------------------------------------------------------------------------------
def test_distillation_lowers_the_loss_on_a_fixed_batch(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="v")
    teacher = _model(afdm, dev)
    student = copy.deepcopy(teacher)
    g = torch.Generator().manual_seed(5)
    images = (torch.rand(8, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    eps = torch.randn(8, 3, 32, 32, generator=g).to(dev)
    k = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3])
    step = afdm.DistillStep(student, teacher, diff, diff.ddim_timesteps(8), lr=1e-4)
    losses = [float(step(images, k=k, eps=eps)) for _ in range(30)]
    print("distillation 8 -> 4 on one fixed batch, 30 steps at lr 1e-4: first loss", losses[0], "last", losses[-1])
    note("distillation on a fixed batch: last / first loss", losses[-1] / losses[0])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses


# ---- 8. the loop and ddpm_run ------------------------------------------------------------------------------------------------------------
def test_progressive_distill_halves_round_after_round(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="v")
    model = _model(afdm, dev)
    before = _flat_of(model).clone()
    g = torch.Generator().manual_seed(9)
    loader = [(torch.rand(2, 3, 32, 32, generator=g) * 2 - 1, torch.zeros(2)) for _ in range(3)]       # 3 batches, cycled
    seen = []
    afdm.set_seed(1)
    student, rounds = afdm.progressive_distill(model, diff, loader, 8, 2, 2, 1e-4, dev, ema_beta=0.5,
                                               on_round=lambda info, s, ema: seen.append((info["steps"], s, ema)))
    torch.cuda.synchronize()
    c8 = diff.ddim_timesteps(8)
    assert [r["steps"] for r in rounds] == [4, 2] and [r["chain"] for r in rounds] == [c8[0::2], c8[0::4]]
    assert all(math.isfinite(r["mean_loss"]) and r["mean_loss"] > 0 for r in rounds)
    assert [s[0] for s in seen] == [4, 2] and seen[1][1] is student and student is not model and seen[0][2] is not None
    assert _same_bits(_flat_of(model), before)                        # the first teacher is left as it was
    assert not _same_bits(_flat_of(student), before)
    xq, _ = diff.sample(student, n=2, image_channels=3, steps=rounds[-1]["chain"])
    assert xq.dtype == torch.uint8 and tuple(xq.shape) == (2, 3, 32, 32)


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_ddpm_run_with_distill(A, tmp_path, monkeypatch):
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
    for key, extra in (("plain", {}), ("distill", {"distill": {"start_steps": 4, "end_steps": 2, "iters": 2}})):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        runs[key] = (afdm.ddpm_run(dict(params, **extra)), _files(wd))
    (plain, plain_files), (out, files) = runs["plain"], runs["distill"]
    assert "distill" not in plain and not any("distill" in f for f in plain_files)
    new = "models/DDPM_Uncondtional_MNIST_3/ckpt_MNIST_3_distill2.pt"
    assert files == sorted(plain_files + [new])                       # the same file set, plus the student
    d = out["distill"]
    assert d["modelpath"] == str(tmp_path / "distill" / new)
    assert [r["steps"] for r in d["rounds"]] == [2] and d["rounds"][0]["chain"] == [11, 4]
    assert all(math.isfinite(r["mean_loss"]) for r in d["rounds"])
    sd = torch.load(d["modelpath"], weights_only=True)
    ck = torch.load(out["modelpath"], weights_only=True)
    assert sd.keys() == ck.keys() and any(not torch.equal(sd[k], ck[k]) for k in sd)
    assert len([f for f in files if f.startswith("images/generated/MNIST_3/")]) == len(
        [f for f in plain_files if f.startswith("images/generated/MNIST_3/")])
