"""Training objectives on the GPU: the fused objective loss (forward / backward) and the output-to-eps conversion against fp64
torch on the host, samplers on a v- / x0-model against the same model read as eps, TrainStep parity and launch modes, data
parallel, and the drop-in keys."""
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import check, load_golden, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 1e-5                  # the project's per-op rel-L2 gate
KINDS = ("eps", "v", "x0")
SHAPES = ((1, 3), (3, 255), (16, 3072), (256, 3072))


def T_(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42, num_classes=None):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


# ---- kernels against fp64 torch on the host ---------------------------------------------------------------------------------
def _placed(x, dev, shift):
    """x on the device as a contiguous view that starts `shift` floats into its buffer (shift 0: 16-byte aligned)."""
    buf = torch.empty(x.numel() + 4, device=dev, dtype=torch.float32)
    v = buf[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * shift
    return v


def _case(B, chw, T, seed):
    """Independent random pred / x0 / eps (the kernels map any values; x0 doubles as x_t for the conversion), t over all of
    1 .. T-1 with both ends present when B allows."""
    g = torch.Generator().manual_seed(seed)
    pred, eps = torch.randn(B, chw, generator=g), torch.randn(B, chw, generator=g)
    x0 = torch.rand(B, chw, generator=g) * 2 - 1
    t = torch.randint(1, T, (B,), generator=g)
    t[0] = T - 1
    if B > 1:
        t[1] = 1
    return pred, x0, eps, t


def _ref(kind, pred, x0, eps, t, ah, w):
    """fp64: (loss, dpred for dloss = 1)."""
    a = ah.double()[t][:, None]
    sa, sb = torch.sqrt(a), torch.sqrt(1.0 - a)
    p, x, e = pred.double(), x0.double(), eps.double()
    tgt = {"eps": e, "x0": x, "v": sa * e - sb * x}[kind]
    wr = torch.ones(len(t), dtype=torch.float64) if w is None else w.double()[t]
    n = pred.numel()
    loss = (wr[:, None] * (p - tgt) ** 2).sum() / n
    dpred = 2.0 * wr[:, None] * (p - tgt) / n
    return loss, dpred


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_objective_loss_against_fp64(A, kind, weighted, schedule):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule, prediction=kind)
    ah = diff.alpha_hat.cpu()
    w = diff.snr_weights("min_snr", 5.0).float() if weighted else None
    w_d = None if w is None else w.to(dev)
    for B, chw in SHAPES:
        pred, x0, eps, t = _case(B, chw, 1000, 7 * B + chw)
        want_loss, want_d = _ref(kind, pred, x0, eps, t, ah, w)
        t_d = t.to(dev)
        got = {}
        for shift in (0, 1):
            p_d = _placed(pred, dev, shift).requires_grad_(True)
            x_d, e_d = _placed(x0, dev, shift), _placed(eps, dev, shift)
            runs = []
            for _ in range(2):
                p_d.grad = None
                loss = afdm.ops.objective_loss(p_d, x_d, e_d, t_d, diff.alpha_hat, w_d, kind)
                loss.backward()
                runs.append((loss.detach().clone(), p_d.grad.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # identical bytes run to run
            got[shift] = runs[0]
            tag = f"{kind} w={weighted} {schedule} B={B} chw={chw} shift={shift}"
            check("objective loss fwd vs fp64", got[shift][0].cpu().reshape(1), want_loss.reshape(1), GATE, tag)
            check("objective loss bwd vs fp64", got[shift][1].cpu(), want_d, GATE, tag)
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])               # vector path == scalar path
        # dloss scales the gradient (the kernel reads it from the device)
        p_d = pred.to(dev).requires_grad_(True)
        (afdm.ops.objective_loss(p_d, x0.to(dev), eps.to(dev), t_d, diff.alpha_hat, w_d, kind) * 3.0).backward()
        check("objective loss bwd vs fp64", p_d.grad.cpu(), 3.0 * want_d, GATE, f"{kind} dloss=3 B={B} chw={chw}")


def test_unweighted_eps_objective_is_the_mse(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    pred, x0, eps, t = _case(16, 3072, 1000, 5)
    p1 = pred.to(dev).requires_grad_(True)
    p2 = pred.to(dev).requires_grad_(True)
    l1 = afdm.ops.objective_loss(p1, x0.to(dev), eps.to(dev), t.to(dev), diff.alpha_hat, None, "eps")
    l2 = afdm.ops.mse_loss(eps.to(dev), p2)
    l1.backward()
    l2.backward()
    check("objective loss (eps, unweighted) vs mse_loss", l1.detach().cpu().reshape(1), l2.detach().cpu().reshape(1), 1e-6)
    assert torch.equal(p1.grad, p2.grad)                    # the same expression, operation for operation


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("kind", ("v", "x0"))
def test_pred_to_eps_against_fp64(A, kind, schedule):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule, prediction=kind)
    ah = diff.alpha_hat.cpu()
    for B, chw in SHAPES:
        out, x_t, _, t = _case(B, chw, 1000, 3 * B + chw)
        a = ah.double()[t][:, None]
        sa, sb = torch.sqrt(a), torch.sqrt(1.0 - a)
        want = sa * out.double() + sb * x_t.double() if kind == "v" else (x_t.double() - sa * out.double()) / sb
        t_d = t.to(dev)
        got = {}
        for shift in (0, 1):
            o_d, x_d = _placed(out, dev, shift), _placed(x_t, dev, shift)
            dst = _placed(torch.zeros_like(out), dev, shift)
            r1 = afdm.ops.pred_to_eps(o_d, x_d, t_d, diff.alpha_hat, kind, eps_out=dst).clone()
            r2 = afdm.ops.pred_to_eps(o_d, x_d, t_d, diff.alpha_hat, kind)
            assert torch.equal(r1, r2) and torch.equal(o_d.cpu(), out)                               # run to run; input untouched
            check("pred_to_eps vs fp64", r1.cpu(), want, GATE, f"{kind} {schedule} B={B} chw={chw} shift={shift}")
            same = afdm.ops.pred_to_eps(o_d, x_d, t_d, diff.alpha_hat, kind, eps_out=o_d)            # in place
            assert same is o_d and torch.equal(o_d, r1)
            got[shift] = r1
        assert torch.equal(got[0], got[1])
    with pytest.raises(afdm.AfdError, match="afd_pred_to_eps: kind must be AFD_PRED_V or AFD_PRED_X0"):
        afdm.ops.pred_to_eps(o_d, x_d, t_d, diff.alpha_hat, "eps")


def test_conversion_is_consistent_with_noise_images(A):
    """x_t from noise_images and the v target of the loss kernel: converting the exact target back gives eps to fp32 rounding."""
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction="v")
    _, x0, eps, t = _case(64, 3072, 1000, 11)
    x0, eps, t = x0.to(dev), eps.to(dev), t.to(dev)
    x_t, _ = diff.noise_images(x0, t, eps)
    v = diff.training_target(x0.double(), eps.double(), t).float()
    back = afdm.ops.pred_to_eps(v, x_t, t, diff.alpha_hat, "v")
    check("pred_to_eps(training_target) vs eps", back.cpu(), eps.cpu(), GATE)
    loss = afdm.ops.objective_loss(v, x0, eps, t, diff.alpha_hat, None, "v")
    # the kernel's target is that v up to four fp32 roundings of values below 8: at most 4 * 2^-21 = 2e-6 per element
    assert float(loss) < 4e-12


def test_non_finite_values_are_ordinary_data(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="v")
    pred, x0, eps, t = (a.to(dev) for a in _case(4, 255, 1000, 2))
    pred[1, 7] = float("nan")
    pred[2, 9] = float("inf")
    p = pred.clone().requires_grad_(True)
    loss = afdm.ops.objective_loss(p, x0, eps, t, diff.alpha_hat, None, "v")
    loss.backward()
    assert not math.isfinite(float(loss))
    bad = ~torch.isfinite(p.grad)
    assert bad[1, 7] and bad[2, 9] and int(bad.sum()) == 2                # they stay where they are
    e = afdm.ops.pred_to_eps(pred, x0, t, diff.alpha_hat, "v")
    bad = ~torch.isfinite(e)
    assert bad[1, 7] and bad[2, 9] and int(bad.sum()) == 2


# ---- samplers: a v- / x0-model equals the same model read as eps ---------------------------------------------------------------
class AsKind(torch.nn.Module):
    """An eps-model presented as a v- or x0-model: its output is the `training_target`-style tensor formed from its eps and the
    x0 that eps implies at x_t, in fp64 torch ops, rounded once to fp32."""

    def __init__(self, net, diff, kind):
        super().__init__()
        self.net, self.kind, self.ah = net, kind, diff.alpha_hat.double()

    label_emb = property(lambda self: self.net.label_emb)
    _t_range = property(lambda self: self.net._t_range, lambda self, v: setattr(self.net, "_t_range", v))

    def forward(self, x, t, y=None):
        e = (self.net(x, t) if y is None else self.net(x, t, y)).double()
        a = self.ah[t].reshape(-1, 1, 1, 1)
        sa, sb = torch.sqrt(a), torch.sqrt(1.0 - a)
        x0 = (x.double() - sb * e) / sa
        return (x0 if self.kind == "x0" else sa * e - sb * x0).float()


def _sampler_runs(afdm, dev, diff, model, cond_model):
    g = torch.Generator().manual_seed(1)
    images = (torch.rand(2, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros(1, 1, 32, 32)
    mask[..., :16] = 1
    labels = torch.tensor([1, 3])
    return {
        "ddim": lambda gr: diff.sample(model, n=2, image_channels=3, noise_source="device", return_float=True, steps=10, eta=0.0, graph=gr)[2],
        "dpmpp_2m": lambda gr: diff.sample(model, n=2, image_channels=3, noise_source="device", return_float=True, steps=10,
                                           sampler="dpmpp_2m", graph=gr)[2],
        "inpaint": lambda gr: diff.inpaint(model, images, mask, steps=10, noise_source="device", return_float=True, graph=gr)[2],
        "guided": lambda gr: diff.sample(cond_model, n=2, image_channels=3, noise_source="device", return_float=True, steps=10,
                                         eta=0.0, labels=labels, cfg_scale=3.0, graph=gr)[2],
    }


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
def test_samplers_on_v_and_x0_models_equal_the_eps_model(A, schedule):
    afdm, dev = A
    net, cnet = _model(afdm, dev), _model(afdm, dev, seed=43, num_classes=5)
    base = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule)
    want = {}
    for name, run in _sampler_runs(afdm, dev, base, net, cnet).items():
        afdm.set_seed(9)
        want[name] = run(False).clone()
        assert bool(torch.isfinite(want[name]).all())
    for kind in ("v", "x0"):
        diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule, prediction=kind)
        runs = _sampler_runs(afdm, dev, diff, AsKind(net, diff, kind), AsKind(cnet, diff, kind))
        for name, run in runs.items():
            got = {}
            for gr in (False, True):
                afdm.set_seed(9)
                got[gr] = run(gr).clone()
            e = rel_l2(got[False].cpu(), want[name].cpu())
            print(f"{schedule} {kind} {name}: rel-L2 to the eps run {e:.3e}; graph == eager: {torch.equal(got[True], got[False])}")
            check("sampler on a v/x0 model vs the eps model", got[False].cpu(), want[name].cpu(), GATE, f"{schedule} {kind} {name}")
            assert torch.equal(got[True], got[False]), (schedule, kind, name)


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
def test_calc_bpd_on_v_and_x0_models_equals_the_eps_model(A, schedule):
    afdm, dev = A
    net = _model(afdm, dev)
    g = torch.Generator().manual_seed(4)
    images = torch.randint(0, 256, (4, 3, 32, 32), generator=g, dtype=torch.uint8)
    base = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule)
    afdm.set_seed(6)
    want = base.calc_bpd(net, images, t_samples=8)["bpd"]
    for kind in ("v", "x0"):
        diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule=schedule, prediction=kind)
        afdm.set_seed(6)
        got = diff.calc_bpd(AsKind(net, diff, kind), images, t_samples=8)["bpd"]
        e = float(((got - want).abs() / want.abs()).max())
        print(f"calc_bpd {schedule} {kind}: {got.tolist()} against {want.tolist()}: max rel {e:.3e}")
        note("calc_bpd on a v/x0 model vs the eps model (max rel)", e, f"{schedule} {kind}")
        assert e < 1e-5, (schedule, kind, e)


# ---- train step --------------------------------------------------------------------------------------------------------------
def _batch(dev, B=16, seed=0, labels=False):
    g = torch.Generator().manual_seed(seed)
    images = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    steps = [(torch.randint(1, 1000, (B,), generator=g), torch.randn(B, 3, 32, 32, generator=g).to(dev)) for _ in range(3)]
    y = torch.randint(0, 5, (B,), generator=g) if labels else None
    return images, steps, y


@pytest.mark.parametrize("kind,weighting", (("v", "min_snr"), ("x0", "min_snr"), ("eps", "min_snr"), ("v", None)))
def test_train_step_parity_with_the_loss_in_torch_ops(A, kind, weighting):
    afdm, dev = A
    images, steps, _ = _batch(dev)
    t, eps = steps[0]
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction=kind)
    step = afdm.TrainStep(_model(afdm, dev), diff, lr=3e-4, loss_weighting=weighting)
    loss = step(images, t=t, eps=eps)
    fp = step.opt.fp
    got_grad = fp.grad[:fp.n_active].clone()
    # the same forward, the loss in torch ops on the device, backward through the project's autograd ops into the flat gradient
    ref = afdm.TrainStep(_model(afdm, dev), diff, lr=3e-4)
    t_d = t.to(dev)
    x_t, _ = diff.noise_images(images, t_d, eps)
    pred = ref.model(x_t, t_d)
    w = torch.ones(1000, device=dev) if weighting is None else diff.snr_weights(weighting, 5.0).float().to(dev)
    target = diff.training_target(images, eps, t_d)
    want_loss = (w[t_d][:, None, None, None] * (pred - target) ** 2).mean()
    ref.opt.zero_grad()
    with afdm.ops.inplace_param_grads(ref.wgrad_stream, ref.wgrad_batch):
        want_loss.backward()
    torch.cuda.synchronize()
    want_grad = ref.opt.fp.grad[:ref.opt.fp.n_active]
    tag = f"{kind} {weighting}"
    print(f"{tag}: loss {float(loss):.6f} against {float(want_loss):.6f}")
    check("TrainStep objective loss vs torch ops", loss.cpu().reshape(1), want_loss.detach().cpu().reshape(1), GATE, tag)
    check("TrainStep objective flat gradient vs torch ops", got_grad.cpu(), want_grad.cpu(), GATE, tag)
    if weighting is not None:
        assert step.loss_weights.dtype == torch.float32 and step.loss_weights.is_cuda and tuple(step.loss_weights.shape) == (1000,)


def _make_step(afdm, dev, full, mode, diff_kw, step_kw):
    """full: ema= + max_grad_norm= + lr_schedule= + conditional=True on a UNet(num_classes=5); else the plain step."""
    model = _model(afdm, dev, num_classes=5 if full else None)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **diff_kw)
    kw = dict(step_kw)
    if full:
        kw.update(ema=afdm.EMA(0.9), ema_model=copy.deepcopy(model), ema_start=1, max_grad_norm=0.5, conditional=True,
                  lr_schedule=afdm.LRSchedule("cosine", warmup=1, total=3, min_ratio=0.1))
    return afdm.TrainStep(model, diff, lr=3e-4, graph=mode, **kw)


@pytest.mark.parametrize("full", (False, True))
def test_objective_step_in_every_launch_mode(A, full):
    afdm, dev = A
    images, steps, y = _batch(dev, labels=full)
    got = {}
    for mode in (False, True, "lanes"):
        step = _make_step(afdm, dev, full, mode, dict(schedule="cosine", prediction="v"), dict(loss_weighting="min_snr"))
        losses = [step(images, t=t, eps=e, y=y).clone() for t, e in steps]
        torch.cuda.synchronize()
        assert all(math.isfinite(float(l)) for l in losses)
        got[mode] = [torch.stack(losses), step.opt.fp.flat.clone(), step.opt.m.clone(), step.opt.v.clone()]
        if full:
            got[mode].append(step._ema_home.flat.clone())
    default = _make_step(afdm, dev, full, "lanes", {}, {})
    default(images, t=steps[0][0], eps=steps[0][1], y=y)
    print("work nodes of the replayed step: objective", step.lanes_counts[0], "default", default.lanes_counts[0])
    assert step.lanes_counts[0] == default.lanes_counts[0]                 # no launch more than the default step
    for mode in (True, "lanes"):
        for a, b, tag in zip(got[mode], got[False], ("losses", "params", "m", "v", "ema")):
            assert torch.equal(a, b), (mode, tag)


def test_default_step_still_runs_mse_loss(A, monkeypatch):
    afdm, dev = A
    images, steps, _ = _batch(dev)
    calls = {"mse": 0, "objective": 0}
    mse, obj = afdm.ops.mse_loss, afdm.ops.objective_loss

    def counted_mse(*a):
        calls["mse"] += 1
        return mse(*a)

    def counted_obj(*a, **k):
        calls["objective"] += 1
        return obj(*a, **k)
    out = []
    for dkw, skw in (({}, {}), (dict(schedule="linear", prediction="eps"), dict(loss_weighting=None, snr_gamma=5.0))):
        step = afdm.TrainStep(_model(afdm, dev), afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **dkw), lr=3e-4, **skw)
        assert step.loss_weights is None and step.prediction == "eps"
        monkeypatch.setattr(afdm.ops, "mse_loss", counted_mse)
        monkeypatch.setattr(afdm.ops, "objective_loss", counted_obj)
        for t, e in steps:
            step(images, t=t, eps=e)
        monkeypatch.undo()
        torch.cuda.synchronize()
        out.append(step.opt.fp.flat.clone())
    assert calls == {"mse": 6, "objective": 0}
    assert torch.equal(out[0], out[1])
    # ... and an objective step does not
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, prediction="v")
    step = afdm.TrainStep(_model(afdm, dev), diff, lr=3e-4)
    monkeypatch.setattr(afdm.ops, "mse_loss", counted_mse)
    monkeypatch.setattr(afdm.ops, "objective_loss", counted_obj)
    step(images, t=steps[0][0], eps=steps[0][1])
    assert calls == {"mse": 6, "objective": 1}


def test_two_rank_objective_step_equals_single_rank(A, tmp_path):
    afdm, dev = A
    out = tmp_path / "objective_ddp"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29563", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29563", os.path.join(ROOT, "tests", "objective_ddp_worker.py"), "--out", str(out)]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in (0, 1))
    assert torch.equal(r0["params"], r1["params"])
    g = load_golden("train_step.npz")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction="v")
    step = afdm.TrainStep(model, diff, lr=3e-4, loss_weighting="min_snr")
    losses = [float(step(T_(g["images"]).to(dev), t=T_(g[tk]), eps=T_(g[ek]).to(dev))) for tk, ek in (("t0", "eps0"), ("t1", "eps1"))]
    torch.cuda.synchronize()
    err = rel_l2(r0["params"], step.opt.fp.flat.cpu())
    mean = [(a + b) / 2 for a, b in zip(r0["losses"], r1["losses"])]     # equal shards: the one-rank loss is the ranks' mean
    el = max(abs(m - l) / abs(l) for m, l in zip(mean, losses))
    print("2-rank vs 1-rank objective step: params rel-L2", err, "mean loss rel", el)
    note("2-rank objective step vs 1 rank (params)", err)
    assert err < 1e-6 and el < 1e-5                                       # test_two_rank_clip_equals_single_rank's tolerances


# ---- drop-in ---------------------------------------------------------------------------------------------------------------------
def test_ddpm_run_with_the_objective_keys_and_evaluation_as_a_v_model(A, tmp_path, monkeypatch):
    afdm, dev = A
    from PIL import Image
    rng = np.random.default_rng(0)
    for c in ("a", "b"):
        os.makedirs(tmp_path / "data" / c)
        for i in range(4):
            Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / "data" / c / f"{i}.png")
    monkeypatch.chdir(tmp_path)
    params = {"unet_v": 3, "dataset": "synthetic", "epochs": 1, "batchsize": 4, "image_size": 32, "image_channels": 3,
              "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(tmp_path / "data"),
              "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
              "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42,
              "noise_schedule": "cosine", "prediction": "v", "loss_weighting": "min_snr", "snr_gamma": 3.0}
    seen = []
    init = afdm.TrainStep.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        seen.append((self.prediction, self.diffusion.schedule, self.loss_weighting, self.snr_gamma))
    monkeypatch.setattr(afdm.TrainStep, "__init__", spy)
    out = afdm.ddpm_run(dict(params))
    assert seen == [("v", "cosine", "min_snr", 3.0)]
    run = "DDPM_Uncondtional_synthetic_3"
    text = (tmp_path / "runs" / run / "settings_synthetic_3.txt").read_text()
    assert text.endswith("\nnoise_schedule: cosine\nprediction: v\nloss_weighting: min_snr\nsnr_gamma: 3.0")
    ckpt = tmp_path / "models" / run / "ckpt_synthetic_3.pt"
    assert ckpt.exists() and out["modelpath"] == str(ckpt) and all(math.isfinite(l) for l in out["loss_all"])
    # the checkpoint is evaluated as the v-model it is: bpd_results builds its Diffusion from the same keys
    args = afdm.argument(image_size=32, image_channels=3, device="cuda", noise_steps=12, noise_schedule="cosine", prediction="v")
    data = {"args": args, "unet_v": 3, "seed": 42, "f_settings": dict(F_SET), "modelpath": str(ckpt)}
    made = []
    ctor = afdm.Diffusion.__init__

    def spy_d(self, *a, **k):
        ctor(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(afdm.Diffusion, "__init__", spy_d)
    images = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8)
    r = afdm.bpd_results(data, images)
    assert len(made) == 1 and made[0].prediction == "v" and made[0].schedule == "cosine"
    assert bool(torch.isfinite(r["bpd"]).all())
    args.prediction = None                                                # read as an eps-model it scores differently
    r_eps = afdm.bpd_results(data, images)
    assert made[1].prediction == "eps" and not torch.equal(r["bpd"], r_eps["bpd"])
