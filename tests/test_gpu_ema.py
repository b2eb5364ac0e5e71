"""EMA of the weights on the MI355X: the three kernels against torch evaluated on the device (bit for bit), the fused
TrainStep(ema=...) in every launch mode, the unused tail of variant 4, sampling from the EMA model, data parallelism and the
ddpm_run drop-in."""
import copy
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def T(a):
    return torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _rule(ema, p, copy_, beta):
    """the reference's update_average / load_state_dict, in torch on the device"""
    return p.clone() if copy_ else ema * beta + (1 - beta) * p


def _views(n, dev, offset, k, seed):
    """k device vectors of n fp32 values, each a view `offset` elements into its own allocation (offset 1: not 16-byte aligned)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(n + offset, device=dev, generator=g)[offset:] for _ in range(k)]


SIZES = (1, 3, 4, 4099, 6_000_003)


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_ema_step_kernel_bit_exact(A, n, offset):
    afdm, dev = A
    from afdm import ops
    L = afdm.lib()
    for beta in (0.995, 0.9, 0.0, 1.0):
        for copy_ in (1, 0):
            ema, p = _views(n, dev, offset, 2, seed=n + offset)
            want = _rule(ema, p, copy_, beta)
            p0 = p.clone()
            L.afd_ema_step(ema.data_ptr(), p.data_ptr(), n, copy_, float(beta), float(1.0 - beta), ops._stream())
            torch.cuda.synchronize()
            assert torch.equal(ema, want), (n, offset, beta, copy_)
            assert torch.equal(p, p0)


def _adam_inputs(n, dev, offset, seed):
    p, g, m, v, ema = _views(n, dev, offset, 5, seed)
    v = v.abs_()
    m.mul_(0.1)
    return p, g, m, v, ema


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_adamw_ema_step_bit_exact_against_adamw_step(A, n, offset):
    afdm, dev = A
    from afdm import ops
    L, s = afdm.lib(), ops._stream()
    lr, b1, b2, eps, wd, gs = 3e-4, 0.9, 0.999, 1e-8, 0.01, 0.5
    beta = 0.995
    for tail in (0, 5):
        n_ema = n + tail
        for calls, start in ((0, 1), (3, 1), (6, 2000)):           # copy, blend, copy
            p, g, m, v, ema = _adam_inputs(n_ema, dev, offset, seed=7 * n + offset + tail)
            state = torch.tensor([calls, 0, 0, 0], device=dev, dtype=torch.float32)
            # the plain AdamW step on copies
            p1, m1, v1, st1 = p.clone(), m.clone(), v.clone(), state.clone()
            L.afd_adamw_tick(st1.data_ptr(), b1, b2, s)
            L.afd_adamw_step(p1.data_ptr(), g.data_ptr(), m1.data_ptr(), v1.data_ptr(), n, st1.data_ptr(), lr, b1, b2, eps, wd, gs, s)
            # the fused form
            p0, ema0 = p.clone(), ema.clone()
            es = torch.tensor([calls, 7], device=dev, dtype=torch.int32)
            L.afd_adamw_ema_tick(state.data_ptr(), b1, b2, es.data_ptr(), start, s)
            L.afd_adamw_ema_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, state.data_ptr(), lr, b1, b2, eps, wd,
                                 gs, ema.data_ptr(), n_ema, es.data_ptr(), beta, float(1.0 - beta), s)
            torch.cuda.synchronize()
            copy_ = calls < start
            assert es.tolist() == [calls + 1, int(copy_)]
            assert torch.equal(state, st1)
            assert torch.equal(p[:n], p1[:n]) and torch.equal(m[:n], m1[:n]) and torch.equal(v[:n], v1[:n]), (n, offset, tail)
            assert torch.equal(p[n:], p0[n:]) and torch.equal(m[n:], m1[n:]) and torch.equal(v[n:], v1[n:])   # the tail: no AdamW
            assert torch.equal(ema, _rule(ema0, p, copy_, beta)), (n, offset, tail, calls)                   # the rule on the NEW p
            if not copy_ and tail:
                assert not torch.equal(ema[n:], ema0[n:])                                                    # the tail was blended


def _setup(afdm, dev, variant=3, num_classes=None):
    afdm.set_seed(42)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=variant, **kw).to(dev)
    return model, afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)


def _inputs(dev):
    g = load_golden("train_step.npz")
    images = T(g["images"]).to(dev)
    return images, [(T(g["t0"]), T(g["eps0"]).to(dev)), (T(g["t1"]), T(g["eps1"]).to(dev)), (T(g["t0"]), T(g["eps1"]).to(dev))]


def _named(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def _plain_then_slow_ema(afdm, dev, beta, start, images, batches, variant=3, num_classes=None):
    """The reference's loop: a plain TrainStep, then the per-tensor EMA on a copy of the model that no FlatParams owns."""
    model, diff = _setup(afdm, dev, variant, num_classes)
    ref_ema = copy.deepcopy(model)
    step = afdm.TrainStep(model, diff, lr=3e-4)
    ema = afdm.EMA(beta)
    for t, e in batches:
        step(images, t=t, eps=e)
        snap = copy.deepcopy(model)                              # (Parameter deepcopy clones: not homed)
        ema.step_ema(ref_ema, snap, step_start_ema=start)
    assert ema._home is None                                     # the slow path ran
    return _named(model), _named(ref_ema)


def test_train_step_ema_in_every_launch_mode(A):
    afdm, dev = A
    beta = 0.9
    images, batches = _inputs(dev)
    plain_params, slow_ema = _plain_then_slow_ema(afdm, dev, beta, 1, images, batches)
    got = {}
    for mode in (False, True, "lanes"):
        model, diff = _setup(afdm, dev)
        ema_model = copy.deepcopy(model)                         # made before the model is homed
        ema = afdm.EMA(beta)
        step = afdm.TrainStep(model, diff, lr=3e-4, graph=mode, ema=ema, ema_model=ema_model, ema_start=1)
        fp, h = step.opt.fp, step._ema_home
        ref = None
        for k, (t, e) in enumerate(batches):                     # calls 1 copy, 2 and 3 blend: the boundary is crossed in replays
            step(images, t=t, eps=e)
            torch.cuda.synchronize()
            ref = fp.flat.clone() if ref is None else ref * beta + (1 - beta) * fp.flat
            assert torch.equal(h.flat, ref), (mode, k)           # the rule on this mode's own parameters, bit for bit
            assert ema.step == k + 1
        assert h.state.tolist() == [3, 0]
        with pytest.raises(RuntimeError, match="TrainStep"):
            ema.step_ema(ema_model, model)
        name_of, ep = {id(q): n for n, q in model.named_parameters()}, dict(ema_model.named_parameters())
        assert all(ep[name_of[id(q)]].data_ptr() == h.flat.data_ptr() + 4 * o for q, o in zip(fp.params, fp.offsets))
        got[mode] = (_named(model), _named(ema_model), h.flat.clone(), getattr(step, "lanes_counts", None))
    # eager: AdamW bit-identical to the plain step, the EMA bit-identical to the reference's per-tensor loop after it
    for k in plain_params:
        assert torch.equal(got[False][0][k], plain_params[k]), k
        assert torch.equal(got[False][1][k], slow_ema[k]), k
    # the captured step issued two ways: bit-identical; against eager as close as the parameters themselves (test_gpu_model)
    assert torch.equal(got[True][2], got["lanes"][2])
    e_graph = rel_l2(got[True][2].cpu(), got[False][2].cpu())
    print("EMA graph vs eager rel-L2", e_graph)
    assert e_graph < 1e-6
    # no added launch: the same replay list as the step without EMA
    model, diff = _setup(afdm, dev)
    plain = afdm.TrainStep(model, diff, lr=3e-4, graph="lanes")
    plain(images, t=batches[0][0], eps=batches[0][1])
    assert got["lanes"][3] == plain.lanes_counts


def test_variant4_unused_tail_is_blended_like_the_reference(A):
    """Variant 4 with num_classes, trained without labels: label_emb and the stage-level norm1 sit beyond n_active.  The fused
    EMA must equal the reference's per-tensor EMA applied after each step to the same parameters, tail included."""
    afdm, dev = A
    beta = 0.9                                                   # (not 0.5: v * 2^-1 + v * 2^-1 is v exactly)
    images, batches = _inputs(dev)
    model, diff = _setup(afdm, dev, variant=4, num_classes=10)
    ref_ema = copy.deepcopy(model)
    afdm.FlatParams(model)                                       # homed first, copied after: the other order
    ema_model = copy.deepcopy(model)
    with torch.no_grad():
        for p in ema_model.parameters():
            p.mul_(3.0)                                          # the first call copies: no trace of this may remain
    ema, slow = afdm.EMA(beta), afdm.EMA(beta)
    step = afdm.TrainStep(model, diff, lr=3e-4, ema=ema, ema_model=ema_model, ema_start=1)
    tail = {n for n, p in model.named_parameters() if id(p) in {id(q) for q in model.unused_parameters()}}
    assert any(n.startswith("label_emb") for n in tail) and any(".norm1." in n for n in tail)
    assert step.opt.fp.n_active < step.opt.fp.numel
    tail0 = {k: v for k, v in _named(model).items() if k in tail}
    for t, e in batches:
        step(images, t=t, eps=e)
        slow.step_ema(ref_ema, copy.deepcopy(model), step_start_ema=1)      # (the deepcopy is not homed: per-tensor path)
        got, want = _named(ema_model), _named(ref_ema)
        for k in want:
            assert torch.equal(got[k], want[k]), (slow.step, k)
    assert slow._home is None and ema.step == slow.step == 3
    now = _named(model)
    assert all(torch.equal(now[k], tail0[k]) for k in tail)                  # AdamW left the tail alone ...
    assert any(not torch.equal(got[k], now[k]) for k in tail)                # ... the EMA blended it (v*b + v*(1-b) is not always v)


def _sample(afdm, diff, net, seed):
    afdm.set_seed(seed)
    _, _, x = diff.sample(net, n=4, image_channels=3, steps=20, return_float=True)
    return x


def test_sampling_from_the_ema_model_equals_a_loaded_copy(A):
    afdm, dev = A
    images, batches = _inputs(dev)
    model, diff = _setup(afdm, dev)
    ema_model = copy.deepcopy(model)
    ema = afdm.EMA(0.9)
    step = afdm.TrainStep(model, diff, lr=3e-4, ema=ema, ema_model=ema_model, ema_start=1)
    for t, e in batches[:2]:
        step(images, t=t, eps=e)

    def loaded():
        buf = io.BytesIO()
        torch.save(ema_model.state_dict(), buf)
        buf.seek(0)
        net = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
        net.load_state_dict(torch.load(buf, weights_only=True))
        return net

    a = _sample(afdm, diff, ema_model, 11)
    assert torch.equal(a, _sample(afdm, diff, loaded(), 11))
    step(images, t=batches[2][0], eps=batches[2][1])             # the EMA moves: cached weight images of ema_model are stale
    b = _sample(afdm, diff, ema_model, 11)
    assert not torch.equal(a, b)
    assert torch.equal(b, _sample(afdm, diff, loaded(), 11))


def test_two_rank_ema_equals_single_rank(A, tmp_path):
    afdm, dev = A
    out = tmp_path / "ema_ddp"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "tests", "ema_ddp_worker.py"), "--out", str(out)]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in (0, 1))
    assert torch.equal(r0["ema"], r1["ema"]) and torch.equal(r0["params"], r1["params"])
    assert r0["ema_step"] == 2 and r0["state"].tolist() == [2, 0]
    images, batches = _inputs(dev)
    model, diff = _setup(afdm, dev)
    ema_model = copy.deepcopy(model)
    step = afdm.TrainStep(model, diff, lr=3e-4, ema=afdm.EMA(0.9), ema_model=ema_model, ema_start=1)
    for t, e in batches[:2]:
        step(images, t=t, eps=e)
    err = rel_l2(r0["ema"], step._ema_home.flat.cpu())
    print("2-rank vs 1-rank EMA rel-L2", err)
    assert err < 1e-6


def test_ddpm_run_with_ema(A, tmp_path, monkeypatch):
    afdm, dev = A
    rng = np.random.default_rng(0)
    csvp = tmp_path / "mnist.csv"
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    np.savetxt(csvp, arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
    monkeypatch.chdir(tmp_path)
    params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
              "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(csvp),
              "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
              "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42,
              "ema_beta": 0.9, "ema_start": 1}
    out = afdm.ddpm_run(params)
    run = "DDPM_Uncondtional_MNIST_3"
    ema_file = tmp_path / "models" / run / "ckpt_MNIST_3_ema.pt"
    assert out["ema_modelpath"] == str(ema_file) and ema_file.exists()
    assert (tmp_path / "results" / run / "0.jpg").exists() and (tmp_path / "results" / run / "0_ema.jpg").exists()
    assert (tmp_path / "images" / "generated" / "MNIST_3" / "image_3.png").exists()
    sd_ema = torch.load(ema_file, weights_only=True)
    sd = torch.load(tmp_path / "models" / run / "ckpt_MNIST_3.pt", weights_only=True)
    assert len(sd_ema) == 182 and set(sd_ema) == set(sd)
    net = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    net.load_state_dict(sd_ema)
    assert any(not torch.equal(sd_ema[k], sd[k]) for k in sd)                # 2 steps: a copy, then a blend
