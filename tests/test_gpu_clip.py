"""Gradient-norm clipping and the learning-rate schedule on the MI355X: the norm kernel against torch in fp64, the control tick
against its host mirrors, the ctl-driven AdamW step bit for bit against the by-value one, optimiser parity against
clip_grad_norm_ + AdamW + LambdaLR on the CPU, TrainStep in every launch mode, data parallelism and the ddpm_run drop-in.
Non-finite values are ordinary data to these kernels: no test here provokes a device fault."""
import copy
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, COEF, NORM, SKIP, NSKIP, SQ, INDEX, FACTOR = range(8)
LR_TOL = 2e-7      # device lr against the fp64 host value, relative: the rounding to fp32 (2^-24 = 6e-8) + one fp32 ulp for the device's cos (1.2e-7)


def T(a):
    return torch.from_numpy(np.asarray(a))


def schedule_grid():
    """(kind, warmup, total, min_ratio): the grid of test_clip_host.test_lr_schedule_equals_lambda_lr_exactly"""
    for kind in ("constant", "linear", "cosine"):
        for warmup in (0, 1, 3):
            for min_ratio in (0.0, 0.1, 1.0):
                for total in (warmup, 10, 1000):
                    yield kind, warmup, total, min_ratio


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _partials(afdm, g, scale):
    from afdm import ops
    L = afdm.lib()
    n_p = L.afd_grad_sqnorm_n_partials()
    out = torch.full((n_p,), -1.0, device=g.device, dtype=torch.float64)
    L.afd_grad_sqnorm_partials(g.data_ptr(), g.numel(), scale, out.data_ptr(), n_p, ops._stream())
    torch.cuda.synchronize()
    return out


def _ordered(parts):
    """the tick's sum: index order, fp64"""
    s = 0.0
    for x in parts.cpu().tolist():
        s += x
    return s


NORM_SIZES = (1, 3, 255, 4097, 2 ** 20 + 5, 5_900_000)


@pytest.mark.parametrize("n", NORM_SIZES)
def test_grad_sqnorm_kernel_against_fp64_torch(A, n):
    afdm, dev = A
    gen = torch.Generator(device=dev).manual_seed(1000 + n % 997)
    aligned = torch.randn(n, device=dev, generator=gen)
    shifted = torch.empty(n + 1, device=dev)[1:]                 # the same data one float into its allocation: not 16-byte aligned
    shifted.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    seen = {}
    for offset, g in ((0, aligned), (1, shifted)):
        for scale in (1.0, 0.5):
            parts = _partials(afdm, g, scale)
            again = _partials(afdm, g, scale)
            assert torch.equal(parts, again)                     # run to run: identical bytes
            want = float(torch.linalg.vector_norm(g.double() * scale)) ** 2
            got = _ordered(parts)
            err = abs(got - want) / want
            print(f"sqnorm n={n} offset={offset} scale={scale}: rel err of sq {err:.3e}")
            note("grad_sqnorm: rel err of sq vs torch fp64", err, f"n={n} offset={offset} scale={scale}")
            assert err <= 1e-12, (n, offset, scale, err)
            seen[offset, scale] = parts
    for scale in (1.0, 0.5):
        assert torch.equal(seen[0, scale], seen[1, scale])       # aligned and misaligned views of the same data: identical bytes


def test_grad_sqnorm_extremes(A):
    afdm, dev = A
    n = 4097
    g = torch.full((n,), 1e20, device=dev)
    sq = _ordered(_partials(afdm, g, 1.0))
    assert math.isfinite(sq) and abs(math.sqrt(sq) - 1e20 * math.sqrt(n)) < 1e-6 * 1e20 * math.sqrt(n)      # fp32 squares would overflow
    g = torch.randn(n, device=dev)
    g[1234] = float("inf")
    assert math.isinf(_ordered(_partials(afdm, g, 0.5)))
    g[1234] = float("nan")
    assert math.isnan(_ordered(_partials(afdm, g, 1.0)))


SIZES = (1, 3, 4, 4099, 6_000_003)              # the grid of test_gpu_ema.test_adamw_ema_step_bit_exact_against_adamw_step


def _views(n, dev, offset, k, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return [torch.randn(n + offset, device=dev, generator=g)[offset:] for _ in range(k)]


def _adam_inputs(n, dev, offset, seed):
    p, g, m, v, ema = _views(n, dev, offset, 5, seed)
    v = v.abs_()
    m.mul_(0.1)
    return p, g, m, v, ema


def _ctl(dev, lr, coef=1.0, skip=0.0):
    c = torch.zeros(8, device=dev, dtype=torch.float64)
    c[LR], c[COEF], c[SKIP] = float(np.float32(lr)), coef, skip
    return c


@pytest.mark.parametrize("offset", (0, 1))
@pytest.mark.parametrize("n", SIZES)
def test_adamw_ctl_step_bit_exact_against_the_by_value_steps(A, n, offset):
    afdm, dev = A
    from afdm import ops
    L, s = afdm.lib(), ops._stream()
    lr, b1, b2, eps, wd, gs = 3e-4, 0.9, 0.999, 1e-8, 0.01, 0.5
    beta, omb = 0.995, float(1.0 - 0.995)
    for tail in (0, 5):
        n_ema = n + tail
        p, g, m, v, ema = _adam_inputs(n_ema, dev, offset, seed=11 * n + offset + tail)
        p1, m1, v1 = p.clone(), m.clone(), v.clone()                                     # by value, no EMA
        p2, m2, v2, e2 = p.clone(), m.clone(), v.clone(), ema.clone()                    # by value, EMA
        pa, ma, va = _views(n_ema, dev, offset, 3, 1)                                    # ctl, no EMA (same alignment as the others)
        pa.copy_(p); ma.copy_(m); va.copy_(v)
        pb, mb, vb, eb = _views(n_ema, dev, offset, 4, 2)                                # ctl, EMA
        pb.copy_(p); mb.copy_(m); vb.copy_(v); eb.copy_(ema)
        st1, st2 = (torch.zeros(4, device=dev) for _ in range(2))
        es2 = torch.tensor([0, 0], device=dev, dtype=torch.int32)
        ctl = _ctl(dev, lr)
        for k in range(3):                                                               # 3 consecutive steps: copy, blend, blend
            g.copy_(torch.randn(n_ema, device=dev, generator=torch.Generator(device=dev).manual_seed(n + k)))
            L.afd_adamw_tick(st1.data_ptr(), b1, b2, s)
            L.afd_adamw_step(p1.data_ptr(), g.data_ptr(), m1.data_ptr(), v1.data_ptr(), n, st1.data_ptr(), lr, b1, b2, eps, wd, gs, s)
            L.afd_adamw_ctl_step(pa.data_ptr(), g.data_ptr(), ma.data_ptr(), va.data_ptr(), n, st1.data_ptr(), ctl.data_ptr(), b1, b2,
                                 eps, wd, gs, None, 0, None, 0.0, 0.0, s)
            L.afd_adamw_ema_tick(st2.data_ptr(), b1, b2, es2.data_ptr(), 1, s)
            L.afd_adamw_ema_step(p2.data_ptr(), g.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, st2.data_ptr(), lr, b1, b2, eps, wd, gs,
                                 e2.data_ptr(), n_ema, es2.data_ptr(), beta, omb, s)
            L.afd_adamw_ctl_step(pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), n, st2.data_ptr(), ctl.data_ptr(), b1, b2,
                                 eps, wd, gs, eb.data_ptr(), n_ema, es2.data_ptr(), beta, omb, s)
            torch.cuda.synchronize()
            assert torch.equal(pa, p1) and torch.equal(ma, m1) and torch.equal(va, v1), (n, offset, tail, k)
            assert torch.equal(pb, p2) and torch.equal(mb, m2) and torch.equal(vb, v2) and torch.equal(eb, e2), (n, offset, tail, k)
            assert torch.equal(p1[:n], p2[:n])
        assert not torch.equal(p1[:n], p[:n])                                            # something moved
        # skip = 1: every buffer byte for byte unchanged
        skip = _ctl(dev, lr, skip=1.0)
        before = [x.clone() for x in (pa, ma, va, pb, mb, vb, eb)]
        L.afd_adamw_ctl_step(pa.data_ptr(), g.data_ptr(), ma.data_ptr(), va.data_ptr(), n, st1.data_ptr(), skip.data_ptr(), b1, b2, eps,
                             wd, gs, None, 0, None, 0.0, 0.0, s)
        L.afd_adamw_ctl_step(pb.data_ptr(), g.data_ptr(), mb.data_ptr(), vb.data_ptr(), n, st2.data_ptr(), skip.data_ptr(), b1, b2, eps,
                             wd, gs, eb.data_ptr(), n_ema, es2.data_ptr(), beta, omb, s)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((pa, ma, va, pb, mb, vb, eb), before))


def _tick(afdm, dev, state, cfg_kw, parts=None, es=None, start=0, ctl=None):
    from afdm import ops
    from afdm.training import _OptCtl
    d = dict(base_lr=3e-4, warmup=0, total=10, kind=0, min_ratio=0.0, max_norm=0.0, skip_nonfinite=0)
    d.update(cfg_kw)
    cfg = _OptCtl(d["base_lr"], d["warmup"], d["total"], d["kind"], d["min_ratio"], d["max_norm"], d["skip_nonfinite"])
    ctl = torch.zeros(8, device=dev, dtype=torch.float64) if ctl is None else ctl
    afdm.lib().afd_adamw_ctl_tick(state.data_ptr(), 0.9, 0.999, None if es is None else es.data_ptr(), start,
                                  None if parts is None else parts.data_ptr(), 0 if parts is None else parts.numel(),
                                  ctypes.byref(cfg), ctl.data_ptr(), ops._stream())
    return ctl


def test_ctl_tick_schedule_matches_the_host_mirror(A):
    afdm, dev = A
    from afdm import ops
    from afdm.training import _LR_KINDS
    base = 3e-4
    worst = 0
    for kind, warmup, total, min_ratio in schedule_grid():
        sch = afdm.LRSchedule(kind, warmup=warmup, total=total, min_ratio=min_ratio)
        ks = sorted(set(range(min(total, 14) + 3)) | {max(0, total - 1), total, total + 1, total + 2} | {total // 2, total // 3})
        states = torch.zeros(len(ks), 4, device=dev)
        states[:, 0] = torch.tensor(ks, dtype=torch.float32)                          # step count BEFORE the tick = k
        ref = states.clone()
        ctls = torch.zeros(len(ks), 8, device=dev, dtype=torch.float64)
        for i in range(len(ks)):
            _tick(afdm, dev, states[i], dict(base_lr=base, warmup=warmup, total=total, kind=_LR_KINDS[kind], min_ratio=min_ratio),
                  ctl=ctls[i])
            afdm.lib().afd_adamw_tick(ref[i].data_ptr(), 0.9, 0.999, ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(states, ref)                                                # the Adam state: adamw_tick_k's, bit for bit
        got = ctls.cpu().numpy()
        for i, k in enumerate(ks):
            want = np.float32(sch.lr(base, k))
            lr = np.float32(got[i, LR])
            assert float(lr) == got[i, LR]                                             # an fp32 value, widened
            ulps = abs(int(lr.view(np.int32)) - int(want.view(np.int32)))
            worst = max(worst, ulps)
            assert ulps <= 1, (kind, warmup, total, min_ratio, k, lr, want)
            assert got[i, INDEX] == k and got[i, COEF] == 1.0 and got[i, SKIP] == 0.0 and got[i, NORM] == 0.0
            assert abs(got[i, FACTOR] - sch.factor(k)) <= 4e-16
    print("ctl tick: worst lr distance from the host mirror, in fp32 ulps:", worst)


def test_ctl_tick_clip_coefficient_and_skip(A):
    afdm, dev = A
    n_p = afdm.lib().afd_grad_sqnorm_n_partials()
    gen = torch.Generator().manual_seed(5)
    for max_norm in (1.0, 100.0, 0.0, -1.0):
        parts = (torch.rand(n_p, generator=gen, dtype=torch.float64) * 3.0).to(dev)
        state = torch.zeros(4, device=dev)
        ctl = _tick(afdm, dev, state, dict(max_norm=max_norm), parts=parts)
        torch.cuda.synchronize()
        c = ctl.cpu().tolist()
        sq = _ordered(parts)
        assert c[SQ] == sq and abs(c[NORM] - math.sqrt(sq)) <= 1e-15 * math.sqrt(sq)
        want = afdm.clip_coefficient(c[NORM], max_norm)
        assert abs(c[COEF] - want) <= 1e-15 * want, (max_norm, c[COEF], want)
        assert (c[COEF] < 1.0) == (max_norm == 1.0) and c[NORM] > 1.0           # monitoring without clipping still reports the norm
        assert state.tolist()[0] == 1.0 and c[SKIP] == 0.0
    # a few partials only (n_partials is the caller's)
    ctl = _tick(afdm, dev, torch.zeros(4, device=dev), dict(max_norm=1.0), parts=torch.tensor([9.0, 16.0], device=dev, dtype=torch.float64))
    torch.cuda.synchronize()
    assert ctl[NORM].item() == 5.0 and ctl[COEF].item() == 1.0 / (5.0 + 1e-6)
    # skip_nonfinite with an inf (and a NaN) partial: nothing advances, n_skipped counts
    for bad in (float("inf"), float("nan")):
        parts = torch.ones(n_p, device=dev, dtype=torch.float64)
        parts[7] = bad
        state = torch.tensor([4.0, 0.25, 0.5, 0.0], device=dev)
        es = torch.tensor([4, 1], device=dev, dtype=torch.int32)
        ctl = torch.tensor([1e-3, 0.5, 2.0, 0.0, 2.0, 4.0, 3.0, 1.0], device=dev, dtype=torch.float64)
        _tick(afdm, dev, state, dict(max_norm=1.0, skip_nonfinite=1), parts=parts, es=es, start=2, ctl=ctl)
        torch.cuda.synchronize()
        assert state.tolist() == [4.0, 0.25, 0.5, 0.0] and es.tolist() == [4, 1]
        c = ctl.cpu().tolist()
        assert c[SKIP] == 1.0 and c[NSKIP] == 3.0 and not math.isfinite(c[NORM])
        assert c[LR] == 1e-3 and c[COEF] == 0.5 and c[INDEX] == 3.0
        # the same partials without skip_nonfinite: the step is taken, the EMA counter too
        _tick(afdm, dev, state, dict(max_norm=1.0), parts=parts, es=es, start=2, ctl=ctl)
        torch.cuda.synchronize()
        assert state.tolist()[0] == 5.0 and es.tolist() == [5, 0] and ctl[SKIP].item() == 0.0 and ctl[NSKIP].item() == 3.0
        assert (ctl[COEF].item() == 0.0) if math.isinf(bad) else math.isnan(ctl[COEF].item())
    # finite norm with skip_nonfinite: an ordinary tick
    state, es = torch.zeros(4, device=dev), torch.tensor([0, 0], device=dev, dtype=torch.int32)
    ctl = _tick(afdm, dev, state, dict(max_norm=1.0, skip_nonfinite=1), parts=torch.ones(n_p, device=dev, dtype=torch.float64), es=es, start=1)
    torch.cuda.synchronize()
    assert state.tolist()[0] == 1.0 and es.tolist() == [1, 1] and ctl[SKIP].item() == 0.0 and ctl[NSKIP].item() == 0.0


def _cpu_lambda(kind, warmup, total, min_ratio):
    def lam(k):
        if k < warmup:
            return float(k) / float(max(1, warmup))
        if kind == "constant":
            return 1.0
        pr = min(1.0, float(k - warmup) / float(max(1, total - warmup)))
        base = 0.5 * (1.0 + math.cos(math.pi * pr)) if kind == "cosine" else 1.0 - pr
        return min_ratio + (1.0 - min_ratio) * base
    return lam


@pytest.mark.parametrize("max_norm,clips", ((1.0, True), (100.0, False), (None, False)))
def test_optimiser_parity_with_clip_grad_norm_adamw_lambda_lr(A, max_norm, clips):
    afdm, dev = A
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(0)
    lin = torch.nn.Linear(37, 11)
    ref = torch.nn.Linear(37, 11)
    ref.load_state_dict(lin.state_dict())
    lin = lin.to(dev)
    sch = afdm.LRSchedule("cosine", warmup=3, total=10, min_ratio=0.1)
    opt = afdm.FusedAdamW(lin, lr=3e-4, max_grad_norm=max_norm, lr_schedule=sch)
    ropt = torch.optim.AdamW(ref.parameters(), lr=3e-4)
    rsched = torch.optim.lr_scheduler.LambdaLR(ropt, _cpu_lambda("cosine", 3, 10, 0.1))
    for s in range(12):
        gw, gb = torch.randn(11, 37, generator=g), torch.randn(11, generator=g)
        opt.zero_grad()
        lin.weight.grad.copy_(gw.to(dev)); lin.bias.grad.copy_(gb.to(dev))
        opt.step()
        ref.weight.grad, ref.bias.grad = gw.clone(), gb.clone()
        lr_ref = ropt.param_groups[0]["lr"]
        if max_norm is not None:
            total = float(torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm))
            assert (total > max_norm) == clips                       # the regime this case is meant to be in
            assert abs(opt.last_grad_norm - total) <= 1e-6 * total
        else:
            assert opt.last_grad_norm is None and opt.partials is None
        ropt.step()
        rsched.step()
        assert abs(opt.last_lr - lr_ref) <= LR_TOL * lr_ref, (s, opt.last_lr, lr_ref)
    ew, eb = rel_l2(lin.weight.detach().cpu(), ref.weight.detach()), rel_l2(lin.bias.detach().cpu(), ref.bias.detach())
    print(f"clip+schedule optimiser parity (max_norm={max_norm}): weight {ew:.3e} bias {eb:.3e}")
    note("FusedAdamW clip+schedule vs torch CPU", max(ew, eb), f"max_norm={max_norm}")
    assert ew < 1e-6 and eb < 1e-6
    assert opt.n_skipped == 0 and opt.state[0].item() == 12.0


def _setup(afdm, dev):
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    return model, afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)


def _inputs(dev):
    g = load_golden("train_step.npz")
    images = T(g["images"]).to(dev)
    b = [(T(g["t0"]), T(g["eps0"]).to(dev)), (T(g["t1"]), T(g["eps1"]).to(dev)), (T(g["t0"]), T(g["eps1"]).to(dev))]
    return images, [b[0], b[1], b[2], b[1], b[0]]                    # 5 steps with fixed t / eps


def _first_norm(afdm, dev, images, batches):
    model, diff = _setup(afdm, dev)
    step = afdm.TrainStep(model, diff, lr=3e-4, track_grad_norm=True)
    step(images, t=batches[0][0], eps=batches[0][1])
    norm = step.last_grad_norm
    want = float(torch.linalg.vector_norm(step.opt.fp.grad[:step.opt.fp.n_active].double()))
    assert abs(norm - want) <= 1e-6 * want
    return norm


@pytest.mark.parametrize("with_ema", (False, True))
def test_train_step_clip_and_schedule_in_every_launch_mode(A, with_ema):
    afdm, dev = A
    images, batches = _inputs(dev)
    norm0 = _first_norm(afdm, dev, images, batches)
    max_norm = 0.5 * norm0                                           # below the first step's measured norm: it clips
    print("first step's gradient norm", norm0)
    got = {}
    for mode in (False, True, "lanes"):
        model, diff = _setup(afdm, dev)
        kw = {}
        if with_ema:
            kw = dict(ema=afdm.EMA(0.9), ema_model=copy.deepcopy(model), ema_start=1)
        sch = afdm.LRSchedule("cosine", warmup=2, total=5, min_ratio=0.1)
        step = afdm.TrainStep(model, diff, lr=3e-4, graph=mode, max_grad_norm=max_norm, lr_schedule=sch, **kw)
        lrs, coefs = [], []
        for k, (t, e) in enumerate(batches):
            step(images, t=t, eps=e)
            assert abs(step.last_lr - sch.lr(3e-4, k)) <= LR_TOL * sch.lr(3e-4, k), (mode, k)      # the schedule advances inside replays
            lrs.append(step.last_lr)
            coefs.append(step.opt.ctl[COEF].item())
            fp = step.opt.fp
            want = float(torch.linalg.vector_norm(fp.grad[:fp.n_active].double()))
            assert abs(step.last_grad_norm - want) <= 1e-6 * want, (mode, k)
            assert coefs[-1] == afdm.clip_coefficient(step.last_grad_norm, max_norm)
        assert coefs[0] < 1.0 and step.n_skipped == 0 and step.opt.ctl[INDEX].item() == 4.0
        assert step.opt.state[0].item() == 5.0
        torch.cuda.synchronize()
        got[mode] = (step.opt.fp.flat.clone(), step.opt.m.clone(), step.opt.v.clone(), step.opt.ctl.clone(),
                     step._ema_home.flat.clone() if with_ema else None, step._ema_home.state.tolist() if with_ema else None)
    for mode in (True, "lanes"):
        for i, tag in enumerate(("params", "m", "v", "ctl", "ema")):
            if got[mode][i] is None:
                continue
            print(f"{mode} vs eager, {tag}: rel-L2 {rel_l2(got[mode][i].cpu(), got[False][i].cpu()):.3e}")
    for mode in (True, "lanes"):
        for i, tag in enumerate(("params", "m", "v", "ctl", "ema")):
            if got[mode][i] is not None:
                assert torch.equal(got[mode][i], got[False][i]), (mode, tag)
        assert got[mode][5] == got[False][5]
    if with_ema:
        assert got[False][5] == [5, 0]


def test_new_path_with_nothing_to_do_equals_the_default_step(A):
    afdm, dev = A
    images, batches = _inputs(dev)
    out = []
    for kw in ({}, dict(lr_schedule=afdm.LRSchedule("constant"), track_grad_norm=True)):
        model, diff = _setup(afdm, dev)
        step = afdm.TrainStep(model, diff, lr=3e-4, **kw)
        for t, e in batches[:3]:
            step(images, t=t, eps=e)
        torch.cuda.synchronize()
        out.append((step.opt.fp.flat.clone(), step.opt.m.clone(), step.opt.v.clone()))
        assert (step.opt.ctl is None) == (not kw)
    assert all(torch.equal(a, b) for a, b in zip(*out))              # new path == old path, bit for bit


def test_default_step_keeps_its_launches_and_clipping_adds_one(A):
    """Replay lists (work nodes, main lane, side lane, cross-lane waits).  The waits are what is left after the replay builder
    drops the implied ones, which depends on the order the runtime lists the nodes in: only the launches are compared."""
    afdm, dev = A
    images, batches = _inputs(dev)
    counts = {}
    for tag, kw in (("default", {}), ("schedule", dict(lr_schedule=afdm.LRSchedule("cosine", warmup=2, total=5))),
                    ("clip", dict(max_grad_norm=1.0)),
                    ("ema", "ema"), ("ema+clip", "ema")):
        model, diff = _setup(afdm, dev)
        if kw == "ema":
            kw = dict(ema=afdm.EMA(0.9), ema_model=copy.deepcopy(model), ema_start=1)
            if tag == "ema+clip":
                kw.update(max_grad_norm=1.0, lr_schedule=afdm.LRSchedule("linear", total=5))
        step = afdm.TrainStep(model, diff, lr=3e-4, graph="lanes", **kw)
        step(images, t=batches[0][0], eps=batches[0][1])
        counts[tag] = step.lanes_counts
        n, n_main, n_side, n_wait = step.lanes_counts
        assert n == n_main + n_side and 2 <= n_wait <= n_side
    print("lanes_counts", counts)
    n, n_main, n_side, _ = counts["default"]
    assert (n, n_main, n_side) == (303, 221, 82)                           # the default step's replay list, as before this feature
    assert counts["schedule"][:3] == counts["ema"][:3] == (n, n_main, n_side)      # a schedule alone: the same number of launches
    assert counts["clip"][:3] == counts["ema+clip"][:3] == (n + 1, n_main + 1, n_side)      # the norm pass: one more, on the main lane


def test_skip_nonfinite_drops_the_whole_update(A):
    afdm, dev = A
    torch.manual_seed(0)
    lin = torch.nn.Linear(37, 11).to(dev)
    opt = afdm.FusedAdamW(lin, lr=1e-2, skip_nonfinite=True)
    g = torch.Generator().manual_seed(3)
    opt.zero_grad()
    lin.weight.grad.copy_(torch.randn(11, 37, generator=g).to(dev))
    opt.step()
    snap = [x.clone() for x in (opt.fp.flat, opt.m, opt.v, opt.state)]
    for bad in (float("inf"), float("nan")):
        opt.zero_grad()
        lin.weight.grad.copy_(torch.randn(11, 37, generator=g).to(dev))
        lin.weight.grad[3, 5] = bad
        opt.step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((opt.fp.flat, opt.m, opt.v, opt.state), snap))
        assert not math.isfinite(opt.last_grad_norm)
    assert opt.n_skipped == 2
    opt.zero_grad()
    lin.weight.grad.copy_(torch.randn(11, 37, generator=g).to(dev))
    opt.step()
    torch.cuda.synchronize()
    assert opt.state[0].item() == 2.0 and not torch.equal(opt.fp.flat, snap[0]) and opt.n_skipped == 2
    assert torch.isfinite(opt.fp.flat).all()


def test_two_rank_clip_equals_single_rank(A, tmp_path):
    afdm, dev = A
    images, batches = _inputs(dev)
    max_norm = 0.5 * _first_norm(afdm, dev, images, batches)         # clips the first step
    out = tmp_path / "clip_ddp"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561", PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29561", os.path.join(ROOT, "tests", "clip_ddp_worker.py"), "--out", str(out),
           "--max-norm", repr(max_norm)]
    subprocess.run(cmd, check=True, env=env, timeout=600)
    r0, r1 = (torch.load(f"{out}.{r}", weights_only=True) for r in (0, 1))
    assert torch.equal(r0["ctl"], r1["ctl"]) and torch.equal(r0["params"], r1["params"])      # same bytes: no collective needed
    assert r0["ctl"][COEF].item() < 1.0 and r0["ctl"][INDEX].item() == 1.0
    model, diff = _setup(afdm, dev)
    assert r0["max_norm"] == max_norm
    step = afdm.TrainStep(model, diff, lr=3e-4, max_grad_norm=max_norm,
                          lr_schedule=afdm.LRSchedule("linear", warmup=0, total=4, min_ratio=0.1))
    for t, e in batches[:2]:
        step(images, t=t, eps=e)
    torch.cuda.synchronize()
    err = rel_l2(r0["params"], step.opt.fp.flat.cpu())
    en = abs(r0["ctl"][NORM].item() - step.last_grad_norm) / step.last_grad_norm
    print("2-rank vs 1-rank with clipping: params rel-L2", err, "norm rel", en)
    assert err < 1e-6 and en < 1e-5


def test_ddpm_run_with_clipping_and_schedule(A, tmp_path, monkeypatch):
    afdm, dev = A
    rng = np.random.default_rng(0)
    csvp = tmp_path / "mnist.csv"
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    np.savetxt(csvp, arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
    monkeypatch.chdir(tmp_path)
    params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
              "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(csvp),
              "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
              "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
    run = "DDPM_Uncondtional_MNIST_3"
    settings = tmp_path / "runs" / run / "settings_MNIST_3.txt"
    afdm.ddpm_run(dict(params))
    plain = settings.read_text()
    assert "max_grad_norm" not in plain and "lr_" not in plain.replace("lr: ", "")
    assert plain.splitlines()[-1].startswith("omega_c_up: ")                 # the parent's last line: nothing appended
    afdm.ddpm_run(dict(params, max_grad_norm=1.0, lr_warmup=1, lr_schedule="cosine", lr_min_ratio=0.1))
    text = settings.read_text()
    assert text.startswith(plain)
    assert text[len(plain):] == "\nmax_grad_norm: 1.0\nlr_warmup: 1\nlr_schedule: cosine\nlr_min_ratio: 0.1"
    assert (tmp_path / "models" / run / "ckpt_MNIST_3.pt").exists() and (tmp_path / "results" / run / "0.jpg").exists()
