"""Cost of consistency distillation and of a consistency sampling step on one MI355X (variant-3 UNet at 32 x 32: Config D).

    python tools/consistency_bench.py [--mode eager|graph|lanes] [--windows 30] [--out FILE.json]

One process, one JSON line.  Three parts (the method of tools/distill_bench.py):
  1. the three kernels alone at n = 6 and n = 256 rows of 3 x 32 x 32, events over 200 back-to-back launches each, against the
     same expressions written as torch ops in fp64 on the device (what a caller without the kernels would run), and against
     their byte counts (fn 12, target 20, step 16 bytes per element);
  2. alternating windows of 10 steps at B = 256 (after 10 warm-up steps each; medians over W windows, the fastest window and the
     90th percentile as the spread):
       consistency_ms   a ConsistencyStep call (v-prediction, cosine schedule, truncated-SNR weights, the 8-step chain): the inner
                        TrainStep with its fused EMA, the teacher's and the target network's eval forwards and the three
                        elementwise launches;
       pieces_ms        what the parent commit already had, on the same batch: one TrainStep call of the same objective plus two
                        eval forwards of a second copy of the model under no_grad.  consistency_ms - pieces_ms is what the
                        feature adds: the noising, the teacher's move, the target kernel, the gather and the EMA's traffic;
  3. a consistency sampling step against a DDIM step at n = 6 and n = 256: one forward plus the fused update each, windows as in 2.
Alternating keeps both sides beside the same neighbours on a shared machine."""
import gc
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
B = 256
MODES = {"eager": False, "graph": True, "lanes": "lanes"}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _spread(w):
    w = sorted(w)
    return round(w[len(w) // 2], 4), round(w[0], 4), round(w[int(len(w) * 0.9)], 4)


def _kernel_us(torch, fn, reps=200):
    for _ in range(10):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    us = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
    return round(us[reps // 2], 2), round(us[0], 2), round(us[int(reps * 0.9)], 2)


def _windows(torch, sides, W):
    """{name: [ms per call of each of W alternating windows of 10]} and the last value returned"""
    for fn in sides.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    w, last = {k: [] for k in sides}, None
    for _ in range(W):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                last = fn()
            torch.cuda.synchronize()
            w[k].append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    return w, last


def _torch_forms(torch, diff, coef, kind="v"):
    """The three kernels' expressions as torch ops: fp64 on the device, rounded once (v-prediction)."""
    ah = diff.alpha_hat.double()

    def level(t):
        a = ah[t].view(-1, 1, 1, 1)
        return a.sqrt(), (1 - a).sqrt()

    def cc(t):
        c = coef[t]
        return c[:, 0].view(-1, 1, 1, 1), c[:, 1].view(-1, 1, 1, 1)

    def f64(out, z, t):
        (al, sg), (cs, co) = level(t), cc(t)
        z = z.double()
        return torch.where(co == 0, z, cs * z + co * (al * z - sg * out.double()))

    def fn(out, z, t):
        return f64(out, z, t).float()

    def target(out_tgt, z_prev, z_t, t, t_prev):
        (al, sg), (cs, co) = level(t), cc(t)
        z = z_t.double()
        x = (f64(out_tgt, z_prev, t_prev) - cs * z) / co
        return x.float(), ((z - al * x) / sg).float()

    def step(out, z, noise, t, t_next):
        f = fn(out, z, t)
        a = diff.alpha_hat[t_next].view(-1, 1, 1, 1)
        return a.sqrt() * f + (1 - a).sqrt() * noise

    return fn, target, step


def main():
    import copy
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    from afdm import ops
    mode, W = arg("--mode", "eager"), arg("--windows", 30)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    teacher = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction="v")
    ah, coef = diff.alpha_hat, diff.consistency_coefficients().to(dev)
    chain = diff.ddim_timesteps(8)
    row = {"mode": mode, "B": B, "windows": W}

    # 1. the kernels alone
    t_fn, t_target, t_step = _torch_forms(torch, diff, coef)
    for n in (6, B):
        out, z, zp, noise = (torch.randn(n, 3, 32, 32, device=dev) for _ in range(4))
        o1, o2 = torch.empty_like(z), torch.empty_like(z)
        k = torch.randint(0, len(chain), (n,))
        tt, tp = (tab[k].to(dev) for tab in diff.consistency_levels(chain))
        t_rows, tn_rows = (torch.full((n,), v, device=dev, dtype=torch.long) for v in (500, 143))
        cases = {
            "fn": (12, lambda: ops.consistency_fn(out, z, tt, ah, coef, "v", f_out=o1), lambda: t_fn(out, z, tt)),
            "target": (20, lambda: ops.consistency_target(out, zp, z, tt, tp, ah, coef, "v", x_out=o1, eps_out=o2),
                       lambda: t_target(out, zp, z, tt, tp)),
            "step": (16, lambda: ops.consistency_step(out, z, noise, ah, coef, "v", 500, 143, x_out=o1),
                     lambda: t_step(out, z, noise, t_rows, tn_rows)),
        }
        for name, (bpe, kern, torch_form) in cases.items():
            key = f"{name}_n{n}"
            row[f"{key}_us"], row[f"{key}_us_min"], row[f"{key}_us_p90"] = _kernel_us(torch, kern)
            row[f"{key}_torch_us"], _, row[f"{key}_torch_us_p90"] = _kernel_us(torch, torch_form)
            row[f"{key}_TBps"] = round(bpe * z.numel() / (row[f"{key}_us"] * 1e-6) / 1e12, 3)

    # 2. the training step against its pieces
    cstep = afdm.ConsistencyStep(copy.deepcopy(teacher), teacher, diff, chain, lr=1e-4, graph=MODES[mode])
    plain = afdm.TrainStep(copy.deepcopy(teacher), diff, lr=1e-4, graph=MODES[mode], loss_weighting="truncated_snr")
    other = copy.deepcopy(teacher).eval()
    images = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    t = torch.full((B,), 500, device=dev, dtype=torch.long)

    def pieces():
        loss = plain(images)
        with torch.no_grad():
            other(images, t)
            other(images, t)
        return loss

    sides = {"consistency": lambda: cstep(images), "pieces": pieces}
    w, loss = _windows(torch, sides, W)
    row["loss"] = float(loss)
    for k in sides:
        row[f"{k}_ms"], row[f"{k}_ms_min"], row[f"{k}_ms_p90"] = _spread(w[k])
    row["added_ms"] = round(row["consistency_ms"] - row["pieces_ms"], 4)
    del cstep, plain
    torch.cuda.empty_cache()

    # 3. a consistency sampling step against a DDIM step: one forward and the fused update each
    net = other
    for n in (6, B):
        x, noise = torch.randn(n, 3, 32, 32, device=dev), torch.randn(n, 3, 32, 32, device=dev)
        t_rows = torch.full((n,), 500, device=dev, dtype=torch.long)
        xo = torch.empty_like(x)

        def c_step():
            with torch.no_grad():
                ops.consistency_step(net(x, t_rows).contiguous(), x, noise, ah, coef, "v", 500, 143, x_out=xo)

        def d_step():
            with torch.no_grad():
                ops.ddim_step(x, diff.predict_eps(net, x, t_rows), None, ah, 500, 143, 0.0, out=xo)

        sides = {"consistency": c_step, "ddim": d_step}
        w, _ = _windows(torch, sides, W)
        for k in sides:
            row[f"sample_{k}_n{n}_ms"], row[f"sample_{k}_n{n}_ms_min"], row[f"sample_{k}_n{n}_ms_p90"] = _spread(w[k])
    print(json.dumps(row), flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
