"""Cost of one progressive-distillation step on one MI355X (variant-3 UNet at 32 x 32, B = 256: Config D).

    python tools/distill_bench.py [--mode eager|graph|lanes] [--windows 30] [--out FILE.json]

One process, one JSON line.  Alternating windows of 10 (after 10 warm-up steps each; medians over W windows with the fastest
window and the 90th percentile as the spread, the method of tools/objective_bench.py):
  distill_ms   a DistillStep call (v-prediction, cosine schedule, truncated-SNR weights, the 8-step chain): the inner TrainStep,
               the teacher's two eval forwards and the three elementwise launches;
  pieces_ms    what the parent commit already had, on the same batch: one TrainStep call of the same objective plus two eval
               forwards of a second copy of the model under no_grad.  distill_ms - pieces_ms is what the feature adds: the
               noising, the two target kernels and the step-index gather.
Then the two target kernels alone with events over 200 back-to-back launches each, against their byte counts (12 and 20 bytes per
element).  Alternating keeps both sides beside the same neighbours on a shared machine."""
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
    chain = diff.ddim_timesteps(8)
    distill = afdm.DistillStep(copy.deepcopy(teacher), teacher, diff, chain, lr=1e-4, graph=MODES[mode])
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

    sides = {"distill": lambda: distill(images), "pieces": pieces}
    for fn in sides.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    w = {k: [] for k in sides}
    for _ in range(W):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                loss = fn()
            torch.cuda.synchronize()
            w[k].append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    row = {"mode": mode, "B": B, "windows": W, "loss": float(loss)}
    for k in sides:
        row[f"{k}_ms"], row[f"{k}_ms_min"], row[f"{k}_ms_p90"] = _spread(w[k])
    row["added_ms"] = round(row["distill_ms"] - row["pieces_ms"], 4)
    # the two kernels alone, back to back on the same tensors
    out, z = torch.randn_like(images), torch.randn_like(images)
    z_mid, x_t, e_t = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    k = torch.randint(0, 4, (B,))
    tt, tm, tp = (tab[k].to(dev) for tab in diff.distill_levels(chain))
    n = images.numel()
    row["mid_us"], row["mid_us_min"], row["mid_us_p90"] = _kernel_us(
        torch, lambda: ops.distill_mid(out, z, tt, tm, diff.alpha_hat, "v", out=z_mid))
    row["target_us"], row["target_us_min"], row["target_us_p90"] = _kernel_us(
        torch, lambda: ops.distill_target(out, z_mid, z, tt, tm, tp, diff.alpha_hat, "v", x_out=x_t, eps_out=e_t))
    row["mid_bytes"], row["target_bytes"] = 12 * n, 20 * n
    row["mid_TBps"] = round(12 * n / (row["mid_us"] * 1e-6) / 1e12, 3)
    row["target_TBps"] = round(20 * n / (row["target_us"] * 1e-6) / 1e12, 3)
    print(json.dumps(row), flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump(row, fh, indent=1)


if __name__ == "__main__":
    main()
