"""Inpainting (RePaint) cost against sampling, variant 3 at 32 x 32, one MI355X.

    python tools/inpaint_bench.py [--out FILE.json] [--reps 5]

Prints one JSON line per measurement and, with --out, writes them all to FILE.json:
  step        ms per down-move of `Diffusion.inpaint` (half the pixels known, no jumps) against ms per step of
              `Diffusion.sample`, eager, at n = 6 and n = 256, for the DDPM chain and DDIM S = 50 (eta = 1).  Each figure is
              the median over --reps whole trajectories divided by their forward count; the two samplers alternate so that
              drift hits both.  The DDPM chain is timed with T = 101 (100 forwards): a step costs what it costs at T = 1000.
  kernel      us per launch of the masked update against the plain one (HIP events over 200 back-to-back launches,
              median of 5 such windows), at n = 256 images: the DDPM and DDIM steps, and afd_renoise.
  jumps       RePaint's setting r = 10, j = 10 over DDIM S = 250 at n = 6: trajectory time, forwards, and ms per forward,
              against r = 1.
"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    import afdm
    from afdm import ops
    reps = arg("--reps", 5)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    mask = torch.zeros(1, 1, 32, 32)
    mask[..., :16] = 1
    for n in (6, 256):
        images = torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1
        for chain in ("ddpm", "ddim50"):
            diff = afdm.Diffusion(noise_steps=101 if chain == "ddpm" else 1000, img_size=32, device=dev)
            kw = {} if chain == "ddpm" else {"steps": 50, "eta": 1.0}
            forwards = 100 if chain == "ddpm" else 50
            samp = lambda: diff.sample(model, n=n, image_channels=3, **kw)
            inp = lambda: diff.inpaint(model, images, mask, **kw)
            samp(), inp()                                     # warm-up (allocator, embedding tables, graph-free caches)
            ts, ti = [], []
            for _ in range(reps):
                ts.append(timed(samp))
                ti.append(timed(inp))
            s_ms, i_ms = 1e3 * statistics.median(ts) / forwards, 1e3 * statistics.median(ti) / forwards
            emit({"what": "step", "n": n, "chain": chain, "sample_ms": round(s_ms, 4), "inpaint_ms": round(i_ms, 4),
                  "ratio": round(i_ms / s_ms, 4)})

    # the update kernels alone
    n = 256
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    shape = (n, 3, 32, 32)
    x, e, z, x0 = (torch.randn(shape, device=dev) for _ in range(4))
    m = (torch.rand(shape, device=dev) < 0.5).to(torch.uint8)
    out = torch.empty_like(x)
    launches = {
        "ddpm_plain": lambda: ops.denoise_step(x, e, z, diff.alpha, diff.alpha_hat, diff.beta, 500, out),
        "ddpm_masked": lambda: ops.denoise_step_masked(x, e, z, x0, m, diff.alpha, diff.alpha_hat, diff.beta, 500, out),
        "ddim_plain": lambda: ops.ddim_step(x, e, z, diff.alpha_hat, 500, 480, 1.0, out),
        "ddim_masked": lambda: ops.ddim_step_masked(x, e, z, x0, m, diff.alpha_hat, 500, 480, 1.0, out),
        "renoise": lambda: ops.renoise(x, z, diff.alpha_hat, 480, 680, out),
    }
    for name, fn in launches.items():
        for _ in range(20):
            fn()
        wins = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(200):
                fn()
            b.record()
            b.synchronize()
            wins.append(a.elapsed_time(b) * 1e3 / 200)
        emit({"what": "kernel", "name": name, "n_images": n, "us": round(statistics.median(wins), 3)})

    # RePaint's resampling setting
    n = 6
    images = torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    chain = diff.ddim_timesteps(250)
    res = {}
    for r in (1, 10):
        fwd = sum(1 for a, b in diff.repaint_moves(chain, 10, r) if a > b)
        run = lambda: diff.inpaint(model, images, mask, steps=250, eta=1.0, jump_length=10, jump_n_sample=r)
        run()
        ts = [timed(run) for _ in range(3)]
        res[r] = (statistics.median(ts), fwd)
        emit({"what": "jumps", "n": n, "S": 250, "j": 10, "r": r, "traj_s": round(res[r][0], 4), "forwards": fwd,
              "ms_per_forward": round(1e3 * res[r][0] / fwd, 4)})
    emit({"what": "jumps_ratio", "time_ratio": round(res[10][0] / res[1][0], 3), "forward_ratio": round(res[10][1] / res[1][1], 3)})

    out_path = arg("--out", "")
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
