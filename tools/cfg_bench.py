"""ms per denoise step of the class-conditional / guided sampler, variant 3 at 32 x 32: median over windows of ONE configuration
in this process (run the configurations as separate processes).
    python tools/cfg_bench.py --mode {uncond,cond,cfg,cfg2} --n N [--graph] [--windows 30]
uncond: the unconditional step (timestep tables on, as Diffusion.sample runs it); cond: labels, cfg_scale = 0 (one n-row
forward with the label embedding, so the time embedding is computed every step); cfg: guidance as Diffusion.sample runs it
(ONE 2n-row forward + afd_denoise_step_cfg writing both halves of the 2n input); cfg2: guidance the upstream way (two n-row
forwards, torch.lerp, ops.denoise_step).  --graph: the step captured once and replayed, as Diffusion.sample(graph=True) does (Diffusion._capture)."""
import gc
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import afdm  # noqa: E402
from afdm import ops  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


mode, n, W = arg("--mode", "cfg"), arg("--n", 6), arg("--windows", 30)
use_graph = "--graph" in sys.argv
assert mode in ("uncond", "cond", "cfg", "cfg2"), mode
dev = torch.device("cuda:0")
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
afdm.set_seed(42)
model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=F_SET, device=dev, variant=3, num_classes=10).to(dev)
diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
S = 0.0 if mode in ("uncond", "cond") else 3.0
labels = (torch.arange(n, device=dev) % 10)
y2 = torch.cat([labels, torch.full_like(labels, afdm.NULL_LABEL)])
rows = 2 * n if mode == "cfg" else n
xs = torch.randn(rows, 3, 32, 32, device=dev)
if mode == "cfg":
    xs[n:].copy_(xs[:n])
xh = xs[:n]
t_dev = torch.full((rows,), 500, device=dev, dtype=torch.long)


def one_step():
    noise = torch.randn_like(xh)
    if mode == "uncond":
        eps = model(xs, t_dev)
        ops.denoise_step_dev(xs, eps, noise, diff.alpha, diff.alpha_hat, diff.beta, t_dev, xs)
    elif mode == "cond":
        eps = model(xs, t_dev, labels)
        ops.denoise_step_dev(xs, eps, noise, diff.alpha, diff.alpha_hat, diff.beta, t_dev, xs)
    elif mode == "cfg":
        eps2 = model(xs, t_dev, y2)
        ops.denoise_step_cfg_dev(xh, eps2, noise, diff.alpha, diff.alpha_hat, diff.beta, t_dev, S, xh, xs[n:])
    else:
        ec = model(xs, t_dev, labels)
        eu = model(xs, t_dev)
        ops.denoise_step_dev(xs, torch.lerp(eu, ec, S), noise, diff.alpha, diff.alpha_hat, diff.beta, t_dev, xs)


diff._hint(model)            # as inside Diffusion.sample: the unconditional forward gathers tabulated time embeddings
model.eval()
with torch.no_grad():
    if use_graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one_step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one_step()
        run = g.replay
    else:
        run = one_step
    for _ in range(20):
        xs.normal_()                 # keep the values in range (the step index does not move)
        run()
    gc.collect()
    gc.disable()
    w = []
    for _ in range(W):
        xs.normal_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 20 * 1e3)
s_ = sorted(w)
print(f"cfg_bench mode={mode} n={n} graph={int(use_graph)}: median {s_[len(s_) // 2]:.3f} min {s_[0]:.3f} "
      f"p90 {s_[int(len(s_) * 0.9)]:.3f} ms/step", flush=True)
