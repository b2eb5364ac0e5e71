"""Cost of the equivariance scores (Diffusion.equivariance), variant 3 at 32 x 32, one MI355X.

    python tools/equiv_bench.py [--out FILE.json] [--images N]

n = 64 images, J = 4 timesteps, K = 8 transforms, batch 256: 256 base rows and 2048 transformed rows, 9 forwards of 256 rows.
Three things are timed in one process, alternating, each the median of 5 calls after a warm-up call (a host clock around work
that ends in a device-to-host copy or a synchronise):
  fused     Diffusion.equivariance: one prefilter per field, row-wise resampling, the fused fp64 comparison;
  composed  the straightforward composition of the public single-transform ops it replaces: per transform one
            rotate_spline3_wrap / affine_spline3_wrap of the noised inputs and one of the base outputs (a prefilter each,
            results in fp32), the same forwards, and a torch masked mean;
  forwards  the 9 UNet forwards alone on the same row counts.
share_outside_forwards = 1 - forwards / fused.  Prints one JSON line."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
SPECS = [("translate", 1, 0), ("translate", 8, 8), ("translate", 0.5, 0.5), ("translate", 0.25, -0.75), ("rotate", 5), ("rotate", 10),
         ("rotate", 45), ("rotate", 90)]
TS = [50, 250, 500, 900]
BATCH = 256


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import afdm
    from afdm import ops
    n = arg("--images", 64)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    g = torch.Generator().manual_seed(0)
    x0 = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    J, K = len(TS), len(SPECS)
    eps = torch.randn(n * J, 3, 32, 32, generator=g).to(dev)
    aff = diff.equivariance_transforms(SPECS).numpy()
    masks = [torch.from_numpy(diff.equivariance_mask(a, 32, 32, 4.0)).to(dev) for a in aff]
    img0 = torch.arange(n).repeat_interleave(J).to(dev)
    t0 = torch.tensor(TS).repeat(n).to(dev)
    x0d = x0.to(dev)

    class Noise:
        def __init__(self):
            self.at = 0

        def __call__(self, shape):
            z = eps[self.at:self.at + shape[0]]
            self.at += shape[0]
            return z

    def fused():
        return diff.equivariance(model, x0, TS, SPECS, batch=BATCH, noise_fn=Noise())["mse"]

    def single(x, i):
        sp = SPECS[i]
        return ops.rotate_spline3_wrap(x, sp[1]) if sp[0] == "rotate" else ops.affine_spline3_wrap(x, aff[i][:4].reshape(2, 2), aff[i][4:])

    def forward(x):
        return torch.cat([model(x[lo:hi], t0[lo:hi]) for lo, hi in diff.bpd_chunks(x.shape[0], BATCH)])

    def composed():
        diff._hint(model)
        model.eval()
        out = torch.empty(n * J, K, dtype=torch.float64, device=dev)
        with torch.no_grad():
            xt = ops.noise_images_gather(x0d, img0, eps, t0, diff.alpha_hat)
            f = forward(xt)
            for i in range(K):
                d = (forward(single(xt, i)) - single(f, i)).double()
                out[:, i] = (d * d * masks[i]).sum(dim=(1, 2, 3)) / (3 * masks[i].sum())
        model.train()
        diff._unhint(model)
        return out.view(n, J, K).cpu()

    def forwards():
        diff._hint(model)
        model.eval()
        with torch.no_grad():
            xt = ops.noise_images_gather(x0d, img0, eps, t0, diff.alpha_hat)
            for _ in range(K + 1):
                forward(xt)
        model.train()
        diff._unhint(model)
        torch.cuda.synchronize()

    fns = {"fused": fused, "composed": composed, "forwards": forwards}
    res = {k: fn() for k, fn in fns.items()}                              # warm-up: every shape of the timed calls
    times = {k: [] for k in fns}
    for _ in range(5):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            times[k].append(time.perf_counter() - t)
    med = {k: sorted(v)[2] for k, v in times.items()}
    a, b = res["fused"].numpy(), res["composed"].numpy()
    rel = float(np.max(np.abs(a - b) / np.abs(a)))                       # the composed reference is rounded to fp32: not equal
    line = {"images": n, "J": J, "K": K, "batch": BATCH, "rows": n * J * (K + 1),
            "fused_ms": round(1e3 * med["fused"], 3), "composed_ms": round(1e3 * med["composed"], 3),
            "forwards_ms": round(1e3 * med["forwards"], 3),
            "fused_ms_spread": [round(1e3 * min(times["fused"]), 3), round(1e3 * max(times["fused"]), 3)],
            "composed_ms_spread": [round(1e3 * min(times["composed"]), 3), round(1e3 * max(times["composed"]), 3)],
            "share_outside_forwards": round(1 - med["forwards"] / med["fused"], 4),
            "composed_share_outside_forwards": round(1 - med["forwards"] / med["composed"], 4),
            "mse_worst_rel_diff_fused_vs_composed": rel}
    print(json.dumps(line), flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
