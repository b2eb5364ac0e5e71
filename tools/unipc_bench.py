"""UniPC sampling: the update's cost, the cost of a sampling step against DPM-Solver++(2M), and the accuracy table of DESIGN.md
section 6z, variant 3 at 32 x 32, T = 1000, one MI355X.

    python tools/unipc_bench.py [--out FILE.json] [--windows 15] [--steps 50]

One process, three parts, each printed as a table and, with --out, written as JSON:
  update    microseconds per `ops.unipc_step` (a third-order row, every weight non-zero) at n = 6 and n = 256 images of
            3 x 32 x 32, against the same two expressions in torch ops (the 21 elementwise launches of the fp32 restatement);
            device events around 200 calls, the median of --windows windows.
  step      milliseconds per sampling step of `Diffusion.sample` at n = 6 and n = 256: whole trajectories of --steps steps
            (x_T included) for "unipc_3", "unipc_2" and "dpmpp_2m" on the same timesteps, run alternately, a host clock around a
            trajectory that ends in a device synchronise, the median of --windows rounds, over the number of steps.
  accuracy  the endpoint rel-L2 error against the closed-form solution of the probability-flow ODE of Gaussian data (the data set
            of tests/test_gpu_dpm.py), S in 8 .. 40, for DDIM (eta = 0), DPM++(2M), UniPC-2 and UniPC-3 on `logsnr_timesteps(S)`.
A part that fails ends the run: nothing further is started on the device."""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
T = 1000
NS = (6, 256)
ACC_S = (8, 10, 12, 16, 20, 40)
SOLVERS = ("unipc_3", "unipc_2", "dpmpp_2m")


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def update_cost(torch, ops, diff, dev, W):
    table = diff.unipc_coefficients(diff.dpmpp_pairs(20), 3).to(dev)
    c = table[9].clone()
    cl = [float(v) for v in c]
    rows = []
    for n in NS:
        x, e, xc = (torch.randn(n, 3, 32, 32, device=dev) for _ in range(3))
        hist = torch.randn(3, n, 3, 32, 32, device=dev)
        out = torch.empty_like(x)

        def fused():
            ops.unipc_step(x, e, xc, hist, c, out)

        def torch_ops():
            h1, h2, h3 = hist[2], hist[1], hist[0]
            m = (x - cl[1] * e) / cl[0]
            nc = cl[2] * xc + cl[3] * m + cl[4] * h1 + cl[5] * h2 + cl[6] * h3
            xc.copy_(nc)
            out.copy_(cl[7] * nc + cl[8] * m + cl[9] * h1 + cl[10] * h2)
            h3.copy_(m)

        res = {}
        for name, fn in (("fused", fused), ("torch", torch_ops)):
            for _ in range(50):
                fn()
            w = []
            for _ in range(W):
                xc.normal_()                          # the state is rewritten in place: keep its values in range
                hist.normal_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(200):
                    fn()
                b.record()
                torch.cuda.synchronize()
                w.append(a.elapsed_time(b) / 200 * 1e3)
            res[name] = median(w)
        elems = n * 3 * 32 * 32
        rows.append({"n": n, "fused_us": round(res["fused"], 3), "torch_us": round(res["torch"], 3),
                     "fused_GB_s": round(elems * 4 * 9 / (res["fused"] * 1e-6) / 1e9, 1)})   # 6 planes read, 3 written
    return rows


def step_cost(torch, afdm, diff, model, dev, W, S):
    rows = []
    for n in NS:
        for s in SOLVERS:                                   # warm every shape and solver
            diff.sample(model, n=n, image_channels=3, noise_source="device", steps=3, sampler=s)
        t = {s: [] for s in SOLVERS}
        for _ in range(W):
            for s in SOLVERS:                               # alternating: the three share whatever else the host is doing
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                diff.sample(model, n=n, image_channels=3, noise_source="device", steps=S, sampler=s)
                torch.cuda.synchronize()
                t[s].append((time.perf_counter() - t0) / S * 1e3)
        r = {"n": n, "steps": S}
        for s in SOLVERS:
            r[s + "_ms"] = round(median(t[s]), 4)
            r[s + "_spread"] = round((max(t[s]) - min(t[s])) / median(t[s]), 4)
        rows.append(r)
    return rows


def accuracy(torch, afdm, diff, dev):
    ah = diff.alpha_hat.double()
    g = torch.Generator().manual_seed(0)
    mu = (torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 1.6 - 0.8).to(dev)

    class Gauss(torch.nn.Module):
        def forward(self, x, t):
            a = ah[t].view(-1, 1, 1, 1)
            return ((1 - a).sqrt() * (x.double() - a.sqrt() * mu) / (0.25 * a + 1 - a)).float()

    model = Gauss()
    afdm.set_seed(11)
    xT = torch.randn((1, 4, 32, 32), device=dev).double()
    a0, aT = float(ah[0]), float(ah[T - 1])
    exact = math.sqrt(a0) * mu + math.sqrt(0.25 * a0 + 1 - a0) * (xT - math.sqrt(aT) * mu) / math.sqrt(0.25 * aT + 1 - aT)
    rows = []
    for S in ACC_S:
        r = {"S": S}
        for name, kw in (("ddim", {"steps": diff.logsnr_timesteps(S)}), ("dpmpp_2m", {"steps": S, "sampler": "dpmpp_2m"}),
                         ("unipc_2", {"steps": S, "sampler": "unipc_2"}), ("unipc_3", {"steps": S, "sampler": "unipc_3"})):
            afdm.set_seed(11)
            xf = diff.sample(model, n=1, image_channels=4, noise_source="device", return_float=True, **kw)[2].double()
            r[name] = float((xf - exact).norm() / exact.norm())
        rows.append(r)
    return rows


def main():
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    from afdm import ops
    if not torch.cuda.is_available():
        sys.exit("unipc_bench: needs a GPU (nothing is measured without one)")
    W, S = arg("--windows", 15), arg("--steps", 50)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    res = {}
    res["update"] = update_cost(torch, ops, diff, dev, W)
    print("| n | unipc_step us | torch ops us | ratio | fused GB/s |\n|---|---|---|---|---|")
    for r in res["update"]:
        print(f"| {r['n']} | {r['fused_us']:.2f} | {r['torch_us']:.2f} | {r['torch_us'] / r['fused_us']:.1f} | {r['fused_GB_s']:.0f} |", flush=True)
    res["step"] = step_cost(torch, afdm, diff, model, dev, W, S)
    print("\n| n | S | UniPC-3 ms/step | UniPC-2 ms/step | DPM++(2M) ms/step | UniPC-3 / 2M | spread of a solver's rounds |\n|---|---|---|---|---|---|---|")
    for r in res["step"]:
        print(f"| {r['n']} | {r['steps']} | {r['unipc_3_ms']:.3f} | {r['unipc_2_ms']:.3f} | {r['dpmpp_2m_ms']:.3f} | "
              f"{r['unipc_3_ms'] / r['dpmpp_2m_ms']:.4f} | {100 * max(r[s + '_spread'] for s in SOLVERS):.1f} % |", flush=True)
    res["accuracy"] = accuracy(torch, afdm, diff, dev)
    print("\n| S | DDIM | DPM++(2M) | UniPC-2 | UniPC-3 |\n|---|---|---|---|---|")
    for r in res["accuracy"]:
        print(f"| {r['S']} | {r['ddim']:.2e} | {r['dpmpp_2m']:.2e} | {r['unipc_2']:.2e} | {r['unipc_3']:.2e} |", flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
