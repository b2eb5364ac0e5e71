"""Analytic-DPM: the cost of the step with a tabulated sigma, of the per-row squared norms and of an analytic sampling step,
variant 3 at 32 x 32, T = 1000, one MI355X.

    python tools/analytic_bench.py [--out FILE.json] [--windows 15] [--steps 50]

One process, three parts, each printed as a table and, with --out, written as JSON:
  update    microseconds per `ops.ddim_step_var` at n = 6 and n = 256 images of 3 x 32 x 32, against `ops.ddim_step` (the same
            loads and stores plus one table read) and against the same expression in torch ops; device events around 200
            calls, the median of --windows windows.
  sqnorm    microseconds per `ops.eps_sqnorm_rows` at the same sizes, against eps.double().square().sum((1, 2, 3)).
  step      milliseconds per sampling step of `Diffusion.sample_analytic(steps=, eta=1)` against `Diffusion.sample(steps=, eta=1)`, run alternately: a
            host clock around whole trajectories of --steps steps that end in a device synchronise, the median of --windows
            rounds, over the number of steps.
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


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def windows(torch, fn, W, calls=200):
    """Median over W windows of the microseconds per call of fn, device events around `calls` calls."""
    for _ in range(50):
        fn()
    w = []
    for _ in range(W):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        w.append(a.elapsed_time(b) / calls * 1e3)
    return median(w)


def update_cost(torch, ops, diff, dev, W):
    ah = diff.alpha_hat
    t, tp, eta = 640, 420, 1.0
    a_t, a_p = float(ah[t]), float(ah[tp])
    var = eta * eta * (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
    sq1m, sqat, sqap, sigma, dirc = math.sqrt(1 - a_t), math.sqrt(a_t), math.sqrt(a_p), math.sqrt(var), math.sqrt(1 - a_p - var)
    sig = torch.full((T,), sigma, device=dev)
    rows = []
    for n in NS:
        x, e, z = (torch.randn(n, 3, 32, 32, device=dev) for _ in range(3))
        out = torch.empty_like(x)
        res = {
            "var": windows(torch, lambda: ops.ddim_step_var(x, e, z, ah, sig, t, tp, eta, out), W),
            "ddim": windows(torch, lambda: ops.ddim_step(x, e, z, ah, t, tp, eta, out), W),
            "torch": windows(torch, lambda: out.copy_(sqap * ((x - sq1m * e) / sqat) + dirc * e + sigma * z), W),
        }
        elems = n * 3 * 32 * 32
        rows.append({"n": n, "var_us": round(res["var"], 3), "ddim_us": round(res["ddim"], 3), "torch_us": round(res["torch"], 3),
                     "var_GB_s": round(elems * 4 * 4 / (res["var"] * 1e-6) / 1e9, 1)})       # 3 planes read, 1 written
    return rows


def sqnorm_cost(torch, ops, dev, W):
    rows = []
    for n in NS:
        e = torch.randn(n, 3, 32, 32, device=dev)
        out = torch.empty(n, device=dev, dtype=torch.float64)
        res = {"fused": windows(torch, lambda: ops.eps_sqnorm_rows(e, out=out), W),
               "torch": windows(torch, lambda: e.double().square().sum((1, 2, 3)), W)}
        rows.append({"n": n, "fused_us": round(res["fused"], 3), "torch_us": round(res["torch"], 3)})
    return rows


def step_cost(torch, afdm, diff, model, dev, W, S):
    import numpy as np
    av = afdm.AnalyticVariance.for_diffusion(diff, np.full(T, 0.5))
    kinds = {"analytic": lambda **kw: diff.sample_analytic(model, analytic=av, **kw), "ddim": lambda **kw: diff.sample(model, **kw)}
    rows = []
    for n in NS:
        for run in kinds.values():                          # warm every shape and kind
            run(n=n, image_channels=3, noise_source="device", steps=3, eta=1.0)
        t = {k: [] for k in kinds}
        for _ in range(W):
            for k, run in kinds.items():                    # alternating: the two share whatever else the host is doing
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(n=n, image_channels=3, noise_source="device", steps=S, eta=1.0)
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / S * 1e3)
        r = {"n": n, "steps": S}
        for k in kinds:
            r[k + "_ms"] = round(median(t[k]), 4)
            r[k + "_spread"] = round((max(t[k]) - min(t[k])) / median(t[k]), 4)
        rows.append(r)
    return rows


def main():
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    from afdm import ops
    if not torch.cuda.is_available():
        sys.exit("analytic_bench: needs a GPU (nothing is measured without one)")
    W, S = arg("--windows", 15), arg("--steps", 50)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    res = {}
    res["update"] = update_cost(torch, ops, diff, dev, W)
    print("| n | ddim_step_var us | ddim_step us | torch ops us | var / ddim | var GB/s |\n|---|---|---|---|---|---|")
    for r in res["update"]:
        print(f"| {r['n']} | {r['var_us']:.2f} | {r['ddim_us']:.2f} | {r['torch_us']:.2f} | {r['var_us'] / r['ddim_us']:.3f} | "
              f"{r['var_GB_s']:.0f} |", flush=True)
    res["sqnorm"] = sqnorm_cost(torch, ops, dev, W)
    print("\n| n | eps_sqnorm_rows us | torch fp64 us | ratio |\n|---|---|---|---|")
    for r in res["sqnorm"]:
        print(f"| {r['n']} | {r['fused_us']:.2f} | {r['torch_us']:.2f} | {r['torch_us'] / r['fused_us']:.1f} |", flush=True)
    res["step"] = step_cost(torch, afdm, diff, model, dev, W, S)
    print("\n| n | S | analytic ms/step | DDIM eta=1 ms/step | ratio | spread of a kind's rounds |\n|---|---|---|---|---|---|")
    for r in res["step"]:
        print(f"| {r['n']} | {r['steps']} | {r['analytic_ms']:.3f} | {r['ddim_ms']:.3f} | {r['analytic_ms'] / r['ddim_ms']:.4f} | "
              f"{100 * max(r['analytic_spread'], r['ddim_spread']):.1f} % |", flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
