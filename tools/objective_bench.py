"""Cost of the training objectives on one MI355X (variant-3 UNet at 32 x 32).

Train step, B = 256: the default step (eps-prediction, ops.mse_loss: afd_mse_fwd / afd_mse_bwd) against prediction="v" with
loss_weighting="min_snr" on the cosine schedule (ops.objective_loss: afd_objective_loss_fwd / _bwd, the same number of launches),
eager / graph / lanes.  Sampling: one denoise step (forward + update) at n = 6 and n = 256 with the model read as eps and as v
(one afd_pred_to_eps launch more), and that conversion kernel alone.

    python tools/objective_bench.py [--out FILE.json] [--windows 30]   # the whole table, one process per configuration
    python tools/objective_bench.py --worker --mode eager|graph|lanes [--objective] [--windows W]
    python tools/objective_bench.py --sample-worker --n 6|256 [--windows W]

A train worker measures ONE configuration in its own process and prints one JSON line: step_ms, the median over W windows of 10
train steps (after 10 warm-up steps; the method of tools/step_median.py), with the fastest window and the 90th percentile as the
spread.  The sample worker alternates windows of 10 eager denoise steps of the two readings in one process (the same weights:
only the time is of interest) and times afd_pred_to_eps with events over 200 back-to-back launches.  The driver runs every
worker under `timeout -k 10` and stops at the first failure.  AFD_LIBPATH=<another build> measures that library instead."""
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
B = 256
MODES = {"eager": False, "graph": True, "lanes": "lanes"}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _model():
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    return torch, afdm, dev, afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)


def _spread(w):
    w = sorted(w)
    return round(w[len(w) // 2], 4), round(w[0], 4), round(w[int(len(w) * 0.9)], 4)


def worker():
    import gc
    mode, objective, W = arg("--mode", "eager"), "--objective" in sys.argv, arg("--windows", 30)
    torch, afdm, dev, model = _model()
    if objective:
        diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction="v")
        step = afdm.TrainStep(model, diff, lr=3e-4, graph=MODES[mode], loss_weighting="min_snr")
    else:
        step = afdm.TrainStep(model, afdm.Diffusion(noise_steps=1000, img_size=32, device=dev), lr=3e-4, graph=MODES[mode])
    images = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    for _ in range(10):
        step(images)
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    w = []
    for _ in range(W):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            loss = step(images)
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    med, lo, p90 = _spread(w)
    row = {"mode": mode, "objective": objective, "B": B, "windows": W, "step_ms": med, "step_ms_min": lo, "step_ms_p90": p90,
           "loss": float(loss)}
    if mode == "lanes":
        row["work_nodes"] = step.lanes_counts[0]
    print(json.dumps(row), flush=True)


def sample_worker():
    import gc
    n, W = arg("--n", 6), arg("--windows", 30)
    torch, afdm, dev, model = _model()
    from afdm import ops
    diffs = {k: afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction=k) for k in ("eps", "v")}
    x = torch.randn(n, 3, 32, 32, device=dev)
    noise = torch.randn_like(x)
    t = torch.full((n,), 500, device=dev, dtype=torch.long)
    model.eval()

    def steps(d, k):
        for _ in range(k):
            eps = d.predict_eps(model, x, t)
            ops.denoise_step(x, eps, noise, d.alpha, d.alpha_hat, d.beta, 500)
    w = {k: [] for k in diffs}
    with torch.no_grad():
        for d in diffs.values():
            d._hint(model)
            steps(d, 10)
        torch.cuda.synchronize()
        gc.collect()
        gc.disable()
        for _ in range(W):
            for k, d in diffs.items():                     # alternating: both readings see the same neighbours on the machine
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                steps(d, 10)
                torch.cuda.synchronize()
                w[k].append((time.perf_counter() - t0) / 10 * 1e3)
        gc.enable()
        row = {"n": n, "windows": W}
        for k in diffs:
            row[f"{k}_ms"], row[f"{k}_ms_min"], row[f"{k}_ms_p90"] = _spread(w[k])
        # the conversion alone, back to back on the same 12 * n KB
        out = torch.randn_like(x)
        reps = 200
        for _ in range(10):
            ops.pred_to_eps(out, x, t, diffs["v"].alpha_hat, "v", eps_out=out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
        ev[0].record()
        for i in range(reps):
            ops.pred_to_eps(out, x, t, diffs["v"].alpha_hat, "v", eps_out=out)
            ev[i + 1].record()
        torch.cuda.synchronize()
        us = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
        row["convert_us"], row["convert_us_min"], row["convert_us_p90"] = us[reps // 2], us[0], us[int(reps * 0.9)]
        row["convert_bytes"] = 12 * x.numel()
    print(json.dumps(row), flush=True)


def _run(cmd, limit):
    """One GPU step under its own time limit; None after any failure (the caller then starts nothing more)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        print(f"FAILED rc={p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
        return None
    return p


def driver():
    W = arg("--windows", 30)
    rows, samples = [], []
    for mode in MODES:
        for objective in (False, True):
            cmd = [sys.executable, "tools/objective_bench.py", "--worker", "--mode", mode, "--windows", str(W)]
            p = _run(cmd + (["--objective"] if objective else []), 300)
            if p is None:
                return 1
            rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
    for n in (6, 256):
        p = _run([sys.executable, "tools/objective_bench.py", "--sample-worker", "--n", str(n), "--windows", str(W)], 300)
        if p is None:
            return 1
        samples.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(samples[-1]), flush=True)
    by = {(r["mode"], r["objective"]): r for r in rows}
    print("\n| mode | ms/step default (min .. p90) | v + min_snr (min .. p90) | difference |")
    print("|---|---|---|---|")
    for mode in MODES:
        a, b = by[(mode, False)], by[(mode, True)]
        d = b["step_ms"] - a["step_ms"]
        print(f"| {mode} | {a['step_ms']:.3f} ({a['step_ms_min']:.3f} .. {a['step_ms_p90']:.3f}) | "
              f"{b['step_ms']:.3f} ({b['step_ms_min']:.3f} .. {b['step_ms_p90']:.3f}) | {1e3 * d:+.0f} us ({100 * d / a['step_ms']:+.2f} %) |")
    print("\n| n | ms/denoise step eps (min .. p90) | v (min .. p90) | difference | afd_pred_to_eps alone (min .. p90) |")
    print("|---|---|---|---|---|")
    for s in samples:
        d = s["v_ms"] - s["eps_ms"]
        print(f"| {s['n']} | {s['eps_ms']:.3f} ({s['eps_ms_min']:.3f} .. {s['eps_ms_p90']:.3f}) | "
              f"{s['v_ms']:.3f} ({s['v_ms_min']:.3f} .. {s['v_ms_p90']:.3f}) | {1e3 * d:+.1f} us ({100 * d / s['eps_ms']:+.2f} %) | "
              f"{s['convert_us']:.1f} us ({s['convert_us_min']:.1f} .. {s['convert_us_p90']:.1f}) |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"train": rows, "sample": samples}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    elif "--sample-worker" in sys.argv:
        sample_worker()
    else:
        sys.exit(driver())
