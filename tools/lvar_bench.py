"""Cost of the learned reverse-process variances on one MI355X (variant-3 UNet at 32 x 32).

Train step, B = 256: the default step (UNet(c_out=3), ops.mse_loss) against the learned-variance step (UNet(c_out=6),
Diffusion(variance="learned"), ops.lvar_loss: the same number of launches), eager / graph / lanes.  Sampling: one DDPM denoise step
(forward + update) at n = 6 and n = 256, fixed (afd_denoise_step) against learned (afd_denoise_step_lvar on the 2C output).

    python tools/lvar_bench.py [--out FILE.json] [--windows 30] [--parent-root DIR]
    python tools/lvar_bench.py --worker --mode eager|graph|lanes [--learned] [--windows W] [--root DIR]
    python tools/lvar_bench.py --sample-worker --n 6|256 [--learned] [--windows W] [--root DIR]

Every worker measures ONE configuration in its own process and prints one JSON line: the median over W windows of 10 steps after
10 warm-up steps (the method of tools/step_median.py), with the fastest window and the 90th percentile as the spread.  The default
(fixed-variance) rows are the yardstick: with --parent-root DIR they import the package from DIR, a built checkout of the parent
commit (`git worktree add DIR HEAD~1`, then its build()), so the comparison is never against the code under test alone.  The
driver runs every worker under `timeout -k 10` and stops at the first failure."""
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


def _setup(learned):
    sys.path.insert(0, arg("--root", ROOT))
    import torch
    import afdm
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=6 if learned else 3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **({"variance": "learned"} if learned else {}))
    return torch, afdm, dev, model, diff


def _spread(w):
    w = sorted(w)
    return round(w[len(w) // 2], 4), round(w[0], 4), round(w[int(len(w) * 0.9)], 4)


def _windows(torch, W, body):
    import gc
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    w = []
    for _ in range(W):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            body()
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    return _spread(w)


def worker():
    mode, learned, W = arg("--mode", "eager"), "--learned" in sys.argv, arg("--windows", 30)
    torch, afdm, dev, model, diff = _setup(learned)
    step = afdm.TrainStep(model, diff, lr=3e-4, graph=MODES[mode])
    images = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    for _ in range(10):
        loss = step(images)
    med, lo, p90 = _windows(torch, W, lambda: step(images))
    row = {"mode": mode, "learned": learned, "B": B, "windows": W, "step_ms": med, "step_ms_min": lo, "step_ms_p90": p90,
           "loss": float(loss), "root": arg("--root", ROOT)}
    if mode == "lanes":
        row["work_nodes"] = step.lanes_counts[0]
    print(json.dumps(row), flush=True)


def sample_worker():
    n, learned, W = arg("--n", 6), "--learned" in sys.argv, arg("--windows", 30)
    torch, afdm, dev, model, diff = _setup(learned)
    from afdm import ops
    x = torch.randn(n, 3, 32, 32, device=dev)
    noise = torch.randn_like(x)
    t = torch.full((n,), 500, device=dev, dtype=torch.long)
    model.eval()
    diff._hint(model)

    def body():
        out = model(x, t)
        if learned:
            ops.denoise_step_lvar(x, out, noise, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), "eps", 500)
        else:
            ops.denoise_step(x, out, noise, diff.alpha, diff.alpha_hat, diff.beta, 500)
    with torch.no_grad():
        for _ in range(10):
            body()
        med, lo, p90 = _windows(torch, W, body)
    print(json.dumps({"n": n, "learned": learned, "windows": W, "step_ms": med, "step_ms_min": lo, "step_ms_p90": p90,
                      "root": arg("--root", ROOT)}), flush=True)


def _run(cmd, limit, env):
    """One GPU step under its own time limit; None after any failure (the caller then starts nothing more)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True, env=env)
    if p.returncode != 0:
        print(f"FAILED rc={p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
        return None
    return p


def driver():
    W = arg("--windows", 30)
    parent = ["--root", os.path.abspath(arg("--parent-root", ""))] if "--parent-root" in sys.argv else []
    rows, samples = [], []
    jobs = [(["--worker", "--mode", mode], learned) for mode in MODES for learned in (False, True)]
    jobs += [(["--sample-worker", "--n", str(n)], learned) for n in (6, 256) for learned in (False, True)]
    for extra, learned in jobs:
        cmd = [sys.executable, "tools/lvar_bench.py"] + extra + ["--windows", str(W)] + (["--learned"] if learned else parent)
        p = _run(cmd, 300, dict(os.environ))
        if p is None:
            return 1
        row = json.loads(p.stdout.strip().splitlines()[-1])
        (rows if "mode" in row else samples).append(row)
        print(json.dumps(row), flush=True)
    print("\n| | default, ms (min .. p90) | learned variance, ms (min .. p90) | difference |")
    print("|---|---|---|---|")
    pairs = [(f"train step, {m}", [r for r in rows if r["mode"] == m]) for m in MODES]
    pairs += [(f"denoise step, n = {n}", [s for s in samples if s["n"] == n]) for n in (6, 256)]
    for name, pr in pairs:
        a, b = (next(r for r in pr if r["learned"] == flag) for flag in (False, True))
        d = b["step_ms"] - a["step_ms"]
        print(f"| {name} | {a['step_ms']:.3f} ({a['step_ms_min']:.3f} .. {a['step_ms_p90']:.3f}) | "
              f"{b['step_ms']:.3f} ({b['step_ms_min']:.3f} .. {b['step_ms_p90']:.3f}) | {1e3 * d:+.0f} us ({100 * d / a['step_ms']:+.2f} %) |")
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
