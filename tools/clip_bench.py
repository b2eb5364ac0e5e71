"""Cost of gradient-norm clipping + the learning-rate schedule on the device: a B = 256 variant-3 TrainStep at 32 x 32 on one
MI355X with the feature off (the default step: afd_adamw_tick + afd_adamw_step) and on (afd_grad_sqnorm_partials +
afd_adamw_ctl_tick + afd_adamw_ctl_step), eager / graph / lanes, and the norm kernel alone.

    python tools/clip_bench.py [--out FILE.json] [--windows 30]        # the whole table, one process per configuration
    python tools/clip_bench.py --worker --mode eager|graph|lanes [--clip] [--windows W]
    python tools/clip_bench.py --norm-worker                           # the norm kernel alone over the model's gradient buffer

A worker measures ONE configuration in its own process and prints one JSON line: step_ms, the median over W windows of 10
train steps (after 10 warm-up steps; the method of tools/step_median.py), with the fastest window and the 90th percentile as the
spread.  "on" is max_grad_norm = 1.0 with a cosine schedule (warm-up 100, total 10000): all three launches of the new path.
The norm worker times afd_grad_sqnorm_partials with events over 200 launches in two settings: back to back on the same buffer
(23.6 MB: it stays in the Infinity Cache) and each launch behind a 512 MB fill that evicts it (HBM).  The driver runs every
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


def _setup(mode, clip):
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    kw = {"max_grad_norm": 1.0, "lr_schedule": afdm.LRSchedule("cosine", warmup=100, total=10000, min_ratio=0.1)} if clip else {}
    step = afdm.TrainStep(model, diff, lr=3e-4, graph=MODES[mode], **kw)
    images = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    return torch, afdm, step, images


def worker():
    import gc
    mode, clip, W = arg("--mode", "eager"), "--clip" in sys.argv, arg("--windows", 30)
    torch, afdm, step, images = _setup(mode, clip)
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
            step(images)
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    w.sort()
    row = {"mode": mode, "clip": clip, "B": B, "windows": W, "step_ms": round(w[len(w) // 2], 4), "step_ms_min": round(w[0], 4),
           "step_ms_p90": round(w[int(len(w) * 0.9)], 4), "n_active": step.opt.fp.n_active}
    if clip:
        row.update(last_grad_norm=step.last_grad_norm, last_lr=step.last_lr, n_skipped=step.n_skipped)
    print(json.dumps(row), flush=True)


def norm_worker():
    torch, afdm, step, images = _setup("eager", True)
    from afdm import ops
    for _ in range(3):
        step(images)
    fp, L, s = step.opt.fp, afdm.lib(), ops._stream()
    parts = step.opt.partials
    n, nbytes = fp.n_active, 4 * fp.n_active
    reps = 200

    def launch():
        L.afd_grad_sqnorm_partials(fp.grad.data_ptr(), n, 1.0, parts.data_ptr(), parts.numel(), s)
    for _ in range(10):
        launch()
    torch.cuda.synchronize()
    out = {"n": n, "bytes": nbytes, "n_partials": parts.numel()}
    # back to back on the same buffer
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        launch()
        ev[i + 1].record()
    torch.cuda.synchronize()
    t = sorted(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(reps))
    out["warm_us"], out["warm_us_min"], out["warm_us_p90"] = t[reps // 2], t[0], t[int(reps * 0.9)]
    out["warm_GB_s"] = nbytes / t[reps // 2] / 1e3
    # behind a fill larger than the Infinity Cache
    big = torch.empty(128 * 1024 * 1024, device=fp.grad.device)
    a, b = ([torch.cuda.Event(enable_timing=True) for _ in range(40)] for _ in range(2))
    for i in range(40):
        big.fill_(float(i))
        a[i].record()
        launch()
        b[i].record()
    torch.cuda.synchronize()
    t = sorted(x.elapsed_time(y) * 1e3 for x, y in zip(a, b))
    out["cold_us"], out["cold_us_min"], out["cold_us_p90"] = t[20], t[0], t[36]
    out["cold_GB_s"] = nbytes / t[20] / 1e3
    print(json.dumps(out), flush=True)


def _run(cmd, limit):
    """One GPU step under its own time limit; None after any failure (the caller then starts nothing more)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        print(f"FAILED rc={p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
        return None
    return p


def driver():
    W = arg("--windows", 30)
    rows = []
    for mode in MODES:
        for clip in (False, True):
            cmd = [sys.executable, "tools/clip_bench.py", "--worker", "--mode", mode, "--windows", str(W)]
            p = _run(cmd + (["--clip"] if clip else []), 300)
            if p is None:
                return 1
            r = json.loads(p.stdout.strip().splitlines()[-1])
            rows.append(r)
            print(json.dumps(r), flush=True)
    by = {(r["mode"], r["clip"]): r for r in rows}
    print("\n| mode | ms/step off (min .. p90) | on (min .. p90) | difference |")
    print("|---|---|---|---|")
    for mode in MODES:
        a, b = by[(mode, False)], by[(mode, True)]
        d = b["step_ms"] - a["step_ms"]
        print(f"| {mode} | {a['step_ms']:.3f} ({a['step_ms_min']:.3f} .. {a['step_ms_p90']:.3f}) | "
              f"{b['step_ms']:.3f} ({b['step_ms_min']:.3f} .. {b['step_ms_p90']:.3f}) | {1e3 * d:+.0f} us ({100 * d / a['step_ms']:+.2f} %) |")
    p = _run([sys.executable, "tools/clip_bench.py", "--norm-worker"], 300)
    if p is None:
        return 1
    k = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(k), flush=True)
    print(f"\nnorm kernel over {k['n']} floats ({k['bytes'] / 1e6:.1f} MB): back to back {k['warm_us']:.1f} us = {k['warm_GB_s']:.0f} GB/s; "
          f"behind a 512 MB fill {k['cold_us']:.1f} us = {k['cold_GB_s']:.0f} GB/s")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows, "norm_kernel": k}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    elif "--norm-worker" in sys.argv:
        norm_worker()
    else:
        sys.exit(driver())
