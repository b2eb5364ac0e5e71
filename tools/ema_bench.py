"""Cost of the EMA of the weights fused into AdamW: a B = 256 variant-3 TrainStep at 32 x 32 on one MI355X, with and without
TrainStep(ema=...), eager and "lanes".

    python tools/ema_bench.py [--out FILE.json] [--prof-dir DIR] [--windows 30]   # the whole table, one process per configuration
    python tools/ema_bench.py --worker --mode eager|lanes [--ema] [--windows W]
    python tools/ema_bench.py --profile-run                            # the process that the driver runs under rocprofv3

A worker measures ONE configuration in its own process and prints one JSON line: step_ms, the median over W windows of 10
train steps (after 10 warm-up steps; timesteps from the CPU generator, noise from the device), and the parameter counts.
The driver runs every worker under `timeout -k 10`, stops at the first failure, then runs --profile-run once under
`rocprofv3 --kernel-trace --stats` (a process of its own): eager steps without and with the EMA, so that both instances of
adamw_k<VEC, EMA, CTL> are timed in the same process.  Bytes moved per parameter: 28 for AdamW (p, m, v read and written, g read),
36 for the fused form (and the EMA read and written)."""
import copy
import csv
import glob
import json
import math
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
B = 256


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _setup(mode, use_ema):
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    kw = {"ema": afdm.EMA(0.995), "ema_model": copy.deepcopy(model), "ema_start": 5} if use_ema else {}
    step = afdm.TrainStep(model, diff, lr=3e-4, graph={"eager": False, "lanes": "lanes"}[mode], **kw)
    images = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
    return torch, step, images


def worker():
    import gc
    mode, use_ema, W = arg("--mode", "eager"), "--ema" in sys.argv, arg("--windows", 30)
    torch, step, images = _setup(mode, use_ema)
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
    fp = step.opt.fp
    print(json.dumps({"mode": mode, "ema": use_ema, "B": B, "windows": W, "step_ms": round(w[len(w) // 2], 4),
                      "step_ms_min": round(w[0], 4), "step_ms_p90": round(w[int(len(w) * 0.9)], 4),
                      "n_active": fp.n_active, "numel": fp.numel}), flush=True)


def profile_run():
    for use_ema in (False, True):
        torch, step, images = _setup("eager", use_ema)
        for _ in range(20):
            step(images)
        torch.cuda.synchronize()
        print(json.dumps({"n_active": step.opt.fp.n_active, "numel": step.opt.fp.numel}), flush=True)


def _run(cmd, limit):
    """One GPU step under its own time limit; None after any failure (the caller then starts nothing more)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        print(f"FAILED rc={p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
        return None
    return p


def _kernel_stats(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return []
    with open(files[0]) as fh:
        return list(csv.DictReader(fh))


def driver():
    W = arg("--windows", 30)
    rows = []
    for mode in ("eager", "lanes"):
        for use_ema in (False, True):
            cmd = [sys.executable, "tools/ema_bench.py", "--worker", "--mode", mode, "--windows", str(W)]
            p = _run(cmd + (["--ema"] if use_ema else []), 600)
            if p is None:
                return 1
            r = json.loads(p.stdout.strip().splitlines()[-1])
            rows.append(r)
            print(json.dumps(r), flush=True)
    by = {(r["mode"], r["ema"]): r for r in rows}
    print("\n| mode | ms/step without EMA | with EMA | difference |")
    print("|---|---|---|---|")
    for mode in ("eager", "lanes"):
        a, b = by[(mode, False)]["step_ms"], by[(mode, True)]["step_ms"]
        print(f"| {mode} | {a:.3f} | {b:.3f} | {1e3 * (b - a):+.0f} us ({100 * (b - a) / a:+.2f} %) |")

    pdir = arg("--prof-dir", "") or tempfile.mkdtemp(prefix="ema_prof_")      # the raw rocprofv3 output stays there
    p = _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "ema", "--",
              sys.executable, "tools/ema_bench.py", "--profile-run"], 900)
    if p is None:
        return 1
    counts = json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])
    n_act, n_all = counts["n_active"], counts["numel"]
    prof = {}
    print(f"\nparameters: {n_all} ({n_act} optimised)")
    print("| kernel | calls | mean us | bytes / param | GB/s |")
    print("|---|---|---|---|---|")
    for s in _kernel_stats(pdir):
        name = s.get("Name", s.get("KernelName", ""))
        m = re.search(r"adamw_k<[^,>]+,\s*([^,>]+),", name)         # adamw_k<VEC, EMA, CTL>
        if m is None:
            continue
        nbytes = 28 * n_act + (8 * n_all if m.group(1).strip() in ("true", "(bool)1", "1") else 0)
        mean_ns = float(s["AverageNs"])
        prof[name] = {"calls": int(s["Calls"]), "mean_us": mean_ns / 1e3, "GB_s": nbytes / mean_ns}
        print(f"| {name[:48]} | {s['Calls']} | {mean_ns / 1e3:.2f} | {nbytes / n_act:.1f} | {nbytes / mean_ns:.0f} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows, "kernels": prof, "n_active": n_act, "numel": n_all}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    elif "--profile-run" in sys.argv:
        profile_run()
    else:
        sys.exit(driver())
