"""DDIM sampling cost, variant 3 at 32 x 32, T = 1000, one MI355X.

    python tools/ddim_bench.py [--out FILE.json] [--prof-dir DIR] [--windows 30]   # the whole table, one process per configuration
    python tools/ddim_bench.py --worker --n N --steps S|ddpm [--graph] [--eta E] [--windows W]
    python tools/ddim_bench.py --profile-run                            # the process that the driver runs under rocprofv3

A worker measures ONE configuration in its own process and prints one JSON line:
  step_ms     median over W windows of 20 denoise steps (the UNet forward + the update, and the noise draw when the sampler
              draws one), eager (host launches, as `Diffusion.sample` runs a step) or replaying one captured step (--graph);
  traj_s      wall time of whole `Diffusion.sample` trajectories (x_T included, the graph capture included under --graph):
              the median of 3 after a short warm-up trajectory (1 for the 999-step chains), and images_s = n / traj_s.
--steps ddpm is the DDPM chain (`steps=None`): its step is `afd_denoise_step`, its trajectory 999 forwards.
The driver runs every worker under `timeout -k 10`, stops at the first failure, then runs --profile-run once under
`rocprofv3 --kernel-trace --stats` (a process of its own) and reports the update kernels' own time and achieved bandwidth."""
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
T = 1000
NS = (6, 64, 256)
SS = (50, 100, 250, T - 1)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _setup(n):
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    return torch, afdm, dev, model, diff


def worker():
    import gc
    n, steps, W, eta = arg("--n", 6), arg("--steps", "50"), arg("--windows", 30), arg("--eta", 0.0)
    use_graph = "--graph" in sys.argv
    ddim = steps != "ddpm"
    torch, afdm, dev, model, diff = _setup(n)
    from afdm import ops
    S = int(steps) if ddim else None
    taus = diff.ddim_timesteps(S) if ddim else None
    t, tp = (taus[len(taus) // 2], taus[len(taus) // 2 + 1]) if ddim and S > 2 else (500, 499)
    xs = torch.randn(n, 3, 32, 32, device=dev)
    t_dev = torch.full((n,), t, device=dev, dtype=torch.long)
    tp_dev = torch.full((1,), tp, device=dev, dtype=torch.long)

    def one_step():
        if use_graph:
            eps = model(xs, t_dev)
            if ddim:
                ops.ddim_step_dev(xs, eps, torch.randn_like(xs) if eta > 0 else None, diff.alpha_hat, t_dev, tp_dev, eta, xs)
            else:
                ops.denoise_step_dev(xs, eps, torch.randn_like(xs), diff.alpha, diff.alpha_hat, diff.beta, t_dev, xs)
        else:
            eps = model(xs, diff._t_full(n, t, dev))
            if ddim:
                xs.copy_(ops.ddim_step(xs, eps, torch.randn_like(xs) if eta > 0 else None, diff.alpha_hat, t, tp, eta))
            else:
                xs.copy_(ops.denoise_step(xs, eps, torch.randn_like(xs), diff.alpha, diff.alpha_hat, diff.beta, t))

    diff._hint(model)                # as inside Diffusion.sample
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
            xs.normal_()             # keep the values in range (the step indices do not move)
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
        gc.enable()
    model.train()
    diff._unhint(model)
    kw = {"steps": S, "eta": eta} if ddim else {}
    if ddim:                         # a short warm-up trajectory (the DDPM chain has no short form; its steps warmed up above)
        diff.sample(model, n=n, image_channels=3, noise_source="device", graph=use_graph, steps=3, eta=eta)
    reps = 1 if (not ddim or S >= T - 1) else 3
    traj = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        diff.sample(model, n=n, image_channels=3, noise_source="device", graph=use_graph, **kw)
        torch.cuda.synchronize()
        traj.append(time.perf_counter() - t0)
    w.sort()
    traj.sort()
    ts = traj[len(traj) // 2]
    print(json.dumps({"n": n, "steps": steps, "graph": use_graph, "eta": eta, "windows": W, "step_ms": round(w[len(w) // 2], 4),
                      "step_ms_min": round(w[0], 4), "step_ms_p90": round(w[int(len(w) * 0.9)], 4), "traj_s": round(ts, 4),
                      "traj_reps": reps, "images_s": round(n / ts, 2)}), flush=True)


def profile_run():
    """Trajectories whose update kernels the driver's rocprofv3 pass times: n = 256, S = 50, eta = 1 (so the update reads the
    noise: 16 B / element), unguided and guided (which also writes the other half of the 2n input: 24 B / element)."""
    torch, afdm, dev, model, diff = _setup(256)
    diff.sample(model, n=256, image_channels=3, noise_source="device", steps=50, eta=1.0)
    afdm.set_seed(42)
    cm = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, num_classes=10).to(dev)
    diff.sample(cm, n=256, image_channels=3, noise_source="device", steps=50, eta=1.0, labels=torch.arange(256, device=dev) % 10,
                cfg_scale=3.0)
    torch.cuda.synchronize()


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
    for graph in (False, True):
        for n in NS:
            for steps in ("ddpm",) + tuple(str(s) for s in SS):
                cmd = [sys.executable, "tools/ddim_bench.py", "--worker", "--n", str(n), "--steps", steps, "--windows", str(W)]
                p = _run(cmd + (["--graph"] if graph else []), 600)
                if p is None:
                    return 1
                r = json.loads(p.stdout.strip().splitlines()[-1])
                rows.append(r)
                print(json.dumps(r), flush=True)
    ddpm = {(r["n"], r["graph"]): r for r in rows if r["steps"] == "ddpm"}
    print("\n| n | mode | S | ms/step | DDPM ms/step | images/s | DDPM images/s | speed-up |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        if r["steps"] == "ddpm":
            continue
        d = ddpm[(r["n"], r["graph"])]
        print(f"| {r['n']} | {'graph' if r['graph'] else 'eager'} | {r['steps']} | {r['step_ms']:.3f} | {d['step_ms']:.3f} | "
              f"{r['images_s']:.1f} | {d['images_s']:.2f} | {r['images_s'] / d['images_s']:.1f}x |")

    prof = {}
    pdir = arg("--prof-dir", "") or tempfile.mkdtemp(prefix="ddim_prof_")      # the raw rocprofv3 output stays there
    p = _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "ddim", "--",
              sys.executable, "tools/ddim_bench.py", "--profile-run"], 900)
    if p is None:
        return 1
    stats = _kernel_stats(pdir)
    total = sum(float(s.get("TotalDurationNs", 0)) for s in stats)
    elems = 256 * 3 * 32 * 32
    print("\n| kernel | calls | mean us | GB/s | share of all kernel time |")
    print("|---|---|---|---|---|")
    for s in stats:
        name = s.get("Name", s.get("KernelName", ""))
        if "ddim_step" not in name:
            continue
        guided = "ILb1E" in name or "<true>" in name
        nbytes = elems * (24 if guided else 16)          # x, eps (2 halves when guided), noise read; x_out (and x_out2) written
        mean_ns = float(s["AverageNs"])
        prof[name] = {"calls": int(s["Calls"]), "mean_us": mean_ns / 1e3, "GB_s": nbytes / mean_ns,
                      "share": float(s["TotalDurationNs"]) / total}
        print(f"| {'guided' if guided else 'unguided'} {name[:40]} | {s['Calls']} | {mean_ns / 1e3:.2f} | {nbytes / mean_ns:.0f} | "
              f"{100 * float(s['TotalDurationNs']) / total:.2f} % |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows, "update_kernels": prof}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    elif "--profile-run" in sys.argv:
        profile_run()
    else:
        sys.exit(driver())
