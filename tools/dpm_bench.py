"""DPM-Solver++(2M) sampling cost against DDIM, variant 3 at 32 x 32, T = 1000, one MI355X.

    python tools/dpm_bench.py [--out FILE.json] [--prof-dir DIR] [--windows 15]   # the whole table, one process per configuration
    python tools/dpm_bench.py --worker --n N --steps S --solver dpmpp_2m|ddim [--graph] [--windows W]
    python tools/dpm_bench.py --profile-run                             # the process that the driver runs under rocprofv3

A worker measures ONE configuration in its own process and prints one JSON line:
  step_ms     median over W windows of 20 sampling steps (the UNet forward + the update), at a second-order step of the
              S-step chain for DPM++ (`afd_dpmpp_step` reading x0_prev) and the same t -> t_prev for DDIM (eta = 0), eager
              (host launches, as `Diffusion.sample` runs a step) or replaying one captured step (--graph);
  traj_s      wall time of whole `Diffusion.sample` trajectories (x_T included, the graph capture included under --graph):
              the median of 3 after a short warm-up trajectory, and images_s = n / traj_s.
Both solvers run on `logsnr_timesteps(S)`: DPM++ through sampler="dpmpp_2m", DDIM through the same explicit timestep list.
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
NS = (6, 256)
SS = (10, 20, 50)
SOLVERS = ("dpmpp_2m", "ddim")


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _setup():
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
    n, S, W, solver = arg("--n", 6), arg("--steps", 20), arg("--windows", 15), arg("--solver", "dpmpp_2m")
    use_graph = "--graph" in sys.argv
    dpm = solver == "dpmpp_2m"
    torch, afdm, dev, model, diff = _setup()
    from afdm import ops
    pairs = diff.dpmpp_pairs(S)
    k = len(pairs) // 2                                   # a second-order step of the chain (S >= 3)
    t, tp = pairs[k]
    coef = diff.dpmpp_coefficients(pairs).to(dev)[k].clone()
    xs = torch.randn(n, 3, 32, 32, device=dev)
    x0 = torch.randn_like(xs)
    t_dev = torch.full((n,), t, device=dev, dtype=torch.long)
    tp_dev = torch.full((1,), tp, device=dev, dtype=torch.long)

    def one_step():
        eps = model(xs, t_dev if use_graph else diff._t_full(n, t, dev))
        if dpm:
            ops.dpmpp_step(xs, eps, x0, coef, xs, x0)
        elif use_graph:
            ops.ddim_step_dev(xs, eps, None, diff.alpha_hat, t_dev, tp_dev, 0.0, xs)
        else:
            xs.copy_(ops.ddim_step(xs, eps, None, diff.alpha_hat, t, tp, 0.0))

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
            x0.normal_()
            run()
        gc.collect()
        gc.disable()
        w = []
        for _ in range(W):
            xs.normal_()
            x0.normal_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                run()
            torch.cuda.synchronize()
            w.append((time.perf_counter() - t0) / 20 * 1e3)
        gc.enable()
    model.train()
    diff._unhint(model)
    kw = {"steps": S, "sampler": solver} if dpm else {"steps": diff.logsnr_timesteps(S)}
    warm = {"steps": 3, "sampler": solver} if dpm else {"steps": 3}
    diff.sample(model, n=n, image_channels=3, noise_source="device", graph=use_graph, **warm)
    traj = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        diff.sample(model, n=n, image_channels=3, noise_source="device", graph=use_graph, **kw)
        torch.cuda.synchronize()
        traj.append(time.perf_counter() - t0)
    w.sort()
    traj.sort()
    ts = traj[1]
    print(json.dumps({"solver": solver, "n": n, "steps": S, "graph": use_graph, "windows": W, "step_ms": round(w[len(w) // 2], 4),
                      "step_ms_min": round(w[0], 4), "step_ms_p90": round(w[int(len(w) * 0.9)], 4), "traj_s": round(ts, 4),
                      "images_s": round(n / ts, 2)}), flush=True)


def profile_run():
    """Trajectories whose update kernels the driver's rocprofv3 pass times: n = 256, S = 50, unguided and guided (s = 3).
    Unguided: x, eps and x0_prev read, x_out and x0_out written (20 B / element).  Guided: both halves of eps2 read and x_out2
    written as well (28 B / element)."""
    torch, afdm, dev, model, diff = _setup()
    diff.sample(model, n=256, image_channels=3, noise_source="device", steps=50, sampler="dpmpp_2m")
    afdm.set_seed(42)
    cm = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, num_classes=10).to(dev)
    diff.sample(cm, n=256, image_channels=3, noise_source="device", steps=50, sampler="dpmpp_2m",
                labels=torch.arange(256, device=dev) % 10, cfg_scale=3.0)
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
    W = arg("--windows", 15)
    rows = []
    for graph in (False, True):
        for n in NS:
            for S in SS:
                for solver in SOLVERS:
                    cmd = [sys.executable, "tools/dpm_bench.py", "--worker", "--n", str(n), "--steps", str(S), "--solver", solver,
                           "--windows", str(W)]
                    p = _run(cmd + (["--graph"] if graph else []), 600)
                    if p is None:
                        return 1
                    r = json.loads(p.stdout.strip().splitlines()[-1])
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    ddim = {(r["n"], r["graph"], r["steps"]): r for r in rows if r["solver"] == "ddim"}
    print("\n| n | mode | S | DPM++ ms/step | DDIM ms/step | step ratio | DPM++ images/s | DDIM images/s |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        if r["solver"] == "ddim":
            continue
        d = ddim[(r["n"], r["graph"], r["steps"])]
        print(f"| {r['n']} | {'graph' if r['graph'] else 'eager'} | {r['steps']} | {r['step_ms']:.3f} | {d['step_ms']:.3f} | "
              f"{r['step_ms'] / d['step_ms']:.3f} | {r['images_s']:.1f} | {d['images_s']:.1f} |")

    prof = {}
    pdir = arg("--prof-dir", "") or tempfile.mkdtemp(prefix="dpm_prof_")      # the raw rocprofv3 output stays there
    p = _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "dpm", "--",
              sys.executable, "tools/dpm_bench.py", "--profile-run"], 900)
    if p is None:
        return 1
    stats = _kernel_stats(pdir)
    total = sum(float(s.get("TotalDurationNs", 0)) for s in stats)
    elems = 256 * 3 * 32 * 32
    print("\n| kernel | calls | mean us | GB/s | share of all kernel time |")
    print("|---|---|---|---|---|")
    for s in stats:
        name = s.get("Name", s.get("KernelName", ""))
        if "dpmpp_step" not in name:
            continue
        guided = "ILb1E" in name or "<true" in name
        nbytes = elems * (28 if guided else 20)
        mean_ns = float(s["AverageNs"])
        prof[name] = {"calls": int(s["Calls"]), "mean_us": mean_ns / 1e3, "GB_s": nbytes / mean_ns,
                      "share": float(s["TotalDurationNs"]) / total}
        print(f"| {'guided' if guided else 'unguided'} {name[:48]} | {s['Calls']} | {mean_ns / 1e3:.2f} | {nbytes / mean_ns:.0f} | "
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
