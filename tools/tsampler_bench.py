"""Cost of loss-aware timestep sampling in the train step: a B = 256 variant-3 TrainStep at 32 x 32 on one MI355X, replayed on two
lanes (graph="lanes"), with the sampler off (the default step) and on (TrainStep(t_sampler="loss_second_moment"): the draw outside
the replayed list, afd_loss_rows and afd_tsampler_tick inside it, the loss through the sampler's weight table).

    python tools/tsampler_bench.py [--out FILE.json] [--windows 30] [--learned]     # both rows, one process per configuration
    python tools/tsampler_bench.py --worker [--sampler] [--learned] [--windows W]

A worker measures ONE configuration in its own process and prints one JSON line: step_ms, the median over W windows of 10 train
steps (after 10 warm-up steps, which with 1000 noise steps leave the sampler cold: its launches cost the same warm or cold, so a
second on-row, "warm", starts from a history filled with ones), with the fastest window and the 90th percentile as the spread
(the method of tools/step_median.py and tools/clip_bench.py).  --learned measures the hybrid loss (variance="learned", a UNet with
six output channels) instead.  The driver runs every worker under `timeout -k 10` and stops at the first failure."""
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
B = 256


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def worker():
    import gc
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    sampler, warm, learned, W = "--sampler" in sys.argv, "--warm" in sys.argv, "--learned" in sys.argv, arg("--windows", 30)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=6 if learned else 3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, **({"variance": "learned"} if learned else {}))
    ts = afdm.LossSecondMomentSampler(diff) if sampler else None
    if warm:
        ts.load_state_dict({"hist": torch.ones(ts.T, ts.H, dtype=torch.float64), "count": torch.full((ts.T,), ts.H, dtype=torch.int32),
                            "history_per_term": ts.H, "uniform_prob": ts.uniform_prob})
    step = afdm.TrainStep(model, diff, lr=3e-4, graph="lanes", t_sampler=ts)
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
            step(images)
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    w.sort()
    row = {"sampler": sampler, "warm": warm, "learned": learned, "B": B, "windows": W, "step_ms": round(w[len(w) // 2], 4),
           "step_ms_min": round(w[0], 4), "step_ms_p90": round(w[int(len(w) * 0.9)], 4), "work_nodes": step.lanes_counts[0]}
    if sampler:
        row.update(warmed_up=ts.warmed_up, seen=int((ts.count > 0).sum()))
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
    extra = ["--learned"] if "--learned" in sys.argv else []
    rows = []
    for flags in ([], ["--sampler"], ["--sampler", "--warm"]):
        p = _run([sys.executable, "tools/tsampler_bench.py", "--worker", "--windows", str(W)] + flags + extra, 300)
        if p is None:
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        rows.append(r)
        print(json.dumps(r), flush=True)
    off = rows[0]
    print("\n| sampler | ms/step (min .. p90) | difference | work nodes |")
    print("|---|---|---|---|")
    for r, name in zip(rows, ("off", "on, cold", "on, warm")):
        d = r["step_ms"] - off["step_ms"]
        print(f"| {name} | {r['step_ms']:.3f} ({r['step_ms_min']:.3f} .. {r['step_ms_p90']:.3f}) | "
              f"{1e3 * d:+.0f} us ({100 * d / off['step_ms']:+.2f} %) | {r['work_nodes']} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    else:
        sys.exit(driver())
