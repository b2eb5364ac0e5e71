"""Cost of the bits/dim bound (Diffusion.calc_bpd), variant 3 at 32 x 32, T = 1000, one MI355X.

    python tools/bpd_bench.py [--out FILE.json] [--prof-dir DIR] [--images N]   # the whole table, one process per batch size
    python tools/bpd_bench.py --worker --batch B [--images N]
    python tools/bpd_bench.py --profile-run                   # the process that the driver runs under rocprofv3

A worker measures ONE batch size in its own process and prints one JSON line: the wall time of the full bound (T - 1 = 999
rows per image) over N images (default 128), the median of 3 calls after one warm-up call of the same size (every chunk
shape the timed calls use is then warm).  rows_s = N * 999 / time; s_per_1000 = the seconds 1000 images would take.
The driver runs every worker under `timeout -k 10`, stops at the first failure, then runs --profile-run once under
`rocprofv3 --kernel-trace --stats` (a process of its own) and reports the bound-terms and gathered-noising kernels' own time,
their achieved bandwidth and their share of all kernel time of the loop."""
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
BATCHES = (64, 256, 512)
D = 3 * 32 * 32


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
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8)
    return torch, afdm, model, diff, images


def worker():
    batch, n = arg("--batch", 256), arg("--images", 128)
    torch, afdm, model, diff, images = _setup(n)
    diff.calc_bpd(model, images, batch=batch)                    # warm-up: every chunk shape of the timed calls
    times, bpd = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bpd = diff.calc_bpd(model, images, batch=batch)["bpd"]    # ends in a device-to-host copy of the results
        times.append(time.perf_counter() - t0)
    times.sort()
    ts = times[1]
    print(json.dumps({"batch": batch, "images": n, "rows": n * (T - 1), "time_s": round(ts, 4), "time_s_min": round(times[0], 4),
                      "rows_s": round(n * (T - 1) / ts, 1), "s_per_1000": round(1000 * ts / n, 3),
                      "ms_per_forward": round(1e3 * ts / math.ceil(n * (T - 1) / batch), 4), "bpd_mean": float(bpd.mean())}),
          flush=True)


def profile_run():
    """16 images at batch 256 (63 forwards): the kernels of the loop, the terms kernel among them.  On a KL row the terms
    kernel reads eps and eps_hat (8 B per element); gathered noising reads x0 and eps and writes x_t (12 B per element)."""
    torch, afdm, model, diff, images = _setup(16)
    diff.calc_bpd(model, images, batch=256)
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
    n = arg("--images", 128)
    rows = []
    for batch in BATCHES:
        p = _run([sys.executable, "tools/bpd_bench.py", "--worker", "--batch", str(batch), "--images", str(n)], 600)
        if p is None:
            return 1
        r = json.loads(p.stdout.strip().splitlines()[-1])
        rows.append(r)
        print(json.dumps(r), flush=True)
    print("\n| batch | rows/s | s per 1000 images | ms per forward (chunk) | mean bpd |")
    print("|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['batch']} | {r['rows_s']:.0f} | {r['s_per_1000']:.2f} | {r['ms_per_forward']:.3f} | {r['bpd_mean']:.4f} |")

    prof = {}
    pdir = arg("--prof-dir", "") or tempfile.mkdtemp(prefix="bpd_prof_")      # the raw rocprofv3 output stays there
    p = _run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "bpd", "--",
              sys.executable, "tools/bpd_bench.py", "--profile-run"], 900)
    if p is None:
        return 1
    stats = _kernel_stats(pdir)
    total = sum(float(s.get("TotalDurationNs", 0)) for s in stats)
    print(f"\nall kernels of the profiled loop: {total / 1e6:.2f} ms")
    print("| kernel | calls | mean us | GB/s (256-row chunk) | share of all kernel time |")
    print("|---|---|---|---|---|")
    for s in stats:
        name = s.get("Name", s.get("KernelName", ""))
        kind = "terms" if "vlb_terms" in name else "gather" if "noise_images_gather" in name else "prior" if "vlb_prior" in name else None
        if kind is None:
            continue
        mean_ns = float(s["AverageNs"])
        nbytes = {"terms": 256 * D * 8, "gather": 256 * D * 12, "prior": 16 * D * 4}[kind]
        prof[name] = {"kind": kind, "calls": int(s["Calls"]), "mean_us": mean_ns / 1e3, "GB_s": nbytes / mean_ns,
                      "share": float(s["TotalDurationNs"]) / total}
        print(f"| {kind} {name[:56]} | {s['Calls']} | {mean_ns / 1e3:.2f} | {nbytes / mean_ns:.0f} | "
              f"{100 * float(s['TotalDurationNs']) / total:.2f} % |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows, "kernels": prof, "all_kernels_ms": total / 1e6}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    elif "--profile-run" in sys.argv:
        profile_run()
    else:
        sys.exit(driver())
