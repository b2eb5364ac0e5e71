"""Cost of feeding the train step: a B = 256 variant-3 TrainStep at 32 x 32 on one MI355X, replayed on two lanes (graph="lanes"),
fed by the host loader (`get_data`: PIL per item, collate, H2D inside the loop), by `DeviceLoader` (the data set in device
memory, one gather launch per batch) and by one fixed device-resident batch (the bare step).  DESIGN.md section 6n.

    python tools/loader_bench.py [--out FILE.json] [--n 50000] [--windows 20]     # every row, one process per leg
    python tools/loader_bench.py --worker --leg host|device|bare --data DIR [--windows W]

The driver writes N synthetic 3 x 32 x 32 PNGs (two classes) into a temporary directory, which both loaders then read, and runs one
worker per leg under `timeout -k 10`, stopping at the first failure.  A worker prints one JSON line:
  loader_img_s      images/s of the loader alone (host: the first 40 batches; device: a whole epoch, then a sync)
  gather_us         the gather's time per launch, from 200 back-to-back launches of one batch (device leg)
  iter_ms           the median time per iteration of `for images, _ in loader: step(images)` over W windows of 10 full batches
                    (after 10 warm-up iterations), with the fastest window and the 90th percentile as the spread
The expectation to read off the table: the device-fed loop lies within the spread of the bare loop's windows, or within 1 % of its
median, whichever is larger (the margin DESIGN.md section 6i uses for one more launch on this step)."""
import itertools
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
B = 256


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def write_pngs(root, n):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(0)
    for c in ("a", "b"):
        os.makedirs(os.path.join(root, c), exist_ok=True)
    px = rng.integers(0, 256, (n, 32, 32, 3), dtype=np.uint8)
    for i in range(n):
        Image.fromarray(px[i]).save(os.path.join(root, "ab"[i & 1], f"{i:06d}.png"))


def _windows(batches, step, W, to_dev):
    """W windows of 10 iterations of `step(images)` over `batches` (an endless generator), after 10 warm-up iterations."""
    import gc
    import torch
    for _ in range(10):
        step(to_dev(next(batches)))
    torch.cuda.synchronize()
    gc.collect()
    gc.disable()
    w = []
    for _ in range(W):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            step(to_dev(next(batches)))
        torch.cuda.synchronize()
        w.append((time.perf_counter() - t0) / 10 * 1e3)
    gc.enable()
    w.sort()
    return {"iter_ms": round(w[len(w) // 2], 4), "iter_ms_min": round(w[0], 4), "iter_ms_p90": round(w[int(len(w) * 0.9)], 4)}


def _full_batches(loader):
    """The loader's full batches, epoch after epoch (the ragged last one is left out of the windows)."""
    while True:
        for images, _ in loader:
            if images.shape[0] == B:
                yield images


def worker():
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    leg, data, W = arg("--leg", "bare"), arg("--data", ""), arg("--windows", 20)
    dev = torch.device("cuda:0")
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    step = afdm.TrainStep(model, diff, lr=3e-4, graph="lanes")
    args = afdm.argument(batch_size=B, image_size=32, dataset_path=data, device=dev)
    row = {"leg": leg, "B": B, "windows": W}
    if leg == "bare":
        images = torch.rand(B, 3, 32, 32, device=dev) * 2 - 1
        row.update(_windows(itertools.repeat(images), step, W, lambda x: x))
    elif leg == "host":
        loader, dataset = afdm.get_data(args)
        it, n = iter(loader), 0
        t0 = time.perf_counter()
        for _ in range(40):
            n += next(it)[0].shape[0]
        row.update(n_images=len(dataset), loader_img_s=round(n / (time.perf_counter() - t0), 1))
        row.update(_windows(_full_batches(loader), step, W, lambda x: x.to(dev)))
    else:
        t0 = time.perf_counter()
        loader, dataset = afdm.get_data_device(args)
        row.update(n_images=len(dataset), build_s=round(time.perf_counter() - t0, 2))
        for _ in loader:                                   # (the first epoch also warms the allocator)
            pass
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = sum(images.shape[0] for images, _ in loader)
        torch.cuda.synchronize()
        row["loader_img_s"] = round(n / (time.perf_counter() - t0), 1)
        idx = torch.randperm(len(dataset), device=dev)[:B]
        for _ in range(20):
            dataset.batch(idx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            dataset.batch(idx)
        torch.cuda.synchronize()
        row["gather_us"] = round((time.perf_counter() - t0) / 200 * 1e6, 2)
        row.update(_windows(_full_batches(loader), step, W, lambda x: x))
    print(json.dumps(row), flush=True)


def _run(cmd, limit):
    """One GPU step under its own time limit; None after any failure (the caller then starts nothing more)."""
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    if p.returncode != 0:
        print(f"FAILED rc={p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}", flush=True)
        return None
    return p


def driver():
    W, n = arg("--windows", 20), arg("--n", 50000)
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        write_pngs(tmp, n)
        print(f"wrote {n} PNGs in {time.perf_counter() - t0:.1f} s", flush=True)
        for leg in ("bare", "device", "host"):
            p = _run([sys.executable, "tools/loader_bench.py", "--worker", "--leg", leg, "--data", tmp, "--windows", str(W)], 400)
            if p is None:
                return 1
            rows[leg] = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(rows[leg]), flush=True)
    bare = rows["bare"]
    spread = bare["iter_ms_p90"] - bare["iter_ms_min"]
    print("\n| fed by | ms/iteration (min .. p90) | over the bare step | loader alone, images/s |")
    print("|---|---|---|---|")
    for leg, name in (("bare", "one fixed batch"), ("device", "DeviceLoader"), ("host", "get_data")):
        r = rows[leg]
        d = r["iter_ms"] - bare["iter_ms"]
        print(f"| {name} | {r['iter_ms']:.3f} ({r['iter_ms_min']:.3f} .. {r['iter_ms_p90']:.3f}) | "
              f"{1e3 * d:+.0f} us ({100 * d / bare['iter_ms']:+.2f} %) | {r.get('loader_img_s', '-')} |")
    d = rows["device"]["iter_ms"] - bare["iter_ms"]
    print(f"\ngather: {rows['device']['gather_us']} us per launch; device-fed minus bare {1e3 * d:+.0f} us against a margin of "
          f"{1e3 * max(spread, 0.01 * bare['iter_ms']):.0f} us (the bare windows' spread, or 1 %)")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)
    return 0


if __name__ == "__main__":
    if "--worker" in sys.argv:
        worker()
    else:
        sys.exit(driver())
