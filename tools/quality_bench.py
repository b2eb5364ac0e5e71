"""Time of PSNR / SSIM of image pairs on one MI355X:

  kernel  image_quality on device tensors: one launch of afd_pair_quality_u8 / _f32 (one workgroup per plane, the plane read once,
          five fp64 sums out) and a handful of (n, C)-sized torch ops for the dict; `launch` is ops.pair_quality alone
  torch   the same result with torch ops on the same device in the same process: the five maps a, b, a a, b b, a b stacked in fp64,
          one grouped conv2d with the 11 x 11 outer product of the Gaussian window, the elementwise formula, and the means

    python tools/quality_bench.py [--out FILE.json] [--windows 7] [--reps 20]

Cases: 256 x 3 x 32 x 32 and 10000 x 3 x 32 x 32 uint8, 1024 x 1 x 64 x 64 float32, window 11 / 1.5.  Every figure is the median over
W windows of device events around `reps` calls, after warm-up, with the fastest window and the 90th percentile as the spread; the
forms alternate window by window.  GFMA/s counts the kernel's fp64 multiply-adds, 5 K (K + 1) per window, over the launch's time.
`agree` is the largest absolute difference of the two forms' per-image SSIM and the largest relative one of their MSE.  Nothing
here gates on time: a form that loses is printed as it is."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (((256, 3, 32, 32), "uint8"), ((10000, 3, 32, 32), "uint8"), ((1024, 1, 64, 64), "float32"))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_quality(a, b, win, L, chunk=2048):
    """{"mse", "ssim"} (n,) fp64 from stock ops, `chunk` images at a time."""
    import torch
    import torch.nn.functional as F
    n, C = a.shape[:2]
    K = win.shape[0]
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    w = torch.outer(win, win).view(1, 1, K, K).expand(5 * C, 1, K, K).contiguous()
    mse, ssim = [], []
    for lo in range(0, n, chunk):
        x, y = a[lo:lo + chunk].double(), b[lo:lo + chunk].double()
        d = x - y
        mse.append((d * d).mean((1, 2, 3)))
        m = F.conv2d(torch.cat([x, y, x * x, y * y, x * y], 1), w, groups=5 * C)
        ma, mb, maa, mbb, mab = m.split(C, 1)
        vaa, vbb, vab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
        s = ((2.0 * ma * mb + c1) * (2.0 * vab + c2)) / ((ma * ma + mb * mb + c1) * (vaa + vbb + c2))
        ssim.append(s.mean((1, 2, 3)))
    return {"mse": torch.cat(mse), "ssim": torch.cat(ssim)}


def windows(fns, W, reps, warm=2):
    """fns: {name: callable}; W windows of `reps` calls each between two device events, the forms alternating window by window."""
    import torch
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(W):
        for name, f in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(reps):
                f()
            t1.record()
            torch.cuda.synchronize()
            t[name].append(t0.elapsed_time(t1) / reps)
    out = {}
    for name, w in t.items():
        w.sort()
        out[name] = {"ms": round(w[len(w) // 2], 4), "ms_min": round(w[0], 4), "ms_p90": round(w[int(len(w) * 0.9)], 4)}
    return out


def main():
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    if not torch.cuda.is_available():
        raise SystemExit("quality_bench: no GPU")
    W, reps = arg("--windows", 7), arg("--reps", 20)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    win = afdm.gaussian_window()
    win_dev = win.to(dev)
    rows = []
    for shape, kind in CASES:
        if kind == "uint8":
            a, b = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(dev) for _ in range(2))
            L = 255.0
        else:
            a, b = ((torch.rand(shape, generator=g) * 2 - 1).to(dev) for _ in range(2))
            L = 2.0
        c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
        forms = {"kernel": lambda: afdm.image_quality(a, b), "launch": lambda: afdm.ops.pair_quality(a, b, win, c1, c2),
                 "torch": lambda: torch_quality(a, b, win_dev, L)}
        r = windows(forms, W, reps if shape[0] < 5000 else max(2, reps // 4))
        k, t = forms["kernel"](), forms["torch"]()
        n, C, H, Wd = shape
        fma = n * C * (H - 10) * (Wd - 10) * 5 * 11 * 12
        rows.append({"case": f"{' x '.join(map(str, shape))} {kind}", **r,
                     "agree": {"ssim abs": float((k["ssim"] - t["ssim"]).abs().max()), "mse rel": float(((k["mse"] - t["mse"]).abs() / t["mse"]).max())},
                     "GFMAs": round(fma / (r["launch"]["ms"] * 1e-3) / 1e9, 1)})
        print(json.dumps(rows[-1]), flush=True)
    print("\n| case | image_quality ms (min .. p90) | the launch alone ms | torch ms (min .. p90) | torch / image_quality | fp64 GFMA/s of the launch |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        a, l, b = r["kernel"], r["launch"], r["torch"]
        print(f"| {r['case']} | {a['ms']:.3f} ({a['ms_min']:.3f} .. {a['ms_p90']:.3f}) | {l['ms']:.3f} | {b['ms']:.3f} ({b['ms_min']:.3f} .. "
              f"{b['ms_p90']:.3f}) | {b['ms'] / a['ms']:.2f} x | {r['GFMAs']} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
