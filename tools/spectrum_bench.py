"""Time of the mean power spectrum of an image set on one MI355X:

  kernel  DeviceDataset.power_spectrum (afd_power_spectrum_u8 / _f32: two launches, fp64 matrix pipe), Hann window, mean removed,
          on a random 50 000 x 3 x 32 x 32 uint8 store, on its first 256 images, and on a 10 000 x 1 x 64 x 64 float32 store
  torch   the same result with torch ops on the device, in chunks of 8192 images: table lookup, fp64, mean removal, window,
          torch.fft.rfft2, |.|^2, sum; divided by n at the end

    python tools/spectrum_bench.py [--out FILE.json] [--windows 15] [--n-store 50000] [--n-f32 10000] [--kernel-only]

Every figure is the median over W windows of a host clock around `reps` calls that end in a device synchronise, after warm-up,
with the fastest window and the 90th percentile as the spread; the kernel form and the torch form alternate window by window.
planes_per_us is n C over the kernel form's time; GMAC_per_s counts the multiply-adds the matrix pipe is ISSUED, padding
included: per plane ceil(H / 16) ceil(Wh / 16) tiles of (2 ceil(W / 4) + 4 ceil(H / 4)) instructions of 16 x 16 x 4; store_GBps is
the set's bytes over that time.  rel_l2 is the distance between the two forms' spectra.  --kernel-only runs the kernel form
alone, three calls per set (for a kernel trace)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_spectrum(images, table, win, remove_mean=True):
    """-> (C, H, W // 2 + 1) fp64.  win: the (H, W) fp64 window on the device, or None."""
    import torch
    n, C = images.shape[:2]
    ch = torch.arange(C, device=images.device).view(1, C, 1, 1)
    total = None
    for a in range(0, n, CHUNK):
        x = images[a:a + CHUNK]
        x = table[ch, x.long()].double() if table is not None else x.double()
        if remove_mean:
            x = x - x.mean(dim=(-2, -1), keepdim=True)
        if win is not None:
            x = x * win
        f = torch.fft.rfft2(x)
        p = (f.real * f.real + f.imag * f.imag).sum(0)
        total = p if total is None else total + p
    return total / n


def issued_macs(n, C, H, W):
    Wh = W // 2 + 1
    tiles = -(-H // 16) * -(-Wh // 16)
    return n * C * tiles * (2 * -(-W // 4) + 4 * -(-H // 4)) * 16 * 16 * 4


def windows(fns, W, reps):
    """fns: {name: callable}; W windows of `reps` calls each, the forms alternating window by window."""
    import torch
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    for _ in range(W):
        for name, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / reps * 1e3)
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
        raise SystemExit("spectrum_bench: no GPU")
    W, n_store, n_f32 = arg("--windows", 15), arg("--n-store", 50000), arg("--n-f32", 10000)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    store = afdm.DeviceDataset(torch.randint(0, 256, (n_store, 3, 32, 32), generator=g, dtype=torch.uint8), device=dev)
    floats = afdm.DeviceDataset(torch.randn(n_f32, 1, 64, 64, generator=g), device=dev)
    cases = (("u8 3x32x32", store, n_store, 5), ("u8 3x32x32", store, 256, 50), ("f32 1x64x64", floats, n_f32, 5))
    rows = []
    for name, ds, n, reps in cases:
        C, H, Wd = ds.images.shape[1:]
        win = (afdm.hann_window(H).view(H, 1) * afdm.hann_window(Wd).view(1, Wd)).to(dev)
        forms = {"kernel": lambda: ds.power_spectrum(n=n)["power"]}
        if "--kernel-only" in sys.argv:
            for _ in range(3):
                forms["kernel"]()
            torch.cuda.synchronize()
            continue
        forms["torch"] = lambda: torch_spectrum(ds.images[:n], ds.table, win)
        r = windows(forms, W, reps)
        a, b = forms["kernel"](), forms["torch"]()
        sec = r["kernel"]["ms"] * 1e-3
        rows.append({"set": name, "n": n, **r, "rel_l2": float((a - b).norm() / b.norm()), "planes_per_us": round(n * C / sec / 1e6, 2),
                     "GMAC_per_s": round(issued_macs(n, C, H, Wd) / sec / 1e9, 1),
                     "store_GBps": round(ds.images[:n].numel() * ds.images.element_size() / sec / 1e9, 1)})
        print(json.dumps(rows[-1]), flush=True)
    if rows:
        print("\n| set | n | kernel ms (min .. p90) | torch ms (min .. p90) | torch / kernel | planes / us | issued GMAC/s | set GB/s | rel-L2 |")
        print("|---|---|---|---|---|---|---|---|---|")
        for r in rows:
            a, b = r["kernel"], r["torch"]
            print(f"| {r['set']} | {r['n']} | {a['ms']:.3f} ({a['ms_min']:.3f} .. {a['ms_p90']:.3f}) | "
                  f"{b['ms']:.3f} ({b['ms_min']:.3f} .. {b['ms_p90']:.3f}) | {b['ms'] / a['ms']:.2f} x | {r['planes_per_us']} | {r['GMAC_per_s']} | "
                  f"{r['store_GBps']} | {r['rel_l2']:.1e} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
