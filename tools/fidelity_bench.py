"""Time of the two fp64 contractions behind FID and KID on one MI355X:

  kernel  ops.feature_moments (afd_feature_moments_f32) on random 50 000 x 2048 and 10 000 x 2048 float32 features, and
          ops.poly_mmd_sums (afd_poly_mmd_sums_f32) on 100 subsets of 1000 rows out of two 10 000 x 2048 sets, degree 3: two
          launches each, fp64 matrix pipe, no fp64 copy of the features, no Gram matrix in memory
  torch   the same results with torch ops on the device: X.double().T @ X.double() plus the column sum; per subset gather, fp64
          matmul, pow, masked sum

    python tools/fidelity_bench.py [--out FILE.json] [--windows 7] [--n 50000] [--n-small 10000] [--D 2048] [--subsets 100] [--m 1000]

Every figure is the median over W windows of a host clock around `reps` calls that end in a device synchronise, after warm-up,
with the fastest window and the 90th percentile as the spread; the kernel form and the torch form alternate window by window.
TFLOPs counts the fp64 multiply-adds the matrix pipe is ISSUED, padding included, as 2 flop each: for the moments the 64 x 64 tiles
on or above the diagonal times n, for the MMD the tiles of the three Gram matrices (upper triangles for the symmetric two) times
D.  rel is the largest relative difference between the two forms' results."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_moments(x):
    x64 = x.double()
    return x64.sum(0), x64.T @ x64


def torch_mmd_sums(a, b, ia, ib, degree, gamma, coef0):
    import torch
    S, m = ia.shape
    off = ~torch.eye(m, dtype=torch.bool, device=a.device)
    out = torch.empty(S, 3, dtype=torch.float64, device=a.device)
    for s in range(S):
        x, y = a[ia[s]].double(), b[ib[s]].double()
        out[s, 0] = (((gamma * (x @ x.T) + coef0) ** degree) * off).sum()
        out[s, 1] = (((gamma * (y @ y.T) + coef0) ** degree) * off).sum()
        out[s, 2] = ((gamma * (x @ y.T) + coef0) ** degree).sum()
    return out


def windows(fns, W, reps):
    """fns: {name: callable}; W windows of `reps` calls each, the forms alternating window by window."""
    import torch
    for f in fns.values():
        for _ in range(2):
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
        raise SystemExit("fidelity_bench: no GPU")
    W, n, n_small, D = arg("--windows", 7), arg("--n", 50000), arg("--n-small", 10000), arg("--D", 2048)
    S, m = arg("--subsets", 100), arg("--m", 1000)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    big = (torch.randn(n, D, generator=g) * 0.5 + 0.3).to(dev)
    other = (torch.randn(n_small, D, generator=g) * 0.6 + 0.2).to(dev)
    T = -(-D // 64)
    rows = []
    for name, x, reps in ((f"moments {n} x {D}", big, 20), (f"moments {n_small} x {D}", big[:n_small], 100)):      # ~0.1 s a window
        forms = {"kernel": lambda: afdm.ops.feature_moments(x), "torch": lambda: torch_moments(x)}
        r = windows(forms, W, reps)
        (s1, o1), (s2, o2) = forms["kernel"](), forms["torch"]()
        flop = 2.0 * x.shape[0] * (T * (T + 1) // 2) * 64 * 64
        rows.append({"case": name, **r, "rel": float(max(((s1 - s2).abs() / s2.abs().max()).max(), ((o1 - o2).abs() / o2.abs().max()).max())),
                     "TFLOPs": round(flop / (r["kernel"]["ms"] * 1e-3) / 1e12, 2)})
        print(json.dumps(rows[-1]), flush=True)
    ia, ib = (torch.from_numpy(t).to(dev) for t in afdm.mmd_indices(n_small, n_small, S, m, 2020))
    a, b = big[:n_small], other
    forms = {"kernel": lambda: afdm.ops.poly_mmd_sums(a, b, ia, ib, 3, 1.0 / D, 1.0, check_range=False),
             "torch": lambda: torch_mmd_sums(a, b, ia, ib, 3, 1.0 / D, 1.0)}
    r = windows(forms, W, 4)
    k, t = forms["kernel"](), forms["torch"]()
    MT = -(-m // 64)
    flop = 2.0 * S * (MT * (MT + 1) + MT * MT) * 64 * 64 * (-(-D // 32) * 32)
    rows.append({"case": f"MMD sums {S} x {m} x {D}", **r, "rel": float(((k - t).abs() / t.abs()).max()),
                 "TFLOPs": round(flop / (r["kernel"]["ms"] * 1e-3) / 1e12, 2)})
    print(json.dumps(rows[-1]), flush=True)
    print("\n| case | kernel ms (min .. p90) | torch ms (min .. p90) | torch / kernel | issued fp64 TFLOP/s | largest relative difference |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["kernel"], r["torch"]
        print(f"| {r['case']} | {a['ms']:.2f} ({a['ms_min']:.2f} .. {a['ms_p90']:.2f}) | {b['ms']:.2f} ({b['ms_min']:.2f} .. {b['ms_p90']:.2f}) | "
              f"{b['ms'] / a['ms']:.2f} x | {r['TFLOPs']} | {r['rel']:.1e} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
