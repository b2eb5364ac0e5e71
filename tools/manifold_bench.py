"""Time of precision / recall / density / coverage and of its two fp64 contractions on one MI355X:

  kernel  ops.kth_neighbour (afd_kth_neighbour_f32), ops.ball_membership (afd_ball_membership_f32, count and nearest) and
          manifold_scores (two calls of each) on random 10 000 x 2048 and 50 000 x 2048 float32 features at k = 3: two launches
          a call, fp64 matrix pipe, no fp64 copy of the features, no distance matrix in memory
  torch   the same results with torch ops on the device: X.double() once, then blocks of rows of the Gram form s_i + s_j - 2 X Y^T
          from an fp64 matmul, clamped at 0; the k-th smallest per row (kthvalue or topk, whichever is faster on a trial block, named
          in the output), the comparison against the radii, the row sums and the row minima

    python tools/manifold_bench.py [--out FILE.json] [--windows 5] [--n 50000] [--n-small 10000] [--D 2048] [--k 3] [--block 2048]

Every figure is the median over W windows of a host clock around `reps` calls that end in a device synchronise, after warm-up,
with the fastest window and the 90th percentile as the spread; the kernel form and the torch form alternate window by window.
TFLOPs counts the fp64 multiply-adds the matrix pipe is ISSUED by the kernel's second launch, padding included, as 2 flop each:
ceil(nq / 64) ceil(nr / 64) tiles of 64 x 64 times D rounded up to 32.  `agree` compares the two forms: the largest relative
difference of the radii and of the nearest distances, and the share of rows whose count or nearest row differs (the two forms
round differently, so a distance on a threshold may fall either way)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _blocks(q64, r64, sq, sr, block):
    import torch
    for a in range(0, q64.shape[0], block):
        d = (sq[a:a + block].unsqueeze(1) + sr.unsqueeze(0)) - 2.0 * (q64[a:a + block] @ r64.T)
        yield a, torch.clamp_min_(d, 0.0)


def torch_kth(x, k, block, select):
    import torch
    x64 = x.double()
    s = (x64 * x64).sum(1)
    out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
    for a, d in _blocks(x64, x64, s, s, block):
        rows = torch.arange(d.shape[0], device=x.device)
        d[rows, a + rows] = float("inf")
        out[a:a + d.shape[0]] = d.kthvalue(k, dim=1).values if select == "kthvalue" else d.topk(k, dim=1, largest=False).values[:, k - 1]
    return out


def torch_ball(q, r, radius2, block):
    import torch
    q64, r64 = q.double(), r.double()
    sq, sr = (q64 * q64).sum(1), (r64 * r64).sum(1)
    count = torch.empty(q.shape[0], dtype=torch.int32, device=q.device)
    nearest = torch.empty(q.shape[0], dtype=torch.long, device=q.device)
    nearest_d2 = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    for a, d in _blocks(q64, r64, sq, sr, block):
        count[a:a + d.shape[0]] = (d <= radius2.unsqueeze(0)).sum(1)
        nearest_d2[a:a + d.shape[0]], nearest[a:a + d.shape[0]] = d.min(1)
    return count, nearest, nearest_d2


def torch_scores(fg, fr, k, block, select):
    import torch
    rad_g, rad_r = torch_kth(fg, k, block, select), torch_kth(fr, k, block, select)
    in_gen, _, to_gen = torch_ball(fr, fg, rad_g, block)
    in_real, _, _ = torch_ball(fg, fr, rad_r, block)
    ng, nr = fg.shape[0], fr.shape[0]
    a, b, c, d = torch.stack([(in_real >= 1).sum(), (in_gen >= 1).sum(), in_real.sum(dtype=torch.long), (to_gen <= rad_r).sum()]).tolist()
    p, r = a / ng, b / nr
    return {"precision": p, "recall": r, "f_score": 2 * p * r / (p + r) if p + r > 0 else 0.0, "density": c / (k * ng), "coverage": d / nr}


def windows(fns, W, reps, warm=1):
    """fns: {name: callable}; W windows of `reps` calls each, the forms alternating window by window."""
    import torch
    for f in fns.values():
        for _ in range(warm):
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
        out[name] = {"ms": round(w[len(w) // 2], 3), "ms_min": round(w[0], 3), "ms_p90": round(w[int(len(w) * 0.9)], 3)}
    return out


def main():
    sys.path.insert(0, ROOT)
    import torch
    import afdm
    if not torch.cuda.is_available():
        raise SystemExit("manifold_bench: no GPU")
    W, n, n_small, D, k, block = arg("--windows", 5), arg("--n", 50000), arg("--n-small", 10000), arg("--D", 2048), arg("--k", 3), arg("--block", 2048)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    real = (torch.randn(n, D, generator=g) * 0.5 + 0.3).to(dev)
    gen = (torch.randn(n, D, generator=g) * 0.45 + 0.32).to(dev)
    # the faster of the two selections on one block of the large case
    trial = torch.rand(block, n, dtype=torch.float64, device=dev)
    cost = windows({"kthvalue": lambda: trial.kthvalue(k, dim=1), "topk": lambda: trial.topk(k, dim=1, largest=False)}, 3, 1)
    select = min(cost, key=lambda name: cost[name]["ms"])
    print(json.dumps({"selection of the torch form": select, **cost}), flush=True)
    del trial
    Dp = -(-D // 32) * 32
    rows = []
    for size, reps in ((n_small, 3), (n, 1)):
        fr, fg = real[:size], gen[:size]
        T = -(-size // 64)
        flop = 2.0 * T * T * 64 * 64 * Dp
        forms = {"kernel": lambda: afdm.ops.kth_neighbour(fr, k), "torch": lambda: torch_kth(fr, k, block, select)}
        r = windows(forms, W, reps)
        rk, rt = forms["kernel"](), forms["torch"]()
        rows.append({"case": f"kth_neighbour {size} x {D}, k = {k}", **r, "agree": {"radius2 rel": float(((rk - rt).abs() / rt).max())},
                     "TFLOPs": round(flop / (r["kernel"]["ms"] * 1e-3) / 1e12, 2)})
        print(json.dumps(rows[-1]), flush=True)
        forms = {"kernel": lambda: afdm.ops.ball_membership(fg, fr, rk), "torch": lambda: torch_ball(fg, fr, rk, block)}
        r = windows(forms, W, reps)
        bk, bt = forms["kernel"](), forms["torch"]()
        rows.append({"case": f"ball_membership {size} x {size} x {D}", **r,
                     "agree": {"nearest_d2 rel": float(((bk[2] - bt[2]).abs() / bt[2]).max()), "count differs": float((bk[0] != bt[0]).double().mean()),
                               "nearest differs": float((bk[1] != bt[1]).double().mean())},
                     "TFLOPs": round(flop / (r["kernel"]["ms"] * 1e-3) / 1e12, 2)})
        print(json.dumps(rows[-1]), flush=True)
        forms = {"kernel": lambda: afdm.manifold_scores(fg, fr, k), "torch": lambda: torch_scores(fg, fr, k, block, select)}
        r = windows(forms, W, reps)
        sk, st = forms["kernel"](), forms["torch"]()
        rows.append({"case": f"manifold_scores {size} + {size} x {D}, k = {k}", **r, "agree": {key: abs(sk[key] - st[key]) for key in sk},
                     "scores": sk, "TFLOPs": round(4 * flop / (r["kernel"]["ms"] * 1e-3) / 1e12, 2)})
        print(json.dumps(rows[-1]), flush=True)
    print(f"\n(the torch form selects with {select})")
    print("| case | kernel ms (min .. p90) | torch ms (min .. p90) | torch / kernel | issued fp64 TFLOP/s |")
    print("|---|---|---|---|---|")
    for r in rows:
        a, b = r["kernel"], r["torch"]
        print(f"| {r['case']} | {a['ms']:.2f} ({a['ms_min']:.2f} .. {a['ms_p90']:.2f}) | {b['ms']:.2f} ({b['ms_min']:.2f} .. {b['ms_p90']:.2f}) | "
              f"{b['ms'] / a['ms']:.2f} x | {r['TFLOPs']} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"select": select, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
