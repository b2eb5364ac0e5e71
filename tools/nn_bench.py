"""Time of the nearest-training-image search on one MI355X:

  nearest       DeviceDataset.nearest, 256 random uint8 queries against a random 50 000 x 3 x 32 x 32 uint8 store, k = 1, 5, 16
  self_nearest  DeviceDataset.self_nearest(k, batch = 1024) on a 10 000-row store of the same shape
  torch         the same two searches written with torch ops on the device: the store in chunks of 8192 rows turned to fp32,
                |a|^2 + |b|^2 - 2 a b with one fp32 matmul per chunk, the own row masked for the leave-one-out form, torch.topk
                over the chunk's candidates and the best so far

    python tools/nn_bench.py [--out FILE.json] [--windows 15] [--n-store 50000] [--n-self 10000]

Every figure is the median over W windows of a host clock around `reps` calls that end in a device synchronise, after warm-up,
with the fastest window and the 90th percentile as the spread; the kernel form and the torch form alternate window by window.
store_GBps is N D bytes over the time of one `nearest` call: the rate at which the store passes through the search (one pass per
call).  agree is the share of queries whose neighbour lists are equal in both forms (the fp32 expansion may order near-ties
differently; the kernel's lists are the exact ones)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_nearest(store, queries, k, own=None):
    """Chunked fp32 expansion + topk.  own: None or (n,) the store index each query must skip."""
    import torch
    q = queries.reshape(queries.shape[0], -1).float()
    qn = (q * q).sum(1, keepdim=True)
    flat = store.reshape(store.shape[0], -1)
    best_d = best_i = None
    for a in range(0, flat.shape[0], CHUNK):
        s = flat[a:a + CHUNK].float()
        d = qn + (s * s).sum(1)[None] - 2.0 * (q @ s.t())
        if own is not None:
            d.masked_fill_(own[:, None] == torch.arange(a, a + s.shape[0], device=d.device)[None], float("inf"))
        cd, ci = torch.topk(d, min(k, d.shape[1]), dim=1, largest=False)
        ci = ci + a
        if best_d is not None:
            cd, ci = torch.cat([best_d, cd], 1), torch.cat([best_i, ci], 1)
            cd, sel = torch.topk(cd, min(k, cd.shape[1]), dim=1, largest=False)
            ci = ci.gather(1, sel)
        best_d, best_i = cd, ci
    return best_d, best_i


def torch_self_nearest(store, k, batch=1024):
    import torch
    own = torch.arange(store.shape[0], device=store.device)
    parts = [torch_nearest(store, store[a:a + batch], k, own[a:a + batch]) for a in range(0, store.shape[0], batch)]
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


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
        raise SystemExit("nn_bench: no GPU")
    W, n_store, n_self = arg("--windows", 15), arg("--n-store", 50000), arg("--n-self", 10000)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    store = afdm.DeviceDataset(torch.randint(0, 256, (n_store, 3, 32, 32), generator=g, dtype=torch.uint8), device=dev)
    small = afdm.DeviceDataset(store.images[:n_self].cpu(), device=dev)
    queries = torch.randint(0, 256, (256, 3, 32, 32), generator=g, dtype=torch.uint8).to(dev)
    rows = []
    for k in (1, 5, 16):
        r = windows({"kernel": lambda: store.nearest(queries, k), "torch": lambda: torch_nearest(store.images, queries, k)}, W, 10)
        same = (store.nearest(queries, k)[1] == torch_nearest(store.images, queries, k)[1]).all(1).float().mean().item()
        rows.append({"search": "nearest", "N": n_store, "n": 256, "k": k, **r, "agree": round(same, 4),
                     "store_GBps": round(store.images.numel() / (r["kernel"]["ms"] * 1e-3) / 1e9, 1)})
        print(json.dumps(rows[-1]), flush=True)
    for k in (1, 5):
        r = windows({"kernel": lambda: small.self_nearest(k), "torch": lambda: torch_self_nearest(small.images, k)}, W, 2)
        same = (small.self_nearest(k)[1] == torch_self_nearest(small.images, k)[1]).all(1).float().mean().item()
        passes = -(-n_self // 1024)
        rows.append({"search": "self_nearest", "N": n_self, "n": n_self, "k": k, **r, "agree": round(same, 4),
                     "store_GBps": round(passes * small.images.numel() / (r["kernel"]["ms"] * 1e-3) / 1e9, 1)})
        print(json.dumps(rows[-1]), flush=True)
    print("\n| search | N | n | k | kernel ms (min .. p90) | torch ms (min .. p90) | torch / kernel | store GB/s | agree |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        a, b = r["kernel"], r["torch"]
        print(f"| {r['search']} | {r['N']} | {r['n']} | {r['k']} | {a['ms']:.3f} ({a['ms_min']:.3f} .. {a['ms_p90']:.3f}) | "
              f"{b['ms']:.3f} ({b['ms_min']:.3f} .. {b['ms_p90']:.3f}) | {b['ms'] / a['ms']:.1f} x | {r['store_GBps']} | {r['agree']} |")
    if "--out" in sys.argv:
        with open(arg("--out", ""), "w") as fh:
            json.dump({"rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
