"""Cost of the real-image methods (inversion, slerp, decode), variant 3 at 3 x 32 x 32, one MI355X.

    python tools/edit_bench.py [--out FILE.json] [--reps 5]

Prints one JSON line per measurement and, with --out, writes them all to FILE.json:
  step        us per ascending DDIM step at n = 6 and n = 256 images: the fused launch (`ops.ddim_invert_step`, into a second
              buffer as `Diffusion.invert` runs it) against the same expression in torch ops (six launches and their
              intermediate tensors; the four scalars are taken on the host once, outside the window).  HIP events around 1000
              back-to-back steps, median of --reps such windows; the two forms alternate window by window so that drift hits
              both.  The two results are compared first (rel-L2 in fp64).
  slerp       us per `ops.slerp` of 256 pairs x 8 weights of 3 x 32 x 32 rows against a torch fp64 implementation of the same
              definition (norms and dot products per pair, the coefficients, the weighted sum, one rounding to fp32), timed the
              same way over windows of 200.
  roundtrip   seconds per `invert` + `decode` at n = 256, S = 50, refine in {0, 2}, eager, against seconds per
              `sample(steps=50)` at the same n: medians over --reps whole calls, alternating.  forwards: what each ran.
"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    import afdm
    from afdm import ops
    reps = arg("--reps", 5)
    dev = torch.device("cuda:0")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def windows(forms, window):
        """{name: [us per call, one per window]}: 50 warm-up calls each, then --reps windows per form, alternating."""
        wins = {name: [] for name in forms}
        for fn in forms.values():
            for _ in range(50):
                fn()
        for _ in range(reps):
            for name, fn in forms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(window):
                    fn()
                b.record()
                b.synchronize()
                wins[name].append(a.elapsed_time(b) * 1e3 / window)
        return wins

    def spread(v):
        return [round(min(v), 3), round(max(v), 3)]

    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)

    # the ascending step alone
    s, u = 350, 700
    a_s, a_u = float(diff.alpha_hat[s]), float(diff.alpha_hat[u])
    k = [math.sqrt(1 - a_s), math.sqrt(a_s), math.sqrt(a_u), math.sqrt(1 - a_u)]
    for n in (6, 256):
        g = torch.Generator().manual_seed(n)
        x, e = (torch.randn((n, 3, 32, 32), generator=g).to(dev) for _ in range(2))
        out = torch.empty_like(x)

        def fused():
            return ops.ddim_invert_step(x, e, diff.alpha_hat, s, u, out=out)

        def composed():
            return ((x - e * k[0]) / k[1]) * k[2] + e * k[3]

        with torch.no_grad():
            err = float((fused().double() - composed().double()).norm() / composed().double().norm())
            wins = windows({"fused": fused, "composed": composed}, 1000)
        f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["composed"])
        emit({"what": "step", "n": n, "s": s, "u": u, "fused_us": round(f_us, 3), "composed_us": round(c_us, 3), "composed_launches": 6,
              "speedup": round(c_us / f_us, 3), "fused_spread_us": spread(wins["fused"]), "composed_spread_us": spread(wins["composed"]),
              "rel_l2_between_them": err})

    # slerp
    pairs, W = 256, 8
    g = torch.Generator().manual_seed(1)
    a, b = (torch.randn((pairs, 3, 32, 32), generator=g).to(dev) for _ in range(2))
    w = torch.linspace(0, 1, W)
    w64 = w.to(dev).double().view(1, W, 1)

    def torch_slerp():
        a64, b64 = a.flatten(1).double(), b.flatten(1).double()
        na, nb, d = (a64 * a64).sum(1), (b64 * b64).sum(1), (a64 * b64).sum(1)
        omega = torch.acos((d / torch.sqrt(na * nb)).clamp(-1, 1)).view(pairs, 1, 1)
        so = torch.sin(omega)
        lerp = (so < 1e-6) | (na == 0).view(pairs, 1, 1) | (nb == 0).view(pairs, 1, 1)
        ca = torch.where(lerp, 1 - w64, torch.sin((1 - w64) * omega) / so)
        cb = torch.where(lerp, w64.expand(pairs, W, 1), torch.sin(w64 * omega) / so)
        return (ca * a64[:, None] + cb * b64[:, None]).float().view(pairs, W, 3, 32, 32)

    with torch.no_grad():
        err = float((ops.slerp(a, b, w).double() - torch_slerp().double()).norm() / torch_slerp().double().norm())
        wins = windows({"fused": lambda: ops.slerp(a, b, w), "torch_fp64": torch_slerp}, 200)
    f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["torch_fp64"])
    emit({"what": "slerp", "pairs": pairs, "weights": W, "row": 3 * 32 * 32, "fused_us": round(f_us, 3), "torch_fp64_us": round(c_us, 3),
          "speedup": round(c_us / f_us, 3), "fused_spread_us": spread(wins["fused"]), "torch_fp64_spread_us": spread(wins["torch_fp64"]),
          "rel_l2_between_them": err})

    # invert + decode against sample
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    n, S = 256, 50
    images = (torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    forms = {"sample": lambda: diff.sample(model, n=n, image_channels=3, steps=S)}
    for refine in (0, 2):
        forms[f"roundtrip_refine{refine}"] = lambda refine=refine: diff.decode(model, diff.invert(model, images, S, refine=refine), S)
    for fn in forms.values():                                 # warm-up (allocator, embedding tables)
        fn()
    secs = {name: [] for name in forms}
    for _ in range(reps):
        for name, fn in forms.items():
            secs[name].append(timed(fn))
    base = statistics.median(secs["sample"])
    emit({"what": "roundtrip", "form": "sample", "n": n, "steps": S, "forwards": S, "seconds": round(base, 4),
          "spread_s": [round(min(secs["sample"]), 4), round(max(secs["sample"]), 4)]})
    for refine in (0, 2):
        v = secs[f"roundtrip_refine{refine}"]
        emit({"what": "roundtrip", "form": "invert+decode", "n": n, "steps": S, "refine": refine, "forwards": (refine + 2) * S,
              "seconds": round(statistics.median(v), 4), "spread_s": [round(min(v), 4), round(max(v), 4)],
              "over_sample": round(statistics.median(v) / base, 3)})

    out_path = arg("--out", "")
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
