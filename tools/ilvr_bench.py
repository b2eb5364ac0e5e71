"""Reference-guided sampling (ILVR) cost, variant 3 at 3 x 32 x 32, factor 4 (L = 2), the default 9 x 9 filter, one MI355X.

    python tools/ilvr_bench.py [--out FILE.json] [--reps 5]

Prints one JSON line per measurement and, with --out, writes them all to FILE.json:
  refine      us per refinement at n = 6 and n = 256 images: the fused launch (`ops.lowpass_refine`, in place) against the
              composition of the existing ops -- `noise_images`, a subtraction, L x `FiltDown2`, L x `FiltUp2`, a scale-add:
              2 L + 3 = 7 launches, with the intermediate tensors they allocate.  HIP events around 1000 back-to-back
              refinements, median of --reps such windows; the two forms alternate window by window so that drift hits both.
              The two results are compared first (rel-L2 in fp64).
  step        ms per step of `Diffusion.ilvr` (every move refined) against ms per step of `Diffusion.sample`, eager, at n = 6
              and n = 256, for the DDPM chain and DDIM S = 50 (eta = 1).  Each figure is the median over --reps whole
              trajectories divided by their forward count; the two samplers alternate.  The DDPM chain is timed with T = 101
              (100 forwards): a step costs what it costs at T = 1000.
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
LEVELS, WINDOW = 2, 1000


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

    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    taps = ops.Taps(afdm.circularLowpassKernel(math.pi / 2, 9, beta=8))

    # the refinement alone
    for n in (6, 256):
        shape = (n, 3, 32, 32)
        g = torch.Generator().manual_seed(n)
        x, ref, z = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
        t_rows = torch.full((n,), 500, device=dev, dtype=torch.long)
        out = torch.empty_like(x)

        def fused():
            return ops.lowpass_refine(x, ref, z, diff.alpha_hat, 500, taps, LEVELS, out=out)

        def composed():
            v = ops.noise_images(ref, z, t_rows, diff.alpha_hat) - x
            for _ in range(LEVELS):
                v = ops.FiltDown2.apply(v, taps)
            for _ in range(LEVELS):
                v = ops.FiltUp2.apply(v, taps)
            return torch.add(x, v, alpha=float(4 ** LEVELS))

        with torch.no_grad():
            a64, b64 = fused().double(), composed().double()
            err = float(((a64 - x.double()) - (b64 - x.double())).norm() / (b64 - x.double()).norm())
            wins = {"fused": [], "composed": []}
            for name, fn in (("fused", fused), ("composed", composed)):
                for _ in range(50):
                    fn()
            for _ in range(reps):
                for name, fn in (("fused", fused), ("composed", composed)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(WINDOW):
                        fn()
                    b.record()
                    b.synchronize()
                    wins[name].append(a.elapsed_time(b) * 1e3 / WINDOW)
        f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["composed"])
        emit({"what": "refine", "n": n, "levels": LEVELS, "N": taps.N, "fused_us": round(f_us, 3), "composed_us": round(c_us, 3),
              "composed_launches": 2 * LEVELS + 3, "speedup": round(c_us / f_us, 3), "fused_spread_us": [round(min(wins["fused"]), 3),
              round(max(wins["fused"]), 3)], "composed_spread_us": [round(min(wins["composed"]), 3), round(max(wins["composed"]), 3)],
              "rel_l2_between_them": err})

    # a sampling step with and without the refinement
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for n in (6, 256):
        reference = torch.rand(n, 3, 32, 32, generator=torch.Generator().manual_seed(0)) * 2 - 1
        for chain in ("ddpm", "ddim50"):
            d = afdm.Diffusion(noise_steps=101 if chain == "ddpm" else 1000, img_size=32, device=dev)
            kw = {} if chain == "ddpm" else {"steps": 50, "eta": 1.0}
            forwards = 100 if chain == "ddpm" else 50
            samp = lambda: d.sample(model, n=n, image_channels=3, **kw)
            ilvr = lambda: d.ilvr(model, reference, factor=2 ** LEVELS, **kw)
            samp(), ilvr()                                    # warm-up (allocator, embedding tables)
            ts, ti = [], []
            for _ in range(reps):
                ts.append(timed(samp))
                ti.append(timed(ilvr))
            s_ms, i_ms = 1e3 * statistics.median(ts) / forwards, 1e3 * statistics.median(ti) / forwards
            emit({"what": "step", "n": n, "chain": chain, "sample_ms": round(s_ms, 4), "ilvr_ms": round(i_ms, 4),
                  "ratio": round(i_ms / s_ms, 4)})

    out_path = arg("--out", "")
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
