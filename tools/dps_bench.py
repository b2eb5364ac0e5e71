"""Cost of diffusion posterior sampling, variant 3 at 3 x 32 x 32, one MI355X.

    python tools/dps_bench.py [--out FILE.json] [--reps 5]

Prints one JSON line per measurement and, with --out, writes them all to FILE.json.  The operator is a 9 x 9 Gaussian blur
(sigma 2) followed by stride 2, no mask; n = 6 and n = 256 images.
  residual    us per `ops.dps_residual` (x0_hat, r = A x0_hat - y, the planes' fp64 sums of squares and g = A^T r in one launch)
              against the same expressions in torch ops on the device (the per-row coefficients are built once, outside the
              window).  HIP events around 200 back-to-back calls, median of --reps such windows; the two forms alternate window
              by window so that drift hits both.  The two results are compared first (rel-L2 in fp64).
  correct     us per `ops.dps_correct` against the same expression in torch ops, timed the same way.
  step        ms per step of `posterior_sample(steps=20, eta=1)` (whole calls, host clock around a synchronised call, median of
              --reps, divided by 20) against the parts the parent commit already had: ms per step of `sample(steps=20, eta=1)`
              and ms per `TrainStep._fwd_bwd` (a forward and a full backward, weight gradients included) at the same batch.
              frozen / unfrozen: the same DPS call with the parameters frozen during the vector-Jacobian product (what
              `posterior_sample` does) and left as they are (autograd then computes and drops every weight gradient).
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
    import torch.nn.functional as F
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

    def spread(v, digits=3):
        return [round(min(v), digits), round(max(v), digits)]

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    op = afdm.LinearOperator(afdm.gaussian_kernel(9, 2.0), 2)
    K, s, C = op.K, op.stride, 3
    kd = op.kernel.to(dev).expand(C, 1, K, K).contiguous()
    zeta = 1.0

    for n in (6, 256):
        g = torch.Generator().manual_seed(n)
        x_t, out, v = (torch.randn((n, C, 32, 32), generator=g).to(dev) for _ in range(3))
        y = torch.randn((n, C, 16, 16), generator=g).to(dev)
        t = torch.randint(1, 1000, (n,), generator=g).to(dev)
        a, b = (c.float().to(dev).view(-1, 1, 1, 1) for c in diff.x0_coefficients(t))
        gbuf, sums = torch.empty_like(x_t), torch.empty(n, C, device=dev, dtype=torch.float64)

        def fused():
            return ops.dps_residual(x_t, out, t, diff.alpha_hat, "eps", y, op._taps, s, None, gbuf, sums)

        def composed():
            r = F.conv2d(a * x_t + b * out, kd, padding=K // 2, stride=s, groups=C) - y
            return (F.conv_transpose2d(r, kd, padding=K // 2, stride=s, output_padding=s - 1, groups=C),
                    (r.double() * r.double()).flatten(2).sum(-1))

        with torch.no_grad():
            (g1, s1), (g2, s2) = fused(), composed()
            err = {"g": rel(g1, g2), "sums": rel(s1, s2)}
            wins = windows({"fused": fused, "composed": composed}, 200)
        f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["composed"])
        emit({"what": "residual", "n": n, "planes": n * C, "K": K, "stride": s, "fused_us": round(f_us, 3), "composed_us": round(c_us, 3),
              "speedup": round(c_us / f_us, 3), "fused_spread_us": spread(wins["fused"]), "composed_spread_us": spread(wins["composed"]),
              "rel_l2_between_them": err})

        x = torch.randn((n, C, 32, 32), generator=g).to(dev)
        x_keep = x.clone()

        def fused_c():
            return ops.dps_correct(x, gbuf, v, sums, t, diff.alpha_hat, "eps", zeta)

        def composed_c():
            c = (zeta / sums.sum(1).sqrt()).float().view(-1, 1, 1, 1)
            return x_keep - c * (a * gbuf + b * v)

        with torch.no_grad():
            fused()
            err = rel(fused_c(), composed_c())
            # (x runs away over a window of in-place corrections; its values do not change what an elementwise launch costs)
            wins = windows({"fused": fused_c, "composed": composed_c}, 200)
        f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["composed"])
        emit({"what": "correct", "n": n, "fused_us": round(f_us, 3), "composed_us": round(c_us, 3), "speedup": round(c_us / f_us, 3),
              "fused_spread_us": spread(wins["fused"]), "composed_spread_us": spread(wins["composed"]), "rel_l2_between_them": err})

    # a whole DPS step against the parent commit's parts
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)

    class Unfrozen(afdm.Diffusion):
        """`posterior_sample` with the parameters left as they are during the vector-Jacobian product."""

        def _output_and_vjp(self, model, x_t, t, y, seed_fn):
            with torch.enable_grad():
                x = x_t.detach().requires_grad_(True)
                out = self._raw_output(model, x, t, y)
                found = out.detach()
                (v,) = torch.autograd.grad(out, x, seed_fn(found))
            return found, v.contiguous()

    unfrozen = Unfrozen(noise_steps=1000, img_size=32, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    S = 20
    train = afdm.TrainStep(model, diff, lr=3e-4, graph=False)
    for n in (6, 256):
        g = torch.Generator().manual_seed(n)
        images = (torch.rand(n, 3, 32, 32, generator=g) * 2 - 1).to(dev)
        y = op.measure(images, 0.05)
        t = torch.randint(1, 1000, (n,), generator=g).to(dev)
        eps = torch.randn(n, 3, 32, 32, generator=g).to(dev)
        forms = {
            "dps_frozen": (lambda: diff.posterior_sample(model, y, op, zeta=zeta, steps=S, eta=1.0), S),
            "dps_unfrozen": (lambda: unfrozen.posterior_sample(model, y, op, zeta=zeta, steps=S, eta=1.0), S),
            "sample": (lambda: diff.sample(model, n=n, image_channels=3, steps=S, eta=1.0), S),
            "fwd_bwd": (lambda: [train._fwd_bwd(images, t, eps) for _ in range(S)], S),
        }
        for fn, _ in forms.values():                          # warm-up (allocator, embedding tables, weight images)
            fn()
        ms = {name: [] for name in forms}
        for _ in range(reps):
            for name, (fn, calls) in forms.items():
                ms[name].append(timed(fn) * 1e3 / calls)
        med = {name: statistics.median(v) for name, v in ms.items()}
        emit({"what": "step", "n": n, "steps": S, "dps_ms": round(med["dps_frozen"], 3), "dps_unfrozen_ms": round(med["dps_unfrozen"], 3),
              "sample_ms": round(med["sample"], 3), "fwd_bwd_ms": round(med["fwd_bwd"], 3),
              "dps_over_sample_plus_fwd_bwd": round(med["dps_frozen"] / (med["sample"] + med["fwd_bwd"]), 3),
              "unfrozen_over_frozen": round(med["dps_unfrozen"] / med["dps_frozen"], 3),
              "spread_ms": {name: spread(v) for name, v in ms.items()}})

    out_path = arg("--out", "")
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
