"""Cost of the probability-flow ODE likelihood, variant 3 at 3 x 32 x 32, one MI355X.

    python tools/likelihood_bench.py [--out FILE.json] [--reps 5]

Prints one JSON line per measurement and, with --out, writes them all to FILE.json.  n = 6 and n = 256 images, rows of 3072.
  trace_rows  us per `ops.ode_trace_rows` (both row sums in fp64 and the update of the accumulator, one launch) against
              `acc += cvv * (v.double() * v.double()).flatten(1).sum(1) + cvw * (v.double() * w.double()).flatten(1).sum(1)` in torch
              ops on the device.  HIP events around 1000 back-to-back calls, median of --reps such windows; the two forms alternate
              window by window so that drift hits both.  The two results are compared first (rel-L2 in fp64).
  heun_step   us per `ops.ode_heun_step` against its expression in torch ops, timed the same way.
  move        ms per Heun move of `ode_likelihood(steps=11, P = 1)` (whole calls, host clock around a synchronised call, median of
              --reps; the 10 Heun moves are the call minus an Euler-only call's share of the first move: (heun - euler / 11) / 10)
              against two steps of `posterior_sample(steps=20, eta=1)`, each one forward and one backward with the parameters
              frozen, as tools/dps_bench.py times them, on the same box in the same run.
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

    def spread(v, digits=3):
        return [round(min(v), digits), round(max(v), digits)]

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())

    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    ah = diff.alpha_hat.detach().cpu().double()
    cvv, cvw = 0.01, -0.37
    s, u = 300, 400
    a_s, a_u = float(ah[s]), float(ah[u])
    h = math.sqrt((1 - a_u) / a_u) - math.sqrt((1 - a_s) / a_s)

    for n in (6, 256):
        g = torch.Generator().manual_seed(n)
        v, w, x, es, eu = (torch.randn((n, 3, 32, 32), generator=g).to(dev) for _ in range(5))
        acc_f = torch.zeros(n, device=dev, dtype=torch.float64)
        acc_c = torch.zeros(n, device=dev, dtype=torch.float64)

        def fused():
            return ops.ode_trace_rows(v, w, cvv, cvw, acc_f)

        def composed():
            vd = v.double()
            acc_c.add_(cvv * (vd * vd).flatten(1).sum(1) + cvw * (vd * w.double()).flatten(1).sum(1))
            return acc_c

        with torch.no_grad():
            err = rel(fused(), composed())
            wins = windows({"fused": fused, "composed": composed}, 1000)
        f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["composed"])
        emit({"what": "trace_rows", "rows": n, "per": 3072, "fused_us": round(f_us, 3), "composed_us": round(c_us, 3),
              "speedup": round(c_us / f_us, 3), "fused_spread_us": spread(wins["fused"]), "composed_spread_us": spread(wins["composed"]),
              "rel_l2_between_them": err})

        out = torch.empty_like(x)

        def fused_h():
            return ops.ode_heun_step(x, es, eu, diff.alpha_hat, s, u, out)

        def composed_h():
            return math.sqrt(a_u) * (x / math.sqrt(a_s) + (0.5 * h) * (es + eu))

        with torch.no_grad():
            err = rel(fused_h(), composed_h())
            wins = windows({"fused": fused_h, "composed": composed_h}, 1000)
        f_us, c_us = statistics.median(wins["fused"]), statistics.median(wins["composed"])
        emit({"what": "heun_step", "n": n, "fused_us": round(f_us, 3), "composed_us": round(c_us, 3), "speedup": round(c_us / f_us, 3),
              "fused_spread_us": spread(wins["fused"]), "composed_spread_us": spread(wins["composed"]), "rel_l2_between_them": err})

    # a whole Heun move against two DPS steps
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    op = afdm.LinearOperator(afdm.gaussian_kernel(9, 2.0), 2)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    S, D = 11, 20
    for n in (6, 256):
        g = torch.Generator().manual_seed(n)
        images = (torch.rand(n, 3, 32, 32, generator=g) * 2 - 1).to(dev)
        y = op.measure(images, 0.05)
        forms = {
            "heun": lambda: diff.ode_likelihood(model, images, S, method="heun"),
            "euler": lambda: diff.ode_likelihood(model, images, S, method="euler"),
            "dps": lambda: diff.posterior_sample(model, y, op, zeta=1.0, steps=D, eta=1.0),
        }
        for fn in forms.values():                              # warm-up (allocator, embedding tables, weight images)
            fn()
        ms = {name: [] for name in forms}
        for _ in range(reps):
            for name, fn in forms.items():
                ms[name].append(timed(fn) * 1e3)
        med = {name: statistics.median(vals) for name, vals in ms.items()}
        euler_move = med["euler"] / S
        heun_move = (med["heun"] - euler_move) / (S - 1)
        dps_step = med["dps"] / D
        emit({"what": "move", "n": n, "probes": 1, "heun_move_ms": round(heun_move, 3), "euler_move_ms": round(euler_move, 3),
              "dps_step_ms": round(dps_step, 3), "heun_move_over_two_dps_steps": round(heun_move / (2 * dps_step), 3),
              "call_ms": {name: round(val, 3) for name, val in med.items()}, "call_spread_ms": {name: spread(vals) for name, vals in ms.items()}})

    out_path = arg("--out", "")
    if out_path:
        with open(out_path, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
