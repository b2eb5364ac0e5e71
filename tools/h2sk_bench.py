"""Per-layer A/B of the split-K small-map convolution: conv_h2_sk everywhere (afd_debug_conv_path 72) against the slice-walking
form conv_h2_skw (csrc/h2.hip) -- by the launch rule (the default, 74) or wherever it is possible (71: `python tools/h2sk_bench.py
256 71`).  Every split-K layer shape of bench.CONV3 at B = 256, forward and dgrad, weights ready, microseconds per launch.  The
two modes alternate in one process; the figures are medians of five rounds."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, afdm, bench
dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
NEW = int(sys.argv[2]) if len(sys.argv) > 2 else 74
L, s = afdm.lib(), torch.cuda.current_stream().cuda_stream
shapes = sorted(set(t for t in bench.CONV3 if t[2] <= 8 and t[0] >= 32), key=lambda t: (t[2], t[0], t[1]))
tot = {72: 0.0, NEW: 0.0}
for (ci, co, S) in shapes:
    cnt = bench.CONV3.count((ci, co, S))
    L.afd_debug_conv_path(74)
    k74 = L.afd_conv3x3_weight_kinds(B, ci, co, S, S)
    L.afd_debug_conv_path(75)
    k75 = L.afd_conv3x3_weight_kinds(B, ci, co, S, S)
    L.afd_debug_conv_path(74)
    sk = k74 ^ k75                                                # bit 0 / 1: the forward / dgrad pass runs the split-K kernel
    if not sk:
        continue
    x = torch.randn(B, ci, S, S, device=dev); w = torch.randn(co, ci, 3, 3, device=dev) * 0.05
    y = torch.randn(B, co, S, S, device=dev); dx = torch.empty_like(x)
    uf, ud = torch.empty(16 * ci * co, device=dev), torch.empty(16 * ci * co, device=dev)
    fwd = lambda ready=1: L.afd_conv3x3_wino_fwd(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), B, ci, co, S, S, 0, uf.data_ptr(), ready, k74, s)
    dgr = lambda ready=1: L.afd_conv3x3_wino_dgrad(y.data_ptr(), w.data_ptr(), dx.data_ptr(), None, B, ci, co, S, S, ud.data_ptr(), ready, k74, s)
    passes = [(n, f) for bit, n, f in ((1, "fwd", fwd), (2, "dgrad", dgr)) if sk & bit]
    for _, f in passes:
        f(0)                                                      # builds the weight image
    t = {(n, m): [] for n, _ in passes for m in (72, NEW)}
    for _ in range(5):
        for m in (72, NEW):
            L.afd_debug_conv_path(m)
            for n, f in passes:
                t[(n, m)].append(bench.ev_time(f, reps=20) * 1e3)
    L.afd_debug_conv_path(74)
    line = f"{ci:4d}->{co:4d} @{S}x{S} x{cnt}:"
    for n, _ in passes:
        a, b = statistics.median(t[(n, 72)]), statistics.median(t[(n, NEW)])
        tot[72] += cnt * a; tot[NEW] += cnt * b
        line += f"  {n} conv_h2_sk {a:6.1f} -> mode {NEW} {b:6.1f} us"
    print(line, flush=True)
print(f"split-K layers per step: conv_h2_sk {tot[72] / 1e3:.3f} ms -> mode {NEW} {tot[NEW] / 1e3:.3f} ms")
