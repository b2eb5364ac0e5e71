"""3x3 weight gradient (f16x2 kernel + fold) per Config-D layer shape at B = 256, alone on the chip: the eight-wave plan
(afd_debug_conv_path 51) against four waves wherever covered (52) and the default rule (50), medians over alternating rounds.
  python tools/wgrad_w4_bench.py [rounds]
A launch's time alone does not decide the rule (the step does: tools/step_median.py --lanes, bench.py); this table is what
the rule's choices are read beside."""
import ctypes
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, afdm, bench

dev = torch.device("cuda:0"); B = 256
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
L, s = afdm.lib(), torch.cuda.current_stream().cuda_stream
MODES = ((51, "eight"), (52, "four"), (50, "rule"))
shapes = sorted({t for t in bench.CONV3 if t[0] >= 32}, key=lambda t: (-t[2], t[0], t[1]))
tot = {m: 0.0 for m, _ in MODES}
for (ci, co, S) in shapes:
    x = torch.randn(B, ci, S, S, device=dev); y = torch.randn(B, co, S, S, device=dev); dw = torch.empty(co, ci, 3, 3, device=dev)
    L.afd_debug_conv_path(51)
    ws = torch.empty(L.afd_conv_wgrad_workspace_bytes(B, ci, co, S, S, 3) // 4 + 1, device=dev)      # the eight-wave plan never has fewer slabs
    f = lambda: L.afd_conv_wgrad(x.data_ptr(), y.data_ptr(), dw.data_ptr(), None, B, ci, co, S, S, 3, 0, ws.data_ptr(), s)
    times, plans = {m: [] for m, _ in MODES}, {}
    for r in range(rounds):
        for m, _ in MODES:
            L.afd_debug_conv_path(m)
            info = (ctypes.c_int * 5)()
            plans[m] = (L.afd_conv_wgrad3_plan(B, ci, co, S, S, ctypes.addressof(info)), tuple(info))
            times[m].append(bench.ev_time(f, reps=20) * 1e3)
    n = bench.CONV3.count((ci, co, S))
    line = f"{ci:4d}->{co:4d} @{S:2d}x{S:<2d} x{n}:"
    for m, name in MODES:
        slabs, (tps, nt, bn, bk, nw) = plans[m]
        med = statistics.median(times[m])
        tot[m] += med * n
        line += f"  {name} {bn}x{bk} w{nw} {slabs:3d} slabs {med:6.1f} us"
    print(line, flush=True)
L.afd_debug_conv_path(50)
print("per step: " + "  ".join(f"{name} {tot[m] / 1e3:.3f} ms" for m, name in MODES), flush=True)
