"""Attention timing per block (B=256) for rows-per-lane variants (d=8).
`attn_bench.py ab16 [rounds] [codes...]`: sa1 (d = 16, L = 256) under afd_debug_attn_rows 40 / 41 alternating in one
process, sa5 (d = 8, same map) beside it in every round, then the medians."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, afdm, bench
dev = torch.device("cuda:0"); B = 256
L_, s = afdm.lib(), torch.cuda.current_stream().cuda_stream


def _ab16(rounds, codes):
    import statistics
    def block(C):
        qkv = torch.randn(B, 3 * C, 16, 16, device=dev); g = torch.randn(B, C, 16, 16, device=dev); o = torch.empty_like(g)
        lse = torch.empty(B, 4, 256, device=dev); dq = torch.empty_like(qkv); dl = torch.empty_like(lse)
        P = lambda t: t.data_ptr()
        fwd = lambda: L_.afd_attn_fwd(P(qkv), P(o), P(lse), B, 4, C // 4, 256, s)
        bwd = lambda: L_.afd_attn_bwd(P(qkv), P(o), P(g), P(lse), P(dq), P(dl), B, 4, C // 4, 256, s)
        fwd()
        return (qkv, g, o, lse, dq, dl), fwd, bwd
    keep1, f1, b1 = block(64)
    keep5, f5, b5 = block(32)
    T = {}
    for rnd in range(rounds):
        for code in codes:
            L_.afd_debug_attn_rows(code)
            t = [bench.ev_time(f, reps=20, warm=3) * 1e3 for f in (f1, b1, f5, b5)]
            L_.afd_debug_attn_rows(41)
            T.setdefault(code, []).append(t)
            print(f"mode {code} sa1: fwd {t[0]:7.1f} bwd {t[1]:7.1f} us | sa5: fwd {t[2]:7.1f} bwd {t[3]:7.1f} us", flush=True)
    for code in codes:
        m = [statistics.median(r[i] for r in T[code]) for i in range(4)]
        print(f"median {code} sa1: fwd {m[0]:7.1f} bwd {m[1]:7.1f} us | sa5: fwd {m[2]:7.1f} bwd {m[3]:7.1f} us")


if len(sys.argv) > 1 and sys.argv[1] == "ab16":
    _ab16(int(sys.argv[2]) if len(sys.argv) > 2 else 5, [int(c) for c in sys.argv[3:]] or [40, 41])
    sys.exit(0)
for (C, S) in [(32, 32), (32, 16), (64, 16), (128, 8)]:
    Lq = S * S
    qkv = torch.randn(B, 3 * C, S, S, device=dev); o = torch.empty(B, C, S, S, device=dev)
    lse = torch.empty(B, 4, Lq, device=dev); dq = torch.empty_like(qkv); dl = torch.empty_like(lse)
    for r in ((0, 1, 2, 4) if C == 32 else (0,)):
        L_.afd_debug_attn_rows(r)
        tf = bench.ev_time(lambda: L_.afd_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, 4, C // 4, Lq, s), reps=5, warm=1)
        tb = bench.ev_time(lambda: L_.afd_attn_bwd(qkv.data_ptr(), o.data_ptr(), o.data_ptr(), lse.data_ptr(), dq.data_ptr(), dl.data_ptr(), B, 4, C // 4, Lq, s), reps=5, warm=1)
        print(f"C={C} L={Lq} d={C//4} R={r}: fwd {tf*1e3:8.1f} us  bwd {tb*1e3:8.1f} us")
    L_.afd_debug_attn_rows(0)
    if C == 32:
        for f in (10, 11):
            L_.afd_debug_attn_rows(f)
            tb = bench.ev_time(lambda: L_.afd_attn_bwd(qkv.data_ptr(), o.data_ptr(), o.data_ptr(), lse.data_ptr(), dq.data_ptr(), dl.data_ptr(), B, 4, C // 4, Lq, s), reps=5, warm=1)
            print(f"C={C} L={Lq} d={C//4} mfma8 bwd at every L={'on' if f == 11 else 'off'}: bwd {tb*1e3:8.1f} us")
        L_.afd_debug_attn_rows(10)
