"""Case tables, fp64 references and slice helpers of tests/test_gpu_unet64_ops.py: the kernels and launcher branches that only
the default UNet(image_size=64) reaches.  Needs no device: tests/test_unet64_cases_host.py runs every case in plain CPU fp32
under the gates the GPU test uses, checks that the tables cover the 64 model's layers and that the gates reject the faults
that live at these shapes (a halo row from the next image, a stale last row band, a key tile dropped).

Gates: the project's contract, rel-L2 < 1e-5 against fp64 on the whole tensor (TOL).  Convolution sections A, B and D add
slice checks (per image, border ring, interior, last two-row band on 64-wide maps; slices of >= 1024 elements only) gated at
max(TOL, 2 x the error of plain CPU fp32 torch on that very slice): never derived from a kernel's output."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import ref_ops as R

TOL = 1e-5
MIN_SLICE = 1024


def rel_l2(a, b):
    a = torch.as_tensor(a, dtype=torch.float64).flatten()
    b = torch.as_tensor(b, dtype=torch.float64).flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------
# convolution tables: (B, Cin, Cout, H, W, k, bias, res); `paths` are names of PATH_MODES (those of test_conv_fwd_dgrad_wgrad)
# ---------------------------------------------------------------------------------------------------------------------------
PATH_MODES = {"auto": 0, "big": 1, "splitk": 2, "wgrad4": 32, "wgrad8": 33, "pw": 10, "bf3": 82, "nobf3": 81, "h2reg": (82, 61),
              "h2l64": (82, 62), "h2l256": (82, 63), "h2l32": (82, 59), "h2sk": 73, "wgbf3": 86, "nowgbf3": 85, "noends": 93,
              "wino64x64": 66, "wino32x64": 67, "wino64x32": 68, "wino32x32": 69, "winosk": 70, "nowino": 65, "wgwino": 98,
              "nowgwino": 97}
PATH_RESTORE = (0, 34, 8, 80, 60, 74, 84, 92, 64, 96)          # the `finally` of test_conv_fwd_dgrad_wgrad, in its order
WINO4 = ("wino64x64", "wino32x64", "wino64x32", "wino32x32")

ConvCase = namedtuple("ConvCase", "section case paths ramps why")


def _cc(section, case, paths, why, ramps=False):
    if len(case) == 5:
        case = case + (3, False, False)
    return ConvCase(section, tuple(case), tuple(paths), ramps, why)


_A_FULL = ("auto", "big", "splitk") + WINO4 + ("nowino", "wgrad4", "wgrad8")
# Section B, the forced paths of the existing list whose predicate admits these shapes (square maps of 8 / 16 / 32, channels
# multiples of 64); the GPU test asserts each through the query entry points (kinds = afd_conv3x3_weight_kinds, nb / nd =
# afd_conv3x3_wino_workspace_bytes forward / dgrad, wf = afd_conv_wgrad_form):
#   big / splitk (launch_mfma, conv.hip:866-867): read whenever the layer is on the fp32 tile kernels, which at these batch sizes
#     is the rule's own choice: nb == nd == 0, and the form restated by mfma_form;
#   bf3 / h2reg / h2l64 / h2l256 / h2l32 (direct_plan, bf3.hip:247-250: W in {8,16,32}, K % 32 == N % 32 == 0): kinds & 1 and
#     kinds & 2; which f16x2 kernel by h2_form below;  nobf3: kinds == 0;
#   h2sk (h2_sk_ok, h2.hip:992) and winosk (wino.hip:541) admit W <= 8 only: the 8x8 cases;
#   the four forced Winograd shapes and winosk (wino_plan, wino.hip:529-541: K % 8 == 0, N % 32 == 0): nb, nd != 0, kinds == 0;
#     nowino: nb == nd == 0;
#   wgbf3 (wgrad_plan_full, bf3_wgrad.hip:568-569): wf in (2, 4);  nowgbf3: wf == 1, the Winograd weight gradient by its rule;
#   nowgwino: wf != 1;  nowgbf3+wgwino (85 and 98 together): wf == 1, the Winograd weight gradient forced.
# Not admitted: pw and noends (1x1 layers only); wgrad4 / wgrad8 select the waves of conv_wgrad_mfma, which these shapes never
# reach through ops.conv; wgwino (98) alone: conv_wgrad_impl tries wgrad_h2 before wgrad_wino (conv.hip:1130-1132) and
# wgrad_plan_full takes every one of these shapes by rule (nt * blocks >= 128, bf3_wgrad.hip:592), so 98 alone is a second run
# of auto; it runs paired with 85.
PATH_MODES["nowgbf3+wgwino"] = (85, 98)
_B_ALL = ("auto", "big", "splitk", "bf3", "nobf3", "h2reg", "h2l64", "h2l256", "h2l32", "wgbf3", "nowgbf3") + WINO4 + \
         ("nowino", "nowgbf3+wgwino", "nowgwino")
_B_8 = _B_ALL + ("h2sk", "winosk")

CONV_CASES = [
    # ---- A: 3x3 at 64x64 (and the 2x2 map that also needs NPB = 8)
    _cc("A", (3, 64, 64, 64, 64, 3, False, False), _A_FULL, "by rule at B = 3 the split-K tile; big = conv_mfma GEO 0, BN 64"),
    _cc("A", (5, 64, 96, 64, 64, 3, True, True), _A_FULL, "odd batch, N % 64 != 0, epilogue"),
    _cc("A", (2, 128, 64, 64, 64, 3, True, True), ("auto", "big") + WINO4, "up3"),
    _cc("A", (3, 8, 32, 64, 64, 3, False, False), ("auto", "big", "nowino"), "one K chunk, BN 32"),
    _cc("A", (2, 3, 64, 64, 64, 3, False, False), ("auto",), "inc.conv1: ragged-chunk forward, wgrad_cin3<64>"),
    _cc("A", (16, 64, 64, 64, 64, 3, False, False), ("auto",), "the rule picks Winograd from B = 16"),
    _cc("A", (2, 64, 64, 64, 64), ("wgrad4", "wgrad8"), "NPB = 8 roles WNn 2, WCn 2"),
    _cc("A", (2, 16, 64, 64, 64), ("wgrad4", "wgrad8"), "NPB = 8 roles WNn 2, WCn 1"),
    _cc("A", (2, 64, 32, 64, 64), ("wgrad4", "wgrad8"), "NPB = 8 roles WNn 1, WCn 2"),
    _cc("A", (2, 16, 32, 64, 64), ("wgrad4", "wgrad8"), "NPB = 8 roles WNn 1, WCn 1"),
    _cc("A", (9, 64, 64, 2, 2, 3, False, False), ("auto", "wgrad4", "wgrad8"), "NPB = 8 by whole images, ragged last tile"),
    _cc("A", (2, 128, 128, 64, 64), ("auto", "big"), "up3's residual pair (the one 64x64 layer shape of the model not listed above)"),
    # ---- B: the wide layers
    _cc("B", (3, 256, 512, 8, 8), _B_8, "bot1"),
    _cc("B", (3, 512, 512, 8, 8), _B_8, "bot1 / bot2"),
    _cc("B", (3, 512, 256, 8, 8), _B_8, "bot3"),
    _cc("B", (2, 512, 512, 16, 16), _B_ALL, "up1"),
    _cc("B", (2, 512, 256, 16, 16), _B_ALL, "up1"),
    _cc("B", (2, 256, 256, 32, 32), _B_ALL, "up2"),
    _cc("B", (2, 256, 128, 32, 32), _B_ALL, "up2"),
    # ---- B2: the model's remaining 3x3 layer shapes (maps <= 32, <= 256 channels), at the small batch, by rule
    _cc("B2", (2, 64, 64, 32, 32), ("auto",), "down1"),
    _cc("B2", (2, 64, 128, 32, 32), ("auto",), "down1"),
    _cc("B2", (2, 128, 128, 32, 32), ("auto",), "down1"),
    _cc("B2", (2, 128, 64, 32, 32), ("auto",), "up2"),
    _cc("B2", (2, 128, 128, 16, 16), ("auto",), "down2"),
    _cc("B2", (2, 128, 256, 16, 16), ("auto",), "down2"),
    _cc("B2", (2, 256, 256, 16, 16), ("auto",), "down2"),
    _cc("B2", (2, 256, 128, 16, 16), ("auto",), "up1"),
    _cc("B2", (3, 256, 256, 8, 8), ("auto",), "down3 / bot3"),
    # ---- C: 1x1 (pw: the streaming kernel forced, which pw_launch admits up to K = 64 only, pw.hip:113)
    _cc("C", (2, 256, 768, 16, 16, 1, True, False), ("auto",), "sa2 in_proj (unfused: tok_ok is false at 256)"),
    _cc("C", (3, 256, 256, 8, 8, 1, True, True), ("auto",), "sa3 out_proj / FF + residual"),
    _cc("C", (3, 256, 768, 8, 8, 1, True, False), ("auto",), "sa3 in_proj (the one 1x1 shape of the model not in the list above)"),
    _cc("C", (2, 256, 256, 16, 16, 1, True, True), ("auto",), "sa2 out_proj / FF + residual"),
    _cc("C", (2, 128, 384, 32, 32, 1, True, False), ("auto",), "sa1 in_proj"),
    _cc("C", (1, 64, 192, 64, 64, 1, True, False), ("auto", "pw"), "sa6 in_proj"),
    _cc("C", (2, 64, 3, 64, 64, 1, True, False), ("auto", "pw", "noends"), "outc: the streaming ends kernels"),
    # ---- D: non-square tile_ok maps (run-time geometry with H and W in different roles); inputs carry row and column ramps
    _cc("D", (3, 32, 64, 8, 16), ("auto", "big", "splitk", "wgrad4", "wgrad8"), "two images per 128-pixel tile", ramps=True),
    _cc("D", (3, 32, 64, 16, 8), ("auto", "big", "splitk", "wgrad4", "wgrad8"), "the same, transposed", ramps=True),
    _cc("D", (2, 64, 32, 32, 16), ("auto", "big", "splitk", "wgrad4", "wgrad8"), "eight rows of 16 per tile", ramps=True),
    _cc("D", (5, 64, 64, 4, 8), ("auto", "big", "splitk", "wgrad4", "wgrad8"), "four images per tile, ragged last tile", ramps=True),
]


def conv_id(cc):
    c = cc.case
    return f"{cc.section}_B{c[0]}_{c[1]}to{c[2]}_{c[3]}x{c[4]}_k{c[5]}" + ("_b" if c[6] else "") + ("_r" if c[7] else "")


def conv_inputs(cc):
    B, Cin, Cout, H, W, ks, has_bias, has_res = cc.case
    g = _g(B * 1000 + Cin + Cout + H + 7 * W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / math.sqrt(Cin * ks * ks)
    bias = torch.randn(Cout, generator=g) if has_bias else None
    res = torch.randn(B, Cout, H, W, generator=g) if has_res else None
    dy = torch.randn(B, Cout, H, W, generator=g)
    dr = torch.randn(B, Cin, H, W, generator=g)
    if cc.ramps:                                          # an H / W swap moves these: a row ramp and a (different) column ramp
        r, c = torch.linspace(-1, 1, H)[:, None], torch.linspace(-1, 1, W)[None, :]
        x = x + 0.7 * r - 0.4 * c * c
        dy = dy - 0.5 * r * r + 0.6 * c
    return {"x": x, "w": w, "bias": bias, "res": res, "dy": dy, "dr": dr}


def conv_has_fork(cc):
    return cc.case[5] == 3 and not cc.case[6] and not cc.case[7]         # as _conv_case of test_gpu_ops.py


def conv_torch(cc, inp, dtype, fwd=None):
    """The outputs the GPU test compares, by plain torch on the CPU in `dtype`: y, dx, dw, [db], [dres], [dx_fork], y_gelu.
    `fwd(x, w, bias)` replaces the convolution itself (the perturbed references)."""
    ks = cc.case[5]
    fwd = fwd or (lambda x, w, b: F.conv2d(x, w, b, padding=ks // 2))
    t = {k: (None if v is None else v.to(dtype)) for k, v in inp.items()}
    leaves = {k: t[k].clone().requires_grad_(True) for k in ("x", "w", "bias", "res") if t[k] is not None}
    y = fwd(leaves["x"], leaves["w"], leaves.get("bias"))
    if "res" in leaves:
        y = y + leaves["res"]
    names = list(leaves)
    grads = torch.autograd.grad(y, [leaves[k] for k in names], t["dy"])
    out = {"y": y.detach()}
    for k, gr in zip(names, grads):
        out["d" + {"bias": "b"}.get(k, k)] = gr
    if conv_has_fork(cc):
        out["dx_fork"] = out["dx"] + t["dr"]
    with torch.no_grad():
        z = R.gelu_erf(fwd(t["x"], t["w"], t["bias"]))
        out["y_gelu"] = z + t["res"] if t["res"] is not None else z
    return out


SPATIAL = ("y", "dx", "dx_fork", "y_gelu")


def spatial_slices(shape):
    """[(name, fn)] for a (B, C, H, W) tensor; fn(t) -> the slice's elements.  Only slices of >= MIN_SLICE elements."""
    B, C, H, W = shape
    out = []
    ring = torch.zeros(H, W, dtype=torch.bool)
    ring[0, :] = ring[-1, :] = True
    ring[:, 0] = ring[:, -1] = True
    cand = [(f"image {b}", (lambda t, b=b: t[b]), C * H * W) for b in range(B)]
    cand.append(("border ring", (lambda t: t[:, :, ring]), B * C * int(ring.sum())))
    if H > 2 and W > 2:
        cand.append(("interior", (lambda t: t[:, :, ~ring]), B * C * int((~ring).sum())))
    if W == 64 and H >= 4:
        cand.append(("last row band", (lambda t: t[:, :, H - 2:]), B * C * 2 * W))
        cand += [(f"last row band of image {b}", (lambda t, b=b: t[b, :, H - 2:]), C * 2 * W) for b in range(B)]
    return [(n, f) for n, f, cnt in cand if cnt >= MIN_SLICE]


_CONV_REF = {}


def conv_ref(cc):
    """(inputs, fp64 outputs, gates): computed once per case and shared (never modified).  gates[(output, slice)] is the slice gate,
    max(TOL, 2 x plain CPU fp32's error on that slice); the whole-tensor gate is TOL.  fp32[(output, None | slice)] keeps the fp32
    errors themselves for the host test's record."""
    key = conv_id(cc)
    if key not in _CONV_REF:
        if len(_CONV_REF) >= 2:                          # the references are large: keep the last two
            _CONV_REF.pop(next(iter(_CONV_REF)))
        inp = conv_inputs(cc)
        r64, r32 = conv_torch(cc, inp, torch.float64), conv_torch(cc, inp, torch.float32)
        gates, fp32 = {}, {}
        for k in r64:
            fp32[(k, None)] = rel_l2(r32[k], r64[k])
            if k in SPATIAL and cc.section in ("A", "B", "D"):
                for name, fn in spatial_slices(r64[k].shape):
                    e = rel_l2(fn(r32[k]), fn(r64[k]))
                    fp32[(k, name)] = e
                    gates[(k, name)] = max(TOL, 2.0 * e)
        _CONV_REF[key] = (inp, r64, gates, fp32)
    return _CONV_REF[key]


def conv_checks(cc, got, r64, gates):
    """[(output, slice or None, error, gate)] of a set of outputs against the reference: every whole tensor at TOL, then the slices."""
    res = []
    for k, want in r64.items():
        res.append((k, None, rel_l2(got[k], want), TOL))
        if k in SPATIAL and cc.section in ("A", "B", "D"):
            for name, fn in spatial_slices(want.shape):
                res.append((k, name, rel_l2(fn(got[k]), fn(want)), gates[(k, name)]))
    return res


# ---- the launchers' own rules, restated (no query entry point reports them) ------------------------------------------------------
def tile_ok(H, W, PT):                                   # conv.hip:162-165
    return ((H * W) % PT == 0 and PT % W == 0) or PT % (H * W) == 0


def geom_xs(H, W, PT, halo):                             # make_geom, conv.hip:166-174
    HW = H * W
    TI, TR = (1, PT // W) if HW >= PT else (PT // HW, H)
    return TI * (TR + 2 * halo) * (W + 2 * halo)


def wgrad_npb(H, W):                                     # wgrad_plan, conv.hip:919-921
    need = (geom_xs(H, W, 64, 1) + 31) // 32
    return 4 if need <= 4 else (5 if need <= 5 else 8)


def h2_form(path, B, N, S):
    """The f16x2 kernel h2_conv picks under a forced path (h2.hip:1018-1023,1030,1042; afd_debug_conv_path 59 ... 63 set g_h2_lds)."""
    if path == "h2sk":
        return f"conv_h2_sk / _skw<{S}> (split-K)"
    lds = {"h2reg": 0, "h2l64": 2, "h2l256": 3, "h2l32": 4}.get(path, 1)           # 1: by rule (bf3 = the direct form wherever covered)
    if not (lds > 1 or (lds == 1 and S == 32 and N % 64 != 0)):
        return f"conv_h2<{S}> (register-fed)"
    px = B * S * S
    if lds != 4 and N % 64 == 0 and (lds == 2 or (lds == 1 and ((px + 127) // 128) * (N // 64) >= 512)):
        return f"conv_h2l<{S}, 128 px, 2 blocks>"
    if S >= 16 and (lds == 3 or (lds == 1 and ((px + 255) // 256) * (N // 32) >= 512)):
        return f"conv_h2l<{S}, 256 px, 1 block>"
    return f"conv_h2l<{S}, 128 px, 1 block>"


def wgrad_waves(B, Cin, Cout, H, W):                     # wgrad_plan + launch_wgrad, conv.hip:905-917,930 (default target 256)
    wnn, wcn = (2 if Cout > 32 else 1), (2 if Cin > 32 else 1)
    nchunks = (B * H * W + 63) // 64
    tiles = ((Cout + 32 * wnn - 1) // (32 * wnn)) * ((Cin + 32 * wcn - 1) // (32 * wcn))
    s = min(max(256 // tiles, 1), nchunks)
    cps = (nchunks + s - 1) // s
    return 8 if (cps >= 8 or (cps >= 4 and H * W >= 256)) else 4


def mfma_form(B, K, N, H, W, T, path):
    """The kernel launch_mfma<T> picks (conv.hip:855-897) for reduction width K and N output channels, or the direct kernel
    (use_mfma, conv.hip:850, and the XS limit, conv.hip:881)."""
    if N < 8 or not tile_ok(H, W, 128):
        return "conv_direct"
    ptiles = (B * H * W + 127) // 128
    wgs64, wgs32 = ptiles * ((N + 63) // 64), ptiles * ((N + 31) // 32)
    mode = {"big": 1, "splitk": 2}.get(path, 0)
    use32 = N <= 32 or (wgs64 < 256 and wgs32 >= 256)
    if mode == 1:
        use32 = N <= 32
    want_sk = mode == 2 or (mode == 0 and wgs64 < 256 and wgs32 < 256)
    if want_sk and K >= 32 and tile_ok(H, W, 64) and geom_xs(H, W, 64, 1 if T == 9 else 0) <= 256:
        return "conv_mfma_sk"
    if geom_xs(H, W, 128, 1 if T == 9 else 0) > 512:
        return "conv_direct"
    geo = 5 if T == 1 else ({32: 1, 16: 2, 8: 3, 4: 4}.get(W, 0) if H == W else 0)
    return f"conv_mfma<BN {32 if use32 else 64}, GEO {geo}>"


# ---------------------------------------------------------------------------------------------------------------------------
# E: norms
# ---------------------------------------------------------------------------------------------------------------------------
GN_MODES = ("plain", "res_gelu", "emb", "gelu")
# (shape, misaligned): every one has n = C*H*W > 65536 -> gn_fwd_loop (norm.hip:534,544) and, n > 32768, the plane + apply
# backward (norm.hip:564,580-584) with min(64, ceil(n / 8192)) slices
GN_CASES = [((2, 17, 64, 64), False),      # just past the register path: 9 slices
            ((2, 64, 64, 64), False),      # 32 slices
            ((1, 128, 64, 64), False),     # exactly 64 slices
            ((2, 129, 64, 64), False),     # 65 -> the cap at 64
            ((1, 64, 128, 128), False),    # variant 4's sandwich on the 2x grid
            ((2, 3, 65, 65), False),       # HW % 4 != 0: no vector path in the apply pass; 12675 elements = twelve + loop trips of 1024 threads
            ((2, 64, 64, 64), True),       # x (and res) as views 4 bytes past a 16-byte boundary
            ((1, 256, 32, 32), False),     # up2 and
            ((1, 512, 16, 16), False)]     # up1: the model's two other (C, S) sites with n > 65536
GNFA_CASES = [(2, 64, 64, 64), (1, 128, 32, 32), (2, 256, 16, 16), (2, 512, 8, 8)]
# pixels = B*H*W: >= 32768 -> ln_c_fwd_reg<C> and the SPLIT 4 backward, >= 8192 -> SPLIT 8 (norm.hip:597-598,623); C = 256 is
# the generic ln_c_fwd / ln_c_bwd_dx (norm.hip:603,628)
LN_CASES = [((5, 256, 16, 16), "generic, five workgroups"), ((3, 256, 8, 8), "generic, one partly live workgroup"),
            ((8, 64, 32, 32), "split<64, 8>"), ((8, 64, 64, 64), "fwd_reg<64> / bwd split<64, 4>"),
            ((32, 32, 32, 32), "fwd_reg<32> / bwd split<32, 4>"), ((9, 128, 64, 64), "fwd_reg<128> / bwd split<128, 4>")]


def gn_inputs(shape, mode):
    B, C, H, W = shape
    g = _g(sum(shape) + GN_MODES.index(mode))
    t = {"x": torch.randn(shape, generator=g) * 1.7 + 0.3, "gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g)}
    if mode == "res_gelu":
        t["res"] = torch.randn(shape, generator=g)
    if mode == "emb":
        t["emb"] = torch.randn(B, C, generator=g)
    t["dy"] = torch.randn(shape, generator=g)
    return t


def gn_torch(inp, mode, dtype):
    """-> (y, {name: gradient}) of act(GroupNorm(1, C)(x) gamma + beta + res) + emb."""
    names = [k for k in ("x", "gamma", "beta", "res", "emb") if k in inp]
    lv = {k: inp[k].to(dtype).requires_grad_(True) for k in names}
    z = R.groupnorm1(lv["x"], lv["gamma"], lv["beta"])
    if "res" in lv:
        z = z + lv["res"]
    if mode in ("res_gelu", "gelu"):
        z = R.gelu_erf(z)
    if "emb" in lv:
        z = z + lv["emb"][:, :, None, None]
    grads = torch.autograd.grad(z, [lv[k] for k in names], inp["dy"].to(dtype))
    return z.detach(), dict(zip(names, grads))


def gnfa_inputs(shape, with_res):
    B, C, H, W = shape
    g = _g(11 + sum(shape))
    t = {"x": torch.randn(shape, generator=g) * 2 + 0.5, "gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g)}
    if with_res:
        t["res"] = torch.randn(shape, generator=g)
    t["dy"] = torch.randn(shape, generator=g)
    return t


def filt_kernels():
    return R.lowpass_kernel(math.pi / 2, 3, 2), R.lowpass_kernel(math.pi / 2, 3, 2)


def gnfa_torch(inp, dtype):
    ku, kd = filt_kernels()
    names = [k for k in ("x", "gamma", "beta", "res") if k in inp]
    lv = {k: inp[k].to(dtype).requires_grad_(True) for k in names}
    z = R.groupnorm1(lv["x"], lv["gamma"], lv["beta"])
    if "res" in lv:
        z = z + lv["res"]
    y = R.filt_act(z, ku.to(dtype), kd.to(dtype))
    grads = torch.autograd.grad(y, [lv[k] for k in names], inp["dy"].to(dtype))
    return y.detach(), dict(zip(names, grads))


def ln_inputs(shape):
    B, C, H, W = shape
    g = _g(C + B + H)
    return {"x": torch.randn(shape, generator=g) * 3 + 1, "gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g),
            "dy": torch.randn(shape, generator=g), "dr": torch.randn(shape, generator=g)}


def ln_torch(inp, dtype):
    """-> (y, grads of y . dy, grads of y . dy + x . dr): the two backward legs of test_layernorm_c."""
    shape = inp["x"].shape
    B, C, H, W = shape
    lv = [inp[k].to(dtype).requires_grad_(True) for k in ("x", "gamma", "beta")]
    tok = lv[0].reshape(B, C, H * W).transpose(1, 2)
    y = F.layer_norm(tok, (C,), lv[1], lv[2]).transpose(1, 2).reshape(shape)
    dy, dr = inp["dy"].to(dtype), inp["dr"].to(dtype)
    g1 = torch.autograd.grad(y, lv, dy, retain_graph=True)
    g2 = torch.autograd.grad((y * dy).sum() + (lv[0] * dr).sum(), lv)
    return y.detach(), g1, g2


# ---------------------------------------------------------------------------------------------------------------------------
# F: attention core (B, heads, d, L); G: the attention block (B, C, S); H: one whole step
# ---------------------------------------------------------------------------------------------------------------------------
# forms (attn.hip:382-400,412-446): d = 16 and L % 256 == 0 -> the matrix-core attn_fwd_pv<16> / attn_bwd_fused<16>; d = 32,
# L > 64 -> launch_fwd/dq<32, 2> (+ dkv<32, 1>); d = 64 -> <64, 1>, at L = 64 below the attn_small kernels' d range; d = 2, 4 ->
# <2, 4>, <4, 4>
ATTN_CASES = [(1, 1, 16, 4096), (2, 2, 16, 1024), (1, 2, 32, 1024), (2, 2, 32, 256), (3, 2, 32, 320), (2, 2, 64, 256), (3, 4, 64, 64),
              (1, 2, 64, 320), (2, 3, 2, 100), (2, 3, 4, 100)]
ATTN_VARIANTS = ATTN_CASES[:4]                           # these also run peaked-softmax and row-shift inputs
BLOCK_CASES = [(1, 128, 32), (2, 128, 16), (2, 64, 32)]  # fused chain against the fp64 oracle and the unfused path
BLOCK_UNFUSED_ONLY = [(1, 64, 64)]                       # its fp64 oracle needs several GB on the host: fused against unfused at 5e-6
STEP_CASES = [(3, 3), (0, 3)]                            # (variant, B) at image_size 64


def attn_form(d, L):
    if d == 16 and L % 256 == 0:
        return "attn_fwd_pv<16> + attn_bwd_fused<16>"
    if d in (16, 32) and L <= 64:
        return "attn_small"
    return {2: "fwd/dq/dkv<2, 4>", 4: "fwd/dq/dkv<4, 4>", 16: "fwd/dq/dkv<16, 2>", 32: "fwd/dq<32, 2> + dkv<32, 1>", 64: "fwd/dq/dkv<64, 1>"}[d]


def attn_inputs(cfg, variant="base"):
    B, heads, d, L = cfg
    C = heads * d
    g = _g(L + d + {"base": 0, "peaked": 77, "row shift": 78}[variant])
    qkv, dy = torch.randn(B, 3 * C, L, generator=g), torch.randn(B, C, L, generator=g)
    if variant == "peaked":                              # test_d16_peaked_softmax: one late key x 40, Q x 3
        qkv[:, C:2 * C, (25 * L) // 32] *= 40.0
        qkv[:, :C, :] *= 3.0
    if variant == "row shift":                           # test_d16_row_shift: every score of every row moves by exactly +30
        qkv[:, 0:C:d, :] = 1.0
        qkv[:, C:2 * C:d, :] += 30.0 * math.sqrt(d)
    return qkv, dy


def attn_torch(cfg, qkv, dy, dtype, drop_last_keys=0):
    """-> o (B, C, L), lse (B, heads, L), dqkv (B, 3C, L).  drop_last_keys: the perturbed reference (a key tile never read)."""
    B, heads, d, L = cfg
    C = heads * d
    q0 = qkv.to(dtype).requires_grad_(True)
    q, k, v = q0.split(C, dim=1)
    sh = lambda z: z.reshape(B, heads, d, L).transpose(2, 3)
    s = sh(q) @ sh(k).transpose(-1, -2) / math.sqrt(d)
    vv = sh(v)
    if drop_last_keys:
        s, vv = s[..., :L - drop_last_keys], vv[:, :, :L - drop_last_keys]
    o = (torch.softmax(s, dim=-1) @ vv).transpose(2, 3).reshape(B, C, L)
    (g,) = torch.autograd.grad(o, q0, dy.to(dtype))
    return o.detach(), torch.logsumexp(s, dim=-1).detach(), g


def block_state(case):
    """Seeded SelfAttention(C, S) parameters off their trivial init, input and output gradient (as TOK_CASES' test)."""
    import afdm
    B, C, S = case
    g = _g(1000 + B + C + S)
    torch.manual_seed(5 + C + S)
    mod = afdm.SelfAttention(C, S)
    with torch.no_grad():
        for q in mod.parameters():
            q.add_(0.1 * torch.randn(q.shape, generator=g))
    x, dy = torch.randn(B, C, S, S, generator=g), torch.randn(B, C, S, S, generator=g)
    return mod, x, dy


def block_torch(sd, x, dy, dtype):
    sdt = {k: v.detach().to(dtype).requires_grad_(True) for k, v in sd.items()}
    xt = x.to(dtype).requires_grad_(True)
    y = R.self_attention(sdt, "", xt)
    names = list(sdt)
    grads = torch.autograd.grad(y, [xt] + [sdt[k] for k in names], dy.to(dtype))
    return y.detach(), dict(zip(["x"] + names, grads))


# ---------------------------------------------------------------------------------------------------------------------------
# what UNet(image_size=64) launches
# ---------------------------------------------------------------------------------------------------------------------------
def stage_sizes(net):
    """Map size of every stage, read from the model: the image size at inc / outc / up3's output, and behind each resampling stage
    the size its SelfAttention was built for (unet.py:45-61: sa1 ... sa6 follow down1, down2, down3, up1, up2, up3; bot1-3 stay on
    down3's map)."""
    s = {"inc": net.image_size, "outc": net.image_size}
    for stage, sa in (("down1", net.sa1), ("down2", net.sa2), ("down3", net.sa3), ("up1", net.sa4), ("up2", net.sa5), ("up3", net.sa6)):
        s[stage] = sa.size
    for b in ("bot1", "bot2", "bot3"):
        s[b] = net.sa3.size
    assert s["up3"] == net.image_size and [s[k] for k in ("down1", "down2", "down3")] == [net.image_size // d for d in (2, 4, 8)]
    assert [s[k] for k in ("up1", "up2")] == [net.image_size // 4, net.image_size // 2]
    return s


def model_shapes(net):
    """-> conv3 {(Cin, Cout, S)}, conv1 {(Cin, Cout, S)}, gn {(C, S)}, ln {(C, S)}, sa {(C, S)} of a UNet."""
    import afdm
    size = stage_sizes(net)
    conv3, conv1, gn, ln, sa = set(), set(), set(), set(), set()
    for name, m in net.named_modules():
        stage = name.split(".")[0]
        if isinstance(m, torch.nn.Conv2d):
            (conv3 if m.kernel_size == (3, 3) else conv1).add((m.in_channels, m.out_channels, size[stage]))
        elif isinstance(m, torch.nn.GroupNorm):
            gn.add((m.num_channels, size[stage]))
        elif isinstance(m, afdm.SelfAttention):
            sa.add((m.channels, m.size))
            ln.add((m.channels, m.size))                 # its two LayerNorms work on the block's own map
    return conv3, conv1, gn, ln, sa
