"""The kernels and launcher branches that only the default UNet(image_size=64) reaches, each against an fp64 reference of the
same operation (tests/unet64_cases.py holds the tables, the references and the gates; tests/test_unet64_cases_host.py shows on the
CPU that the cases are the model's, that plain fp32 passes every gate and that the gates reject the faults that live here).

Every case runs forward and every gradient through the public ops.* autograd functions.  Before it launches, a case asks the
library's query entry points which form is about to run, asserts the intended one and puts it in the ledger label; where no query
exists, the launcher's condition is restated in unet64_cases.py with its file and line."""
import ctypes
import math
import os

import pytest
import torch

import unet64_cases as U
from conftest import check, note, rel_l2
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu
TOL = U.TOL
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    return afdm, ops, gpu


# ---------------------------------------------------------------------------------------------------------------------------
# A - D: convolutions
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_forms(L, cc, path):
    """-> the (forward, dgrad, wgrad) forms under the switches now set, from the query entry points; asserts what the case is about."""
    B, Cin, Cout, H, W, ks, _, _ = cc.case
    if ks == 1:
        # no query reports the 1x1 forward / dgrad choice: ends_fwd / ends_dgrad first (Cout < 8, ends.hip), then the streaming
        # pw_mfma kernel where pw_launch admits the layer (pw.hip:113-115: K even, 8 <= K <= 64, N >= 8; by rule only from 32768
        # pixels and, for dgrad, K <= 32), else launch_mfma<1> (conv.hip:985-990); the weight gradient by afd_conv_wgrad_form
        def one(K, N, dgrad):
            if Cout < 8 and path != "noends":
                return "ends"
            ok = K % 2 == 0 and 8 <= K <= 64 and N >= 8
            if ok and (path == "pw" or (B * H * W >= 32768 and not (dgrad and K > 32))):
                return "pw_mfma"
            return U.mfma_form(B, K, N, H, W, 1, path)
        wf = L.afd_conv_wgrad_form(B, Cin, Cout, H, W, 1)
        fwd, dgr = one(Cin, Cout, False), one(Cout, Cin, True)
        if Cout < 8:                                      # outc: the ends kernels come first whatever pw says (conv.hip:985-986,
            assert (fwd, dgr) == (("conv_direct", "conv_mfma<BN 64, GEO 5>") if path == "noends" else ("ends", "ends"))   # 1003-1004)
            assert wf == 0
        else:
            assert wf == 4                                # pw_wgrad_h2
            if path == "pw":                              # forced: the forward is admitted (K = 64), the dgrad is not (K = 192 > 64)
                assert fwd == "pw_mfma" and dgr != "pw_mfma" and fwd != U.mfma_form(B, Cin, Cout, H, W, 1, "auto")
            else:
                assert "pw_mfma" not in (fwd, dgr)
        return fwd, dgr, {0: "conv_wgrad_mfma<1>", 2: "pw_wgrad_bf3", 4: "pw_wgrad_h2"}[wf]
    nb = L.afd_conv3x3_wino_workspace_bytes(B, Cin, Cout, H, W, 0)
    nd = L.afd_conv3x3_wino_workspace_bytes(B, Cin, Cout, H, W, 1)
    kinds = L.afd_conv3x3_weight_kinds(B, Cin, Cout, H, W)
    fwd = (U.h2_form(path, B, Cout, W) if kinds & 1 else "Winograd") if nb else U.mfma_form(B, Cin, Cout, H, W, 9, path)
    dgr = (U.h2_form(path, B, Cin, W) if kinds & 2 else "Winograd") if nd else U.mfma_form(B, Cout, Cin, H, W, 9, path)
    wf = L.afd_conv_wgrad_form(B, Cin, Cout, H, W, 3)
    if wf == 0:
        ok = U.tile_ok(H, W, 64) and U.geom_xs(H, W, 64, 1) <= 256                 # conv.hip:1152
        nw = {"wgrad4": "4 waves forced", "wgrad8": "8 waves forced"}.get(path, f"{U.wgrad_waves(B, Cin, Cout, H, W)} waves by rule")
        wg = f"conv_wgrad_mfma<NPB {U.wgrad_npb(H, W)}, {2 if Cout > 32 else 1}x{2 if Cin > 32 else 1}, {nw}>" if ok else "conv_direct_wgrad"
    elif wf in (2, 4):
        info = (ctypes.c_int * 5)()
        L.afd_conv_wgrad3_plan(B, Cin, Cout, H, W, ctypes.addressof(info))
        wg = f"{'wgrad_h2' if wf == 4 else 'wgrad_bf3'}<{info[2]}x{info[3]}, {info[4]} waves>"
    else:
        wg = {1: "wgrad_wino", 3: "wgrad_cin3"}[wf]
    # ---- what the case is about
    if W == 64 or (H, W) == (2, 2):
        assert kinds == 0, "no f16x2 / bf16x3 direct form on these maps (direct_plan, bf3.hip:247)"
        if Cin >= 8:
            assert wf == 0 and "NPB 8" in wg, (wf, wg)                              # conv_wgrad_mfma<9, ., ., 8, .>
            info = (ctypes.c_int * 5)()
            assert L.afd_conv_wgrad3_plan(B, Cin, Cout, H, W, ctypes.addressof(info)) == 0
    if cc.case[:5] == (2, 3, 64, 64, 64):
        assert wf == 3 and "GEO 0" in fwd and dgr == "conv_direct"               # wgrad_cin3<64>; ragged-chunk forward
    if cc.case[:5] == (16, 64, 64, 64, 64):
        assert nb != 0 and nd != 0 and fwd == "Winograd"                           # the rule really picks Winograd (wino.hip:545)
    if W == 64 and path.startswith("wino") and Cin % 8 == 0 and Cout % 32 == 0:
        assert nb != 0 and fwd == "Winograd", (path, nb)                          # conv_wino<64, BN, NT>, forced
        fwd += f" {path[4:]}"
        if Cout % 8 == 0 and Cin % 32 == 0:
            assert nd != 0
            dgr += f" {path[4:]}"
    if W == 64 and path in ("nowino", "big", "splitk", "wgrad4", "wgrad8") and B < 16:
        assert nb == 0 and nd == 0
    if cc.case[:5] == (3, 64, 64, 64, 64) and path in ("auto", "big", "splitk"):
        assert fwd == {"auto": "conv_mfma_sk", "splitk": "conv_mfma_sk", "big": "conv_mfma<BN 64, GEO 0>"}[path]
    if cc.case[:5] == (3, 8, 32, 64, 64) and path in ("auto", "big", "nowino"):
        assert fwd == "conv_mfma<BN 32, GEO 0>"
    if cc.section == "B":                                 # every forced path really selects its form (unet64_cases.py, section B)
        if path in ("bf3", "h2reg", "h2l64", "h2l256", "h2l32", "h2sk"):
            assert kinds & 1 and kinds & 2 and nb != 0 and nd != 0, (path, kinds)
            want = {"bf3": "register-fed", "h2reg": "register-fed", "h2l64": "128 px, 2 blocks", "h2l32": "128 px, 1 block", "h2sk": "split-K",
                    "h2l256": "256 px, 1 block" if W >= 16 else "128 px, 1 block"}[path]      # (no 256-pixel workgroup on 8x8, h2.hip:1020)
            assert want in fwd and want in dgr, (path, fwd, dgr)
        else:
            assert kinds == 0, (path, kinds)              # auto at these batch sizes, and every path that is not a direct form
        if path in U.WINO4 + ("winosk",):
            assert nb != 0 and nd != 0 and fwd == dgr == "Winograd", (path, nb, nd)
            fwd, dgr = f"Winograd {path[4:]}", f"Winograd {path[4:]}"
        if path in ("auto", "big", "splitk", "nobf3", "nowino", "wgbf3", "nowgbf3", "nowgwino", "nowgbf3+wgwino"):
            assert nb == 0 and nd == 0, (path, nb, nd)
            assert fwd == dgr == (f"conv_mfma<BN 64, GEO {dict(((32, 1), (16, 2), (8, 3)))[W]}>" if path == "big" else "conv_mfma_sk"), (path, fwd)
        if path in ("nowgbf3", "nowgbf3+wgwino"):
            assert wf == 1, (path, wf)                    # wgrad_wino
            wg += " by rule" if path == "nowgbf3" else " forced"
        else:
            assert wf == 4 and wf != 1, (path, wf)        # wgrad_h2 (wgbf3: wherever covered; auto: by rule; nowgwino: not Winograd)
    if cc.section == "D":
        assert nb == 0 and nd == 0 and wf == 0 and ("GEO 0" in fwd or fwd == "conv_mfma_sk") and "conv_wgrad_mfma" in wg, (fwd, wg)
        if path == "big":
            assert "GEO 0" in fwd and "GEO 0" in dgr
        if path == "splitk":
            assert fwd == dgr == "conv_mfma_sk"
    return fwd, dgr, wg


def _conv_run(ops, dev, cc, inp):
    """The legs of _conv_case (test_gpu_ops.py) -> the outputs unet64_cases.conv_torch names."""
    has_bias, has_res = cc.case[6], cc.case[7]
    names = [k for k in ("x", "w", "bias", "res") if inp[k] is not None]
    dl = {k: inp[k].to(dev).requires_grad_(True) for k in names}
    dy = inp["dy"].to(dev)
    yd = ops.conv(dl["x"], dl["w"], dl.get("bias"), dl.get("res"))
    gd = torch.autograd.grad(yd, [dl[k] for k in names], dy)
    out = {"y": yd.detach().cpu()}
    for k, gr in zip(names, gd):
        out["d" + {"bias": "b"}.get(k, k)] = gr.cpu()
    if U.conv_has_fork(cc):
        dr = inp["dr"].to(dev)
        yf, xr = ops.conv(dl["x"], dl["w"], fork=True)
        assert torch.equal(xr.detach(), dl["x"].detach())
        (gx,) = torch.autograd.grad((yf * dy).sum() + (xr * dr).sum(), [dl["x"]])
        out["dx_fork"] = gx.cpu()
    with torch.no_grad():
        out["y_gelu"] = ops.conv_infer(dl["x"], dl["w"], dl.get("bias"), dl.get("res"), act=1).cpu()
    return out


@pytest.mark.parametrize("cc", U.CONV_CASES, ids=U.conv_id)
def test_conv_fwd_dgrad_wgrad_at_unet64_shapes(A, cc):
    """Sections A - D: whole tensors at 1e-5 against fp64, slices (sections A, B, D) at max(1e-5, 2 x CPU fp32's error on the
    slice); every path of the case, the reference computed once."""
    afdm, ops, dev = A
    L = afdm.lib()
    inp, r64, gates, _ = U.conv_ref(cc)
    failed = []
    for path in cc.paths:
        modes = U.PATH_MODES[path]
        for m in (modes if isinstance(modes, tuple) else (modes,)):
            L.afd_debug_conv_path(m)
        try:
            form = _conv_forms(L, cc, path)
            got = _conv_run(ops, dev, cc, inp)
        finally:
            for m in U.PATH_RESTORE:
                L.afd_debug_conv_path(m)
        for k, name, e, gate in U.conv_checks(cc, got, r64, gates):
            leg = 0 if k.startswith("y") else (2 if k in ("dw", "db") else 1)
            fam = f"U64 {cc.section} conv {('fwd', 'dgrad', 'wgrad')[leg]}{'' if name is None else ' slices'} vs fp64 [{form[leg]}]"
            note(fam, e, (cc.case, path, k, name, f"gate {gate:.2e}"))
            if not e < gate:
                failed.append((path, k, name, e, gate))
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------------------------
# E: norms
# ---------------------------------------------------------------------------------------------------------------------------
def _misaligned(t, dev):
    """A contiguous copy of t on the device whose first element sits 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("bwd_form", ["rule", "two_pass"])
@pytest.mark.parametrize("mode", U.GN_MODES)
@pytest.mark.parametrize("shape,odd", U.GN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("view+4" if v else "aligned"))
def test_groupnorm_loop_and_apply(A, shape, odd, mode, bwd_form):
    """n = C*H*W > 65536: gn_fwd_loop (norm.hip:534,544); backward by gn_bwd_plane + gn_bwd_apply over min(64, ceil(n / 8192))
    slices (norm.hip:564,580-584) under both settings of afd_debug_norm_path (n > 32768 leaves the sample-resident form out)."""
    afdm, ops, dev = A
    B, C, H, W = shape
    n = C * H * W
    assert n > 65536 or H * W % 4
    slices = min(64, (n + 8191) // 8192)
    form = f"gn_fwd_loop, plane + apply x {slices} slices{', n / 8192 capped' if n > 64 * 8192 else ''}{', views 4 bytes past 16' if odd else ''}"
    inp = U.gn_inputs(shape, mode)
    y64, g64 = U.gn_torch(inp, mode, torch.float64)
    put = (lambda t: _misaligned(t, dev)) if odd else (lambda t: t.to(dev))
    names = list(g64)
    dl = {k: (put(inp[k]) if k in ("x", "res") else inp[k].to(dev)).requires_grad_(True) for k in names}
    afdm.lib().afd_debug_norm_path(1 if bwd_form == "two_pass" else 0)
    try:
        yd = ops.GroupNorm1.apply(dl["x"], dl["gamma"], dl["beta"], dl.get("res"), dl.get("emb"), 1 if mode in ("res_gelu", "gelu") else 0)
        gd = torch.autograd.grad(yd, [dl[k] for k in names], inp["dy"].to(dev))
    finally:
        afdm.lib().afd_debug_norm_path(0)
    check(f"U64 E GroupNorm fwd vs fp64 [{form}]", yd.detach().cpu(), y64, TOL, (shape, mode, bwd_form))
    for k, gr in zip(names, gd):
        check(f"U64 E GroupNorm bwd vs fp64 [{form}]", gr.cpu(), g64[k], TOL, (shape, mode, bwd_form, "d" + k))


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", U.GNFA_CASES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_filt_act_at_unet64_shapes(A, shape, with_res):
    afdm, ops, dev = A
    B, C, H, W = shape
    gn = bool(afdm.lib().afd_filt_act_fwd_gn_supported(C, H, W, 3))
    assert not gn                                                    # every GroupNorm + filtered GELU site of the 64 model: stats + act
    form = "_gn (sample-resident)" if gn else "stats + act"
    inp = U.gnfa_inputs(shape, with_res)
    y64, g64 = U.gnfa_torch(inp, torch.float64)
    names = list(g64)
    dl = {k: inp[k].to(dev).requires_grad_(True) for k in names}
    ku, kd = U.filt_kernels()
    yd = ops.GroupNormFiltAct.apply(dl["x"], dl["gamma"], dl["beta"], dl.get("res"), ops.Taps(ku), ops.Taps(kd))
    gd = torch.autograd.grad(yd, [dl[k] for k in names], inp["dy"].to(dev))
    check(f"U64 E GroupNorm + filtered GELU fwd vs fp64 [{form}]", yd.detach().cpu(), y64, TOL, (shape, with_res))
    for k, gr in zip(names, gd):
        check(f"U64 E GroupNorm + filtered GELU bwd vs fp64 [{form}]", gr.cpu(), g64[k], TOL, (shape, with_res, "d" + k))


@pytest.mark.parametrize("shape,form", U.LN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_layernorm_c_forms(A, shape, form):
    """The legs of test_layernorm_c at the pixel counts where the launcher changes form (norm.hip:597-603,623-628)."""
    _, ops, dev = A
    B, C, H, W = shape
    pixels = B * H * W
    want = ("generic" if C not in (32, 64, 128) else ("fwd_reg" if pixels >= 32768 else ("split<%d, 8>" % C if pixels >= 8192 else "split<%d, 16>" % C)))
    assert form.startswith(want), (form, want)
    inp = U.ln_inputs(shape)
    y64, g1, g2 = U.ln_torch(inp, torch.float64)
    dl = [inp[k].to(dev).requires_grad_(True) for k in ("x", "gamma", "beta")]
    dy, dr = inp["dy"].to(dev), inp["dr"].to(dev)
    yd, xres = ops.LayerNormC.apply(*dl)
    gd = torch.autograd.grad(yd, dl, dy)
    check(f"U64 E LayerNorm fwd vs fp64 [{form}]", yd.detach().cpu(), y64, TOL, shape)
    assert torch.equal(xres.detach().cpu(), inp["x"])
    for i, (a, b) in enumerate(zip(gd, g1)):
        check(f"U64 E LayerNorm bwd vs fp64 [{form}]", a.cpu(), b, TOL, (shape, i))
    yd, xres = ops.LayerNormC.apply(*dl)                                           # the residual routed through the node
    gd2 = torch.autograd.grad((yd * dy).sum() + (xres * dr).sum(), dl)
    for i, (a, b) in enumerate(zip(gd2, g2)):
        check(f"U64 E LayerNorm bwd (+ residual) vs fp64 [{form}]", a.cpu(), b, TOL, (shape, i))
    (gres,) = torch.autograd.grad((ops.LayerNormC.apply(*dl)[1] * dr).sum(), dl[:1])
    assert rel_l2(gres.cpu(), inp["dr"]) < 1e-7


def test_filt_fast_paths_do_not_write_outside_their_tensors_at_64(A):
    """test_filt_fast_paths_do_not_write_outside_their_tensors at S = 64: one plane per wave, so 1, 3 and 5 planes leave 3, 1 and
    3 waves of the four-wave workgroups without a plane: they must exit."""
    afdm, ops, dev = A
    L = afdm.lib()
    s = torch.cuda.current_stream().cuda_stream
    S = 64
    tk = ops.Taps(afdm.circularLowpassKernel(math.pi / 2, 3, 2))
    for planes in (1, 3, 5):
        B, C = 1, planes
        n, n_hi = planes * S * S, planes * 4 * S * S
        pad = 4096
        x = torch.randn(B, C, S, S, device=dev)
        x_hi = torch.randn(B, C, 2 * S, 2 * S, device=dev)
        st = torch.zeros(B, 2, device=dev); st[:, 1] = 1
        g, be = torch.ones(C, device=dev), torch.zeros(C, device=dev)

        def guarded(numel):
            buf = torch.full((numel + 2 * pad,), 7.25, device=dev)
            return buf, buf[pad:pad + numel]

        def intact(buf, numel, what):
            assert bool((buf[:pad] == 7.25).all()) and bool((buf[pad + numel:] == 7.25).all()), (what, S, planes)
            assert bool(torch.isfinite(buf[pad:pad + numel]).all()) and not bool((buf[pad:pad + numel] == 7.25).all()), (what, "not written")

        buf, y = guarded(n)
        L.afd_filt_act_fwd(x.data_ptr(), y.data_ptr(), B, C, S, S, st.data_ptr(), g.data_ptr(), be.data_ptr(), None, tk.ptr, tk.ptr, 3, None, s)
        intact(buf, n, "filt_act_fwd")
        buf, dv = guarded(n)
        pbuf, part = guarded(B * C * 2)
        L.afd_filt_act_bwd(x.data_ptr(), x.data_ptr(), dv.data_ptr(), B, C, S, S, st.data_ptr(), g.data_ptr(), be.data_ptr(), None, tk.ptr, tk.ptr, 3, None,
                           part.data_ptr(), s)
        intact(buf, n, "filt_act_bwd"); intact(pbuf, B * C * 2, "filt_act_bwd partials")
        buf, up = guarded(n_hi)
        L.afd_filt_up2_fwd(x.data_ptr(), up.data_ptr(), B, C, S, S, 0, 0, tk.ptr, 3, s)
        intact(buf, n_hi, "up2_fwd")
        buf, dn = guarded(n)
        L.afd_filt_down2_fwd(x_hi.data_ptr(), dn.data_ptr(), B, C, 2 * S, 2 * S, 0, 0, tk.ptr, 3, s)
        intact(buf, n, "down2_fwd")
        buf, dx = guarded(n)
        L.afd_filt_up2_bwd(x_hi.data_ptr(), dx.data_ptr(), B, C, S, S, 0, 0, tk.ptr, 3, s)
        intact(buf, n, "up2_bwd")
        buf, dxh = guarded(n_hi)
        L.afd_filt_down2_bwd(x.data_ptr(), dxh.data_ptr(), B, C, 2 * S, 2 * S, 0, 0, tk.ptr, 3, s)
        intact(buf, n_hi, "down2_bwd")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# F: attention core
# ---------------------------------------------------------------------------------------------------------------------------
_cfg_id = lambda c: "B%d_h%d_d%d_L%d" % c


@pytest.mark.parametrize("cfg", U.ATTN_CASES, ids=_cfg_id)
def test_attention_core_at_unet64_shapes(A, cfg):
    """ops.Attention forward and backward against fp64 at 1e-5 (the rule's kernels: attn.hip:382-400,412-446)."""
    afdm, ops, dev = A
    B, heads, d, L = cfg
    form = U.attn_form(d, L)
    qkv, dy = U.attn_inputs(cfg)
    o64, _, g64 = U.attn_torch(cfg, qkv, dy, torch.float64)
    qd = qkv[..., None].to(dev).requires_grad_(True)
    yd = ops.Attention.apply(qd, heads)
    (gd,) = torch.autograd.grad(yd, qd, dy[..., None].to(dev))
    check(f"U64 F attention core fwd vs fp64 [{form}]", yd.detach().cpu()[..., 0], o64, TOL, cfg)
    C = heads * d
    for name, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
        check(f"U64 F attention core bwd vs fp64 [{form}]", gd.cpu()[:, sl, :, 0], g64[:, sl], TOL, (cfg, name))


def _attn_abi(A, cfg, qkv, dy, code=None):
    """afd_attn_fwd + afd_attn_bwd through the C ABI with o, lse, dqkv and the delta workspace starting as NaN (_run of
    test_gpu_attn_d16.py); code 40 forces the round-2 kernels at d = 16."""
    afdm, ops, dev = A
    B, heads, d, L = cfg
    C = heads * d
    P = lambda t: t.data_ptr()
    qd, gd = qkv.to(dev).contiguous(), dy.to(dev).contiguous()
    o = torch.full((B, C, L), float("nan"), device=dev)
    lse = torch.full((B, heads, L), float("nan"), device=dev)
    dqkv = torch.full((B, 3 * C, L), float("nan"), device=dev)
    ws = torch.full((B, heads, L), float("nan"), device=dev)
    lib = afdm.lib()
    try:
        if code is not None:
            lib.afd_debug_attn_rows(code)
        lib.afd_attn_fwd(P(qd), P(o), P(lse), B, heads, d, L, ops._stream())
        lib.afd_attn_bwd(P(qd), P(o), P(gd), P(lse), P(dqkv), P(ws), B, heads, d, L, ops._stream())
        torch.cuda.synchronize()
    finally:
        if code is not None:
            lib.afd_debug_attn_rows(41)
    return o.cpu(), lse.cpu(), dqkv.cpu()


@pytest.mark.parametrize("variant", ["peaked", "row shift"])
@pytest.mark.parametrize("cfg", U.ATTN_VARIANTS, ids=_cfg_id)
def test_attention_core_peaked_and_shifted_rows(A, cfg, variant):
    """test_d16_peaked_softmax / test_d16_row_shift at the 64 model's sequence lengths, with that file's gate unchanged: every
    output finite and its error against fp64 at most twice that of the kernels afd_debug_attn_rows(40) selects on the same
    inputs.  These kernels take exp2(S - lse) from the stored lse, so the error on such rows follows lse's rounding and is not
    promised to 1e-5.  At d = 16 code 40 is the round-2 kernel family; d = 32 has no second family (code 40 leaves
    launch_fwd/dq<32, 2> where they are), so there the test asserts finite outputs and two runs equal bit for bit, and the figures are recorded
    beside those of plain CPU fp32 on the same inputs.  Measured on MI355X, rel-L2 against fp64, kernel | code-40 kernels | CPU
    fp32, the worse of the two cases of each head dim:
      d = 16 peaked     o 3.71e-7 | 1.03e-6 | 2.98e-7   lse 8.68e-8 | 8.67e-8 | 7.22e-8   dqkv 6.37e-6 | 7.32e-6 | 1.77e-6
      d = 16 row shift  o 2.82e-6 | 2.91e-6 | 2.82e-6   lse 4.88e-8 | 3.98e-8 | 3.00e-8   dqkv 2.39e-6 | 2.08e-5 | 9.14e-6
      d = 32 peaked     o 5.05e-7 |  same   | 3.50e-7   lse 8.37e-8 |  same   | 1.10e-7   dqkv 5.56e-6 |  same   | 2.95e-6
      d = 32 row shift  o 3.28e-6 |  same   | 4.45e-6   lse 4.04e-8 |  same   | 3.72e-8   dqkv 1.46e-5 |  same   | 6.93e-6
    The last figure, (1, 2, 32, 1024), is the one above 1e-5: the vector dQ pass contracts dS with K itself, not with K - mean(K)
    as the d = 16 matrix-core backward does, so a common shift of 30 sqrt(d) on one key feature costs it twice CPU fp32's error."""
    B, heads, d, L = cfg
    qkv, dy = U.attn_inputs(cfg, variant)
    r64 = U.attn_torch(cfg, qkv, dy, torch.float64)
    new, old = _attn_abi(A, cfg, qkv, dy), _attn_abi(A, cfg, qkv, dy, code=40)
    assert all(torch.isfinite(t).all() for t in new)
    if d != 16:                                           # the same kernels twice: bit for bit
        assert all(torch.equal(a, b) for a, b in zip(new, old))
    cpu = [rel_l2(a, w) for a, w in zip(U.attn_torch(cfg, qkv, dy, torch.float32), r64)]
    res = []
    for name, a, b, w, c in zip(("o", "lse", "dqkv"), new, old, r64, cpu):
        e_new, e_old = rel_l2(a, w), rel_l2(b, w)
        print(f"attention {variant} {cfg} {name}: {e_new:.2e}  code-40 kernels {e_old:.2e}  CPU fp32 {c:.2e}")
        note(f"U64 F attention core, {variant} rows, vs fp64 [{U.attn_form(d, L)}; gate 2 x the code-40 kernels]", e_new,
             (cfg, name, f"code-40 kernels {e_old:.2e}, CPU fp32 {c:.2e}"))
        res.append((name, e_new, e_old))
    for name, e_new, e_old in res:
        assert e_new <= 2.0 * e_old, (variant, name, e_new, e_old)


# ---------------------------------------------------------------------------------------------------------------------------
# G: the attention block
# ---------------------------------------------------------------------------------------------------------------------------
def _block_run(afdm, dev, mod, x, dy, names, grid_cap):
    L = afdm.lib()
    outs = {}
    try:
        for fused in (True, False):
            afdm.SelfAttention.fused = fused
            L.afd_debug_tok_grid(grid_cap)
            xi = x.to(dev).requires_grad_(True)
            y = mod(xi)
            params = dict(mod.named_parameters())
            grads = torch.autograd.grad(y, [xi] + [params[k] for k in names], dy.to(dev))
            with torch.no_grad():
                y_inf = mod(x.to(dev))
            outs[fused] = (y.detach().cpu(), [t.cpu() for t in grads], y_inf.cpu())
    finally:
        afdm.SelfAttention.fused = True
        L.afd_debug_tok_grid(0)
    return outs


@pytest.mark.parametrize("grid_cap", [0, 1])
@pytest.mark.parametrize("case", U.BLOCK_CASES + U.BLOCK_UNFUSED_ONLY, ids=lambda c: "B%d_C%d_%dx%d" % (c + c[2:]))
def test_fused_attention_block_at_unet64_shapes(A, case, grid_cap):
    """test_fused_attention_block_vs_oracle_and_unfused on sa1 / sa4 / sa5 / sa6 of the 64 model: the fused token chains against
    the fp64 oracle (1e-5) and the unfused HIP path (5e-6); (1, 64, 64) against the unfused path only."""
    afdm, ops, dev = A
    B, C, S = case
    assert afdm.lib().afd_tok_supported(C) and not afdm.lib().afd_tok_supported(256)
    mod, x, dy = U.block_state(case)
    names = list(mod.state_dict())
    with_oracle = case in U.BLOCK_CASES
    if with_oracle:
        y64, g64 = U.block_torch(mod.state_dict(), x, dy, torch.float64)
    outs = _block_run(afdm, dev, mod.to(dev), x, dy, names, grid_cap)
    y, grads, y_inf = outs[True]
    form = f"tok chain C {C}, d {C // 4}, L {S * S}, grid_cap {grid_cap}"
    e_uf = max([rel_l2(y, outs[False][0])] + [rel_l2(a, b) for a, b in zip(grads, outs[False][1])])
    note(f"U64 G fused attention block vs unfused HIP path [{form}]", e_uf, case)
    assert torch.equal(y, y_inf)
    if with_oracle:
        check(f"U64 G fused attention block fwd vs fp64 oracle [{form}]", y, y64, TOL, case)
        for k, gk in zip(["x"] + names, grads):
            check(f"U64 G fused attention block grads vs fp64 oracle [{form}]", gk, g64[k], TOL, (case, k))
    assert e_uf < 5e-6, e_uf


# ---------------------------------------------------------------------------------------------------------------------------
# H: one whole step at 64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,B", U.STEP_CASES, ids=lambda v: str(v))
def test_step_at_64_vs_cpu_oracle(A, variant, B):
    """test_full_batch_step_vs_cpu_oracle at image_size 64: one forward + backward of the product step against
    oracle.ref_ops.train_step_loss_and_grads with the same images / t / eps: loss 2e-5, every parameter-gradient tensor 1e-4."""
    afdm, ops, dev = A
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=64, f_settings=dict(F_SET) if variant else None, device="cpu", variant=variant)
    sd = {k: v.clone().requires_grad_(True) for k, v in model.state_dict().items()}
    model = model.to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=64, device=dev)
    g = torch.Generator().manual_seed(23 + variant)
    images = torch.rand(B, 3, 64, 64, generator=g) * 2 - 1
    t = torch.randint(1, 1000, (B,), generator=g)
    eps = torch.randn(B, 3, 64, 64, generator=g)
    step = afdm.TrainStep(model, diff, lr=3e-4, graph=False)
    loss = step._fwd_bwd(images.to(dev), t.to(dev), eps.to(dev))
    torch.cuda.synchronize()
    got = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    _, _, ah = R.noise_schedule(1000)
    nt = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    try:
        loss_o, _, grads_o = R.train_step_loss_and_grads(sd, images, t, eps, variant, F_SET, ah)
    finally:
        torch.set_num_threads(nt)
    e_loss = abs(loss.item() - loss_o.item()) / abs(loss_o.item())
    note(f"U64 H step at 64x64 (B = {B}, variant {variant}) vs CPU oracle: loss", e_loss)
    assert e_loss < 2e-5, e_loss
    assert set(grads_o) == set(got) and len(got) == 182
    worst = max(check(f"U64 H step at 64x64 (B = {B}, variant {variant}) vs CPU oracle: parameter gradients (fp32 vs fp32)", got[k], grads_o[k], 1e-4, k)
                for k in got)
    print(f"64x64 variant {variant} B = {B} step vs CPU oracle: loss rel {e_loss:.2e}, worst parameter-gradient rel-L2 {worst:.2e} over {len(got)} tensors")
