"""The cases of tests/test_gpu_unet64_ops.py are the model's, fair and sharp (no device needed):
1. the tables of tests/unet64_cases.py cover every layer shape a UNet(image_size=64) launches;
2. with plain CPU fp32 torch in the kernels' place every case passes the gates the GPU test uses (so a gate missed on the device
   is the kernel's fault); the fp32 error is recorded beside the case (printed with -s);
3. the gates reject the faults that live at these shapes: a bottom halo row read from the next image, the last two-row band
   of one image computed with another channel block's weights, the last key tile of an attention row dropped."""
import pytest
import torch
import torch.nn.functional as F

import unet64_cases as U

FP32 = {}                                                 # the record: {case id: worst fp32 error (and where)}


def _record(key, err, where=""):
    if key not in FP32 or err > FP32[key][0]:
        FP32[key] = (err, where)


# ---- 1. the shapes are the model's -----------------------------------------------------------------------------------------
def test_tables_cover_the_layers_of_the_64_model():
    import afdm
    net = afdm.UNet(image_size=64, variant=0, device="cpu")
    assert net.image_size == 64
    conv3, conv1, gn, ln, sa = U.model_shapes(net)
    assert len(conv3) == 20 and conv1 == {(64, 3, 64)}
    have3 = {(c.case[1], c.case[2], c.case[3]) for c in U.CONV_CASES if c.case[5] == 3 and c.case[3] == c.case[4]}
    have1 = {(c.case[1], c.case[2], c.case[3]) for c in U.CONV_CASES if c.case[5] == 1}
    assert conv3 <= have3, sorted(conv3 - have3)
    assert conv1 <= have1
    gn_have = {(s[1], s[2]) for s, _ in U.GN_CASES} | {(s[1], s[2]) for s in U.GNFA_CASES}
    assert {c for c, _ in gn} <= {c for c, _ in gn_have}, (gn, gn_have)                 # every GroupNorm width ...
    big = {(c, s) for c, s in gn if c * s * s > 65536}                                   # ... and every (C, S) site past the register
    assert big <= gn_have and len(big) == 5, sorted(big - gn_have)                       # path (gn_fwd_loop), as the model pairs them
    assert {c for c, _ in ln} <= {s[1] for s, _ in U.LN_CASES} and ln == sa             # LayerNorm widths; the (C, S) pairs below
    blocks = {(c[1], c[2]) for c in U.BLOCK_CASES + U.BLOCK_UNFUSED_ONLY}
    attn = {(c[2], c[3]) for c in U.ATTN_CASES}
    lns = {(s[1], s[2]) for s, _ in U.LN_CASES}
    assert sa == {(128, 32), (256, 16), (256, 8), (128, 16), (64, 32), (64, 64)}
    for C, S in sa:
        assert (C // afdm.SelfAttention.heads, S * S) in attn, (C, S)               # its attention core, whatever the chain
        if C <= 128:                                      # the fused token chain (afd_tok_supported: C in {32, 64, 128})
            assert (C, S) in blocks, (C, S)
        else:                                             # C = 256: LayerNormC + 1x1 convolutions (blocks.py:52-63)
            assert {(C, 3 * C, S), (C, C, S)} <= have1 and (C, S) in lns, (C, S)
    # every listed 64x64 / 2x2 3x3 case needs NPB = 8 in conv_wgrad_mfma (conv.hip:921), and no other map of the model does
    assert U.wgrad_npb(64, 64) == 8 and U.wgrad_npb(2, 2) == 8 and [U.wgrad_npb(s, s) for s in (32, 16, 8, 4)] == [5, 4, 4, 5]
    for variant in (0, 3):                               # section H's count: 182 parameter tensors in both variants
        fs = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": 1.5707963267948966, "omega_c_up": 1.5707963267948966}
        m = afdm.UNet(image_size=64, variant=variant, device="cpu", f_settings=fs if variant else None)
        assert len(list(m.named_parameters())) == 182


def test_launcher_rules_restated():
    """unet64_cases.mfma_form / geom_xs against the figures the issue and conv.hip state."""
    assert U.geom_xs(64, 64, 128, 1) == 264 and U.geom_xs(64, 64, 64, 1) == 198 and U.geom_xs(2, 2, 64, 1) == 256
    assert [U.geom_xs(s, s, 128, 1) for s in (32, 16, 8, 4)] == [204, 180, 200, 288]          # Geo<1..4>, conv.hip:265-268
    assert U.mfma_form(3, 64, 64, 64, 64, 9, "auto") == "conv_mfma_sk"
    assert U.mfma_form(3, 64, 64, 64, 64, 9, "big") == "conv_mfma<BN 64, GEO 0>"
    assert U.mfma_form(3, 8, 32, 64, 64, 9, "auto") == "conv_mfma<BN 32, GEO 0>"
    assert U.mfma_form(2, 16, 24, 6, 10, 9, "auto") == "conv_direct"
    assert U.mfma_form(2, 32, 32, 32, 32, 9, "big") == "conv_mfma<BN 32, GEO 1>"
    for H, W in ((8, 16), (16, 8), (32, 16), (4, 8)):
        assert U.tile_ok(H, W, 128) and U.tile_ok(H, W, 64) and "GEO 0" in U.mfma_form(3, 64, 64, H, W, 9, "big")


# ---- 2. plain fp32 is inside every gate ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", U.CONV_CASES, ids=U.conv_id)
def test_conv_case_passes_in_fp32(cc):
    inp, r64, gates, fp32 = U.conv_ref(cc)
    assert all(float(v.norm()) > 0 and torch.isfinite(v).all() for v in r64.values())
    for (k, name), e in fp32.items():
        _record(U.conv_id(cc), e, (k, name))
        assert e < (U.TOL if name is None else gates[(k, name)]), (k, name, e)
    if cc.section in ("A", "B", "D"):                    # the slices exist, and on 64-wide maps the band of every image is one
        names = {n for (_, n) in gates}
        assert {"border ring", "interior"} <= names or cc.case[3] <= 2
        assert ("last row band of image 0" in names) == (cc.case[4] == 64)
    print(f"{U.conv_id(cc)}: fp32 worst {FP32[U.conv_id(cc)][0]:.2e} at {FP32[U.conv_id(cc)][1]}")


@pytest.mark.parametrize("mode", U.GN_MODES)
@pytest.mark.parametrize("shape", sorted({s for s, _ in U.GN_CASES}))
def test_groupnorm_case_passes_in_fp32(shape, mode):
    inp = U.gn_inputs(shape, mode)
    (y64, g64), (y32, g32) = U.gn_torch(inp, mode, torch.float64), U.gn_torch(inp, mode, torch.float32)
    errs = {"y": U.rel_l2(y32, y64), **{k: U.rel_l2(g32[k], g64[k]) for k in g64}}
    _record(("GroupNorm1", shape, mode), max(errs.values()), max(errs, key=errs.get))
    print(f"GroupNorm1 {shape} {mode}: fp32 {errs}")
    assert max(errs.values()) < U.TOL, errs


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", U.GNFA_CASES)
def test_groupnorm_filt_act_case_passes_in_fp32(shape, with_res):
    inp = U.gnfa_inputs(shape, with_res)
    (y64, g64), (y32, g32) = U.gnfa_torch(inp, torch.float64), U.gnfa_torch(inp, torch.float32)
    errs = {"y": U.rel_l2(y32, y64), **{k: U.rel_l2(g32[k], g64[k]) for k in g64}}
    _record(("GroupNormFiltAct", shape, with_res), max(errs.values()), max(errs, key=errs.get))
    print(f"GroupNormFiltAct {shape} res={with_res}: fp32 {errs}")
    assert max(errs.values()) < U.TOL, errs


@pytest.mark.parametrize("shape", [s for s, _ in U.LN_CASES])
def test_layernorm_case_passes_in_fp32(shape):
    inp = U.ln_inputs(shape)
    r64, r32 = U.ln_torch(inp, torch.float64), U.ln_torch(inp, torch.float32)
    errs = [U.rel_l2(r32[0], r64[0])] + [U.rel_l2(a, b) for leg in (1, 2) for a, b in zip(r32[leg], r64[leg])]
    _record(("LayerNormC", shape), max(errs))
    print(f"LayerNormC {shape}: fp32 {['%.2e' % e for e in errs]}")
    assert max(errs) < U.TOL, errs


@pytest.mark.parametrize("cfg", U.ATTN_CASES, ids=lambda c: "B%d_h%d_d%d_L%d" % c)
def test_attention_case_passes_in_fp32(cfg):
    qkv, dy = U.attn_inputs(cfg)
    r64, r32 = U.attn_torch(cfg, qkv, dy, torch.float64), U.attn_torch(cfg, qkv, dy, torch.float32)
    errs = [U.rel_l2(a, b) for a, b in zip(r32, r64)]
    _record(("attention", cfg), max(errs))
    print(f"attention {cfg} [{U.attn_form(cfg[2], cfg[3])}]: fp32 o {errs[0]:.2e} lse {errs[1]:.2e} dqkv {errs[2]:.2e}")
    assert max(errs) < U.TOL, errs


@pytest.mark.parametrize("case", U.BLOCK_CASES, ids=lambda c: "B%d_C%d_S%d" % c)
def test_attention_block_case_passes_in_fp32(case):
    mod, x, dy = U.block_state(case)
    sd = mod.state_dict()
    (y64, g64), (y32, g32) = U.block_torch(sd, x, dy, torch.float64), U.block_torch(sd, x, dy, torch.float32)
    errs = {"y": U.rel_l2(y32, y64), **{k: U.rel_l2(g32[k], g64[k]) for k in g64}}
    _record(("attention block", case), max(errs.values()), max(errs, key=errs.get))
    print(f"attention block {case}: fp32 worst {max(errs.values()):.2e} at {max(errs, key=errs.get)}")
    assert max(errs.values()) < U.TOL, errs


# ---- 3. the gates see the faults that live here --------------------------------------------------------------------------------
def _failed(cc, got, r64, gates):
    return [(k, n, e, gate) for k, n, e, gate in U.conv_checks(cc, got, r64, gates) if not e < gate]


def _case(section, case):
    return next(c for c in U.CONV_CASES if c.section == section and c.case[:5] == case)


@pytest.mark.parametrize("key", [("A", (3, 64, 64, 64, 64)), ("B", (3, 512, 512, 8, 8))], ids=["64x64", "8x8_two_images_per_tile"])
def test_gates_reject_a_bottom_halo_row_from_the_next_image(key):
    """The padding row below image b holds row 0 of image b + 1 (zero below the last): a tile that spans or abuts images reading
    on instead of masking."""
    cc = _case(*key)
    inp, r64, gates, _ = U.conv_ref(cc)

    def fwd(x, w, b):
        xp = F.pad(x, (1, 1, 1, 1))
        nxt = torch.cat([x[1:, :, 0, :], torch.zeros_like(x[:1, :, 0, :])])
        xp = torch.cat([xp[:, :, :-1], F.pad(nxt, (1, 1))[:, :, None, :]], dim=2)
        return F.conv2d(xp, w, b)
    bad = U.conv_torch(cc, inp, torch.float64, fwd=fwd)
    assert not _failed(cc, r64, r64, gates)                                    # the reference itself passes
    failed = _failed(cc, bad, r64, gates)
    hit = {(k, n) for k, n, _, _ in failed}
    assert ("y", None) in hit and ("y", "border ring") in hit and ("dx", None) in hit, sorted(hit, key=str)
    # the fault is local: the last image (zero below it, as it should be) and, on the 64-wide map, the interior stay clean
    B = cc.case[0]
    assert ("y", f"image {B - 1}") not in hit and (cc.case[3] != 64 or ("y", "last row band") in hit)
    assert all(("y", f"image {b}") in hit for b in range(B - 1))


def test_gates_reject_a_stale_last_row_band_of_one_image():
    """Rows 62-63 of image 1 computed with the weights of the previous 32-channel block (a persistent workgroup that kept the
    previous item's staged weights for its last band): 1/96 of the output."""
    cc = _case("A", (3, 64, 64, 64, 64))
    inp, r64, gates, _ = U.conv_ref(cc)

    def fwd(x, w, b):
        y = F.conv2d(x, w, b, padding=1)
        stale = F.conv2d(x[1:2, :, 60:], torch.roll(w, 32, dims=0), b, padding=1)[:, :, 2:]
        y = y.clone()
        y[1, :, 62:] = stale[0]
        return y
    bad = U.conv_torch(cc, inp, torch.float64, fwd=fwd)
    hit = {(k, n) for k, n, _, _ in _failed(cc, bad, r64, gates)}
    assert {("y", None), ("y", "image 1"), ("y", "last row band"), ("y", "last row band of image 1"), ("y_gelu", "last row band of image 1")} <= hit
    assert ("y", "image 0") not in hit and ("y", "image 2") not in hit and ("y", "last row band of image 0") not in hit
    # the whole-tensor figure dilutes the fault with the batch size; the band slice of that image does not
    e_whole = U.rel_l2(bad["y"], r64["y"])
    e_band = U.rel_l2(bad["y"][1, :, 62:], r64["y"][1, :, 62:])
    assert e_band > 5 * e_whole > 50 * U.TOL


def test_gates_reject_an_attention_reference_without_its_last_64_keys():
    cfg = (1, 1, 16, 4096)
    qkv, dy = U.attn_inputs(cfg)
    good = U.attn_torch(cfg, qkv, dy, torch.float64)
    bad = U.attn_torch(cfg, qkv, dy, torch.float64, drop_last_keys=64)
    errs = [U.rel_l2(a, b) for a, b in zip(bad, good)]
    print("attention without the last 64 of 4096 keys: o %.2e lse %.2e dqkv %.2e" % tuple(errs))
    assert all(e > 100 * U.TOL for e in errs), errs


def test_ramped_inputs_make_an_h_w_swap_visible():
    """Section D: a kernel that took the (8, 16) map for a (16, 8) one reads the same bytes as another image; with the ramps the
    result is far outside the gate, on every output."""
    cc = _case("D", (3, 32, 64, 8, 16))
    inp, r64, gates, _ = U.conv_ref(cc)
    sw = lambda t: None if t is None else (t.reshape(t.shape[0], t.shape[1], 16, 8) if t.dim() == 4 and t.shape[-1] == 16 else t)
    swapped = U.conv_torch(cc, {k: sw(v) for k, v in inp.items()}, torch.float64)
    for k in ("y", "dx", "dw"):
        got = swapped[k].reshape(r64[k].shape)
        assert U.rel_l2(got, r64[k]) > 1000 * U.TOL, k
