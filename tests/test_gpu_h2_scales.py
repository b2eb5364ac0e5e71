"""The running power-of-two scales of the f16x2 convolution kernels (csrc/h2_common.h) on inputs that make them MOVE
(tests/h2_cases.py; tests/test_h2_cases_host.py shows that plain fp32 passes every gate used here on the same inputs):

  conv_h2 (register-fed), conv_h2l as (128 px, 2 blocks), (256, 1), (128, 1), conv_h2_sk       forward and dgrad
  wgrad_h2 on 32 x 32, 16 x 16, 8 x 8 maps, wgrad_h2_s4                                        3x3 weight gradient
  pw_wgrad_h2                                                                                  1x1 / token-Linear weight gradient

Oracle: F.conv2d and autograd (an einsum for the 1x1 gradient) in fp64 on the CPU.  Gate: the contract's rel-L2 < 1e-5, per
slice that owns a scale (each test says which, from the kernel source).  Every case runs the fp32 form of the same call under
the same gates, and asserts that the form under test took the shape."""
import ctypes
import struct

import pytest
import torch

import h2_cases as H
from conftest import note

pytestmark = pytest.mark.gpu
TOL = H.TOL
RESTORE = (0, 34, 8, 80, 60, 74, 84, 92, 64, 96, 88, 78)     # test_conv_fwd_dgrad_wgrad's list, and the two more switches set here


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    yield afdm, ops, gpu
    for m in RESTORE:
        afdm.lib().afd_debug_conv_path(m)


def _modes(L, modes):
    for m in modes:
        L.afd_debug_conv_path(m)


def _gate(family, err, detail):
    note(family, err[0], (detail, err[1]))
    return err[0] < TOL


# ---------------------------------------------------------------------------------------------
# forward / dgrad
# ---------------------------------------------------------------------------------------------
VARIANTS = {"h2reg": (82, 61), "h2l_128x2": (82, 62), "h2l_256x1": (82, 63), "h2l_128x1": (82, 59), "h2sk": (82, 73)}
FP32_FORMS = (65, 81)


def _takes(variant, S, K, N):
    """Does the forced form take a pass with reduction width K and N output channels on an S x S map?  (h2l_launch and
    h2_sk_ok(force) in csrc/h2.hip, restated: the library has no query for the workgroup form.)"""
    if K % 32 or N % 32:
        return False
    if variant == "h2sk":
        return S in (4, 8) and K >= 64
    if S not in (8, 16, 32):
        return False
    if variant == "h2l_128x2":
        return N % 64 == 0
    if variant == "h2l_256x1":
        return S >= 16
    return True


def _conv_cases():
    out = []
    for variant in VARIANTS:
        shapes = H.SK_SHAPES if variant == "h2sk" else H.TILE_SHAPES + ([H.TILE_SHAPE_N64] if variant == "h2l_128x2" else [])
        for shape in shapes:
            S, ci, co, B = shape
            fwd, dgrad = _takes(variant, S, ci, co), _takes(variant, S, co, ci)
            if not (fwd or dgrad):
                continue                                             # (8 x 8, 96 -> 160 has no (128, 2) form either way: TILE_SHAPE_N64 stands in)
            tag = "" if fwd and dgrad else ("_fwd_only" if fwd else "_dgrad_only")
            out.append(pytest.param(variant, shape, fwd, dgrad, id=f"{variant}_{S}x{S}_{ci}to{co}_B{B}{tag}"))
    return out


def _conv_run(ops, dev, x, w, dy):
    xd = x.to(dev).requires_grad_(True)
    y = ops.conv(xd, w.to(dev))
    (gx,) = torch.autograd.grad(y, xd, dy.to(dev))
    return y.detach().cpu(), gx.cpu()


@pytest.mark.parametrize("variant,shape,fwd,dgrad", _conv_cases())
def test_conv_variants_moving_scales(A, variant, shape, fwd, dgrad):
    """k_ramp x pair_scale x {unit, 1e-25, 1e18} on every workgroup form of the forward / dgrad kernels.

    Which outputs share a scale (csrc/h2.hip): conv_h2 and conv_h2l keep ONE running scale of x per workgroup = per tile of
    128 (256) pixels: two whole 8 x 8 images, or 8 / 4 (16 / 8) rows of one 16 x 16 / 32 x 32 image; it is looked at once per
    32-channel chunk.  conv_h2_sk keeps one per WAVE = (32-pixel slice: two 4 x 4 images or four rows of an 8 x 8 image) x
    (K-slice: chunks kw, kw + KSP, ..), unscales each wave's sums by its own scale and adds them through LDS.  No scope spans
    two of pair_scale's groups (pairs on the 4 x 4 / 8 x 8 maps, single images above), and every image is whole scopes, so the
    gate is per IMAGE: an image at 2^-30 is not hidden behind its 2^+30 neighbour.  A case whose id says fwd_only / dgrad_only
    reaches the form in that direction only (N % 64, K >= 64); the other direction runs the form the library picks and is
    checked all the same."""
    afdm, ops, dev = A
    L = afdm.lib()
    S, ci, co, B = shape
    assert fwd or dgrad
    bad = []
    try:
        for tag, x, w, dy in H.conv_inputs(shape):
            y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
            for form, modes in ((variant, VARIANTS[variant]), ("fp32 forms", FP32_FORMS)):
                _modes(L, modes)
                if form == variant:
                    assert L.afd_conv3x3_weight_kinds(B, ci, co, S, S) == 3
                y, dx = _conv_run(ops, dev, x, w, dy)
                ey, ed = H.per_image(y, y64), H.per_image(dx, dx64)
                print(f"h2 scales {form:10s} {shape} {tag}: fwd {ey[0]:.2e} (image {ey[1]}) dgrad {ed[0]:.2e} (image {ed[1]})")
                ok = _gate(f"F5 h2 scales {form}: fwd per image", ey, (shape, tag))
                ok = _gate(f"F5 h2 scales {form}: dgrad per image", ed, (shape, tag)) and ok
                if not ok:
                    bad.append((form, tag, ey, ed))
    finally:
        _modes(L, RESTORE)
    assert not bad, bad


@pytest.mark.parametrize("variant,shape,fwd,dgrad", _conv_cases())
def test_conv_variants_zero_blocks(A, variant, shape, fwd, dgrad):
    """A leading all-zero chunk (the scale stays at its cap, 2^126, until data near 1e18 arrives: the carry-over factor
    underflows to 0 and must meet only zero sums) and an all-zero pair / image (a scope that never leaves the cap): outputs
    finite everywhere, exactly 0 for the all-zero scope (no bias), and the per-image gate of the test above."""
    afdm, ops, dev = A
    L = afdm.lib()
    S, ci, co, B = shape
    try:
        for tag, x, w, dy, zi in H.conv_zero_inputs(shape):
            y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
            for form, modes in ((variant, VARIANTS[variant]), ("fp32 forms", FP32_FORMS)):
                _modes(L, modes)
                if form == variant:
                    assert L.afd_conv3x3_weight_kinds(B, ci, co, S, S) == 3
                y, dx = _conv_run(ops, dev, x, w, dy)
                assert torch.isfinite(y).all() and torch.isfinite(dx).all(), (form, tag)
                assert not y[zi].any() and not dx[zi].any(), (form, tag)
                ey, ed = H.per_image(y, y64), H.per_image(dx, dx64)
                print(f"h2 zero blocks {form:10s} {shape} {tag}: fwd {ey[0]:.2e} dgrad {ed[0]:.2e}")
                assert _gate(f"F5 h2 zero blocks {form}: fwd per image", ey, (shape, tag)), (form, tag, ey)
                assert _gate(f"F5 h2 zero blocks {form}: dgrad per image", ed, (shape, tag)), (form, tag, ed)
    finally:
        _modes(L, RESTORE)


# ---------------------------------------------------------------------------------------------
# 3x3 weight gradient
# ---------------------------------------------------------------------------------------------
def _wgrad_call(A, x, dy, ks, with_bias=False, accumulate=0, fill=(float("nan"), float("nan"))):
    """afd_conv_wgrad_partials + the fold it hands back -> (dw, db, slab count of the weight fold); the workspace starts as NaN"""
    afdm, ops, dev = A
    L = afdm.lib()
    B, K, S = x.shape[0], x.shape[1], x.shape[2]
    N = dy.shape[1]
    P = lambda t: t.data_ptr()
    ws = torch.full((max(L.afd_conv_wgrad_workspace_bytes(B, K, N, S, S, ks) // 4, 1),), float("nan"), device=dev)
    dw = torch.full((N, K, ks, ks), fill[0], device=dev)
    db = torch.full((N,), fill[1], device=dev) if with_bias else None
    buf, n = ctypes.create_string_buffer(112), ctypes.c_int(-1)
    L.afd_conv_wgrad_partials(P(x), P(dy), P(dw), P(db) if with_bias else None, B, K, N, S, S, ks, accumulate, P(ws),
                              ctypes.addressof(buf), ctypes.addressof(n), ops._stream())
    assert 1 <= n.value <= 2
    slabs = struct.unpack(ops.FOLD_DESC, buf.raw[:56])[6]
    ops.fold_now(buf.raw[:56 * n.value])
    torch.cuda.synchronize()
    return dw.cpu(), (db.cpu() if with_bias else None), slabs


def _tiles_per_split(nt, slabs):
    """The fewest tiles any split can hold, given the slab count the launch reported: the plan (wgrad_bf3_plan) cuts nt
    tiles into splits of c = ceil(nt / s) for some s, and reports ceil(nt / c) slabs; the last split holds the rest."""
    cs = {-(-nt // s) for s in range(1, nt + 1) if -(-nt // -(-nt // s)) == slabs}
    assert cs, (nt, slabs)
    return min(min(c, nt - (slabs - 1) * c) for c in cs)


@pytest.mark.parametrize("which", H.WG_SETS, ids=lambda s: s.replace(" ", "_"))
@pytest.mark.parametrize("S,B", H.WG_SHAPES, ids=lambda v: str(v))
def test_wgrad3_moving_scales(A, S, B, which):
    """256 -> 256, 16 tiles of 128 pixels in 4 splits: stream_ramp over the tiles (images on the 4 x 4 / 8 x 8 maps, 128-pixel
    row bands above) on x, on dY, on both in opposite directions (the products stay level while both scales move), and a
    x 2^12 step inside the second split.

    Which outputs share a scale (csrc/h2_wgrad.hip, BN = BK = 32): a workgroup owns one 32 x 32 block (output x input
    channels, nine taps) of one split's slab.  The x scale is the workgroup's and runs over the split's tiles; the dY scale is
    each wave's (16 output channels x one of four 32-pixel steps per tile) and runs over that wave's steps; every wave
    unscales its sums by its own pair before the four step groups are added through LDS, and the splits' slabs are folded
    after.  So every element of a 32 x 32 block of dW went through the same workgroups and the gate is per block.
    Ascending inputs lower a scale tile after tile (the carry-over); descending ones leave late terms small under a scale
    set by the first."""
    afdm, ops, dev = A
    L = afdm.lib()
    C = H.WG_C
    x, dy = H.wg_inputs(S, B, which)
    dw64 = H.wgrad3_ref(x, dy, torch.float64)
    xd, dyd = x.to(dev), dy.to(dev)
    try:
        _modes(L, (86, 78))
        assert L.afd_conv_wgrad_form(B, C, C, S, S, 3) == 4
        dw, _, slabs = _wgrad_call(A, xd, dyd, 3)
        nt = B * S * S // 128
        assert nt == 16 and _tiles_per_split(nt, slabs) >= 3, (nt, slabs)    # else no scale would ever be carried over
        dw2, _, _ = _wgrad_call(A, xd, dyd, 3)
        _modes(L, (85, 97))
        dw32, _, _ = _wgrad_call(A, xd, dyd, 3)
    finally:
        _modes(L, RESTORE)
    e, e32 = H.per_block(dw, dw64), H.per_block(dw32, dw64)
    print(f"wgrad_h2 scales {S}x{S} B{B} {which}: slabs {slabs}, worst block f16x2 {e[0]:.2e} at {e[1]}, fp32 form {e32[0]:.2e} at {e32[1]}")
    ok32 = _gate("F5 h2 wgrad scales fp32 form: per 32x32 block", e32, (S, B, which))
    assert _gate("F5 h2 wgrad scales f16x2: per 32x32 block", e, (S, B, which)), e
    assert ok32, e32
    assert torch.equal(dw, dw2)


# ---------------------------------------------------------------------------------------------
# 1x1 weight gradient
# ---------------------------------------------------------------------------------------------
def _pw_plan(B, K, N, L_, target):
    """pw_wgrad_bf3_plan (csrc/bf3_wgrad.hip) restated -> (splits, fewest steps any live wave takes, NT, pixel slices)"""
    NT = 3 if N % 48 == 0 else 2
    roles = (N // (16 * NT)) * (K // 32)
    NR = 8
    while roles % NR:
        NR //= 2
    st, gy, WP = B * L_ // 32, roles // NR, 8 // NR
    s = min(target // gy, st // WP)
    s = min(max(s, 1), st)
    c = -(-st // s)
    splits = -(-st // c)
    fewest = min(-(-(min(c, st - sp * c) - wp) // WP) for sp in range(splits) for wp in range(WP))
    return splits, fewest, NT, WP


@pytest.mark.parametrize("which", H.PW_SETS, ids=lambda s: s.replace(" ", "_"))
@pytest.mark.parametrize("shape", H.PW_SHAPES, ids=lambda s: "K%d_N%d_%dx%d_B%d" % (s[0], s[1], s[2], s[2], s[3]))
def test_pointwise_wgrad_moving_scales(A, monkeypatch, shape, which):
    """afd_conv_wgrad(ksize = 1) with ONE split walking every step (AFD_PWB_TARGET = 1, read per call), stream_ramp over the
    images on x, on dY, on both opposed (over 2^16, not 2^24: PW_OPP_LO in tests/h2_cases.py says why and what the wider one
    measured), and one value 2^20 above the rest in the LAST step (x, dY): the wave that meets it
    has skipped the wave maximum on every step since its first (`lim` in pw_wgrad_h2) and must now take it, lower the
    scale and carry its sums over.

    Which outputs share a scale (pw_wgrad_h2): a wave = (role: 16 NT output x 32 input channels) x (pixel slice: steps wp,
    wp + WP, .. of the split) keeps its own scales of dY and x, unscales its sums by both and hands them to slice 0 through
    LDS.  dW is gated per 32 x 32 block as everywhere (at NT = 3 a role is 48 output channels: a block lies in one or two
    roles, each wave's fault lands in at most two blocks); in the spike cases also without the spike's column / row, which
    otherwise carries the whole norm of its blocks.  db takes the unscaled values and stays at 5e-6."""
    afdm, ops, dev = A
    L = afdm.lib()
    K, N, S, B = shape
    monkeypatch.setenv("AFD_PWB_TARGET", "1")
    splits, fewest, NT, WP = _pw_plan(B, K, N, S * S, 1)
    assert splits == 1 and fewest >= 3, (splits, fewest)
    x, dy = H.pw_inputs(shape, which)
    dw64, db64 = H.pw_ref(x, dy, torch.float64)
    xd, dyd = x.to(dev), dy.to(dev)
    try:
        _modes(L, (88, 78))
        assert L.afd_conv_wgrad_form(B, K, N, S, S, 1) == 4
        dw, db, slabs = _wgrad_call(A, xd, dyd, 1, with_bias=True)
        assert slabs == splits                                      # the launch walked the plan restated above
        dw2, db2, _ = _wgrad_call(A, xd, dyd, 1, with_bias=True)
        dwa, dba, _ = _wgrad_call(A, xd, dyd, 1, with_bias=True, accumulate=1, fill=(3.0, -2.0))
        dwn, _, _ = _wgrad_call(A, xd, dyd, 1)
        _modes(L, (89,))
        dw32, db32, _ = _wgrad_call(A, xd, dyd, 1, with_bias=True)
    finally:
        _modes(L, RESTORE)
    dw, dw2, dwa, dwn, dw32 = (t.reshape(N, K) for t in (dw, dw2, dwa, dwn, dw32))
    e, e32 = H.per_block(dw, dw64), H.per_block(dw32, dw64)
    eb, eb32 = H.rel(db, db64), H.rel(db32, db64)
    ea, eba = H.rel(dwa - 3.0, dw64), H.rel(dba + 2.0, db64)
    print(f"pw_wgrad_h2 scales {shape} {which}: NT {NT}, {WP} slices, >= {fewest} steps per wave; worst block f16x2 {e[0]:.2e} "
          f"fp32 form {e32[0]:.2e}; db {eb:.2e} | {eb32:.2e}; accumulating dw {ea:.2e} db {eba:.2e}")
    note("F10 h2 1x1 wgrad scales f16x2: db", eb, (shape, which))
    note("F10 h2 1x1 wgrad scales f16x2: accumulating dw", ea, (shape, which))
    ok32 = _gate("F10 h2 1x1 wgrad scales fp32 form: per 32x32 block", e32, (shape, which)) and eb32 < H.TOL_BIAS
    assert _gate("F10 h2 1x1 wgrad scales f16x2: per 32x32 block", e, (shape, which)), e
    assert eb < H.TOL_BIAS and ea < TOL and eba < H.TOL_BIAS, (eb, ea, eba)
    if "spike" in which:
        er = H.rel(H.pw_rest(which, shape, dw), H.pw_rest(which, shape, dw64))
        er32 = H.rel(H.pw_rest(which, shape, dw32), H.pw_rest(which, shape, dw64))
        print(f"pw_wgrad_h2 scales {shape} {which}: without the spike's line f16x2 {er:.2e} fp32 form {er32:.2e}")
        note("F10 h2 1x1 wgrad scales f16x2: beside the spike", er, (shape, which))
        assert er < TOL and er32 < TOL, (er, er32)
    assert ok32, (e32, eb32)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dw, dwn)
