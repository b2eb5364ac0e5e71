"""The small streaming kernels (csrc/elementwise.hip, csrc/ends.hip, the column sums) at their branch edges: sizes that take
the scalar and the vector form, the second grid-stride trip, every trip count of the unrolled batch loops with every
remainder, ragged groups of eight, clamped indices, ties.  fp64 references on the CPU; the gates are the ones the project uses
for the same op (torch.equal, 1e-6 / 2e-6 / 1e-5 relative L2).  Reductions are also gated per output element against the L2
norm of the element's own terms: a sum of signed terms can cancel to anything, so its own magnitude is no scale, and one bad
row or column must not hide in a whole-tensor norm.  Every direct call of the library writes between two sentinel bands."""
import math

import pytest
import torch
import torch.nn.functional as F

import gelu_cases as G
from conftest import check, note, rel_l2
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu
TOL = 1e-5
PAD = 4096
SENTINEL = 7.25


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    return afdm, ops, gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _s():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """`numel` floats between two bands of PAD sentinels; offset = 1 starts the view 4 bytes past a 16-byte boundary."""

    def __init__(self, numel, dev, offset=0, init=None):
        self.buf = torch.full((numel + 2 * PAD + 4,), SENTINEL, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.numel = PAD + offset, numel
        self.t = self.buf[self.lo:self.lo + numel]
        if init is not None:
            self.t.copy_(init.reshape(-1))
        assert self.t.data_ptr() % 16 == 4 * offset

    @property
    def ptr(self):
        return self.t.data_ptr()

    def intact(self, what):
        assert bool((self.buf[:self.lo] == SENTINEL).all()) and bool((self.buf[self.lo + self.numel:] == SENTINEL).all()), what
        return self.t


def sums_ok(family, got, want, scale, tol, detail):
    """Every element of a reduction: |got - want| < tol * (L2 norm of the element's terms)."""
    e = (got.double().cpu() - want.double()).abs() / scale.double().clamp_min(1e-30)
    i = int(e.argmax())
    note(f"{family} (per output, over its terms' L2 norm)", float(e.flatten()[i]), f"{detail} element {i}")
    assert float(e.max()) < tol, (family, detail, i, float(e.max()), tol)


def silu64(t):
    return t * torch.sigmoid(t)


def silu_grad64(t):
    s = torch.sigmoid(t)
    return s * (1 + t * (1 - s))


# ---------------------------------------------------------------------------------------------
# GELU: sizes and forms
# ---------------------------------------------------------------------------------------------
def test_gelu_sizes_alignment_and_tails(A):
    """gelu_fwd_k / gelu_bwd_k: n4 = n / 4 float4 elements plus an n % 4 scalar tail when every pointer is 16-byte aligned, n4 = 0
    (all scalar) otherwise.  n = 1, 3 (tail only), 4 (no tail), 5, 1027 (both).  The aligned n = 1027 run is checked against
    fp64; every other (n, alignment) must be bit-equal to its prefix: the element function does not depend on the form."""
    afdm, _, dev = A
    L = afdm.lib()
    x = torch.randn(1027, generator=_g(3)) * 3
    dy = torch.randn(1027, generator=_g(4))
    base = None
    for n in (1027, 1, 3, 4, 5):
        for off in (0, 1):
            xs, ds = Guarded(n, dev, off, x[:n]), Guarded(n, dev, off, dy[:n])
            y, dx = Guarded(n, dev, off), Guarded(n, dev, off)
            L.afd_gelu_fwd(xs.ptr, y.ptr, n, _s())
            L.afd_gelu_bwd(xs.ptr, ds.ptr, dx.ptr, n, _s())
            yc, dxc = y.intact(("gelu_fwd", n, off)).cpu(), dx.intact(("gelu_bwd", n, off)).cpu()
            xs.intact("x"), ds.intact("dy")
            if base is None:
                check("GELU fwd vs fp64 (sizes)", yc, G.gelu64(x), 1e-6, n)
                check("GELU bwd vs fp64 (sizes)", dxc, dy.double() * G.gelu_grad64(x), 1e-6, n)
                assert G.fwd_metric(yc, x)[0] < G.gate_fwd()
                base = (yc, dxc)
            else:
                assert torch.equal(yc, base[0][:n]) and torch.equal(dxc, base[1][:n]), (n, off)


@pytest.mark.parametrize("form", ["scalar", "vector"])
def test_gelu_second_grid_stride_trip(A, form):
    """gs_grid caps the grid at 32768 workgroups of 256: n = 32768 * 256 + 5 through an offset view makes the scalar loop's
    second trip, n = 4 * 32768 * 256 + 1027 the vector loop's (256 float4 elements) plus the 3-element tail.  The input tiles
    a 4099-element period: the first period is checked against fp64, the rest must be bit-equal to the tiling."""
    afdm, _, dev = A
    L = afdm.lib()
    n, off = (32768 * 256 + 5, 1) if form == "scalar" else (4 * 32768 * 256 + 1027, 0)
    P = 4099
    px = torch.randn(P, generator=_g(5)) * 3
    pdy = torch.randn(P, generator=_g(6))
    reps = -(-n // P)
    xs = Guarded(n, dev, off, px.to(dev).repeat(reps)[:n])
    ds = Guarded(n, dev, off, pdy.to(dev).repeat(reps)[:n])
    y, dx = Guarded(n, dev, off), Guarded(n, dev, off)
    L.afd_gelu_fwd(xs.ptr, y.ptr, n, _s())
    L.afd_gelu_bwd(xs.ptr, ds.ptr, dx.ptr, n, _s())
    for name, out, want in (("fwd", y, G.gelu64(px)), ("bwd", dx, pdy.double() * G.gelu_grad64(px))):
        t = out.intact((name, form))
        check(f"GELU {name} vs fp64 (second trip, first period)", t[:P].cpu(), want, 1e-6, form)
        assert torch.equal(t, t[:P].repeat(reps)[:n]), (name, form)


# ---------------------------------------------------------------------------------------------
# MaxPool2d(2)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [(2, 3), (5, 7), (7, 4), (8, 12)], ids=lambda p: f"{p[0]}x{p[1]}")
def test_maxpool2_ties_odd_planes_and_signed_zeros(A, plane):
    """maxpool2_fwd_k / maxpool2_bwd_k: floor mode (odd trailing rows and columns get no gradient), ties (the first maximum in
    scan order takes the gradient: values from {-1, 0, 1}, a constant plane, +-0.0 mixed), bit-equal to ATen."""
    afdm, ops, dev = A
    L = afdm.lib()
    H, W = plane
    B, C = 2, 4
    g = _g(H * 100 + W)
    x = torch.randint(-1, 2, (B, C, H, W), generator=g).float()
    x[0, 1] = 1.0                                                              # a constant plane
    x[1, 2] = torch.where(torch.rand(H, W, generator=g) < 0.5, 0.0, -0.0)      # signed zeros only
    x[1, 3] = torch.randn(H, W, generator=g)                                   # no ties
    xo = x.clone().requires_grad_(True)
    yo = F.max_pool2d(xo, 2)
    dy = torch.randn(yo.shape, generator=g)
    (go,) = torch.autograd.grad(yo, xo, dy)
    assert float(go[..., 2 * (H // 2):, :].abs().sum()) == 0 and float(go[..., :, 2 * (W // 2):].abs().sum()) == 0
    xd = x.to(dev).requires_grad_(True)
    yd = ops.MaxPool2.apply(xd)
    (gd,) = torch.autograd.grad(yd, xd, dy.to(dev))
    assert torch.equal(yd.detach().cpu(), yo.detach()) and torch.equal(gd.cpu(), go)
    xs, ds = Guarded(x.numel(), dev, 0, x), Guarded(dy.numel(), dev, 1, dy)
    y, dx = Guarded(dy.numel(), dev, 1), Guarded(x.numel(), dev, 1)
    L.afd_maxpool2_fwd(xs.ptr, y.ptr, B, C, H, W, _s())
    L.afd_maxpool2_bwd(xs.ptr, ds.ptr, dx.ptr, B, C, H, W, _s())
    assert torch.equal(y.intact("maxpool2_fwd").cpu().reshape(yo.shape), yo.detach())
    assert torch.equal(dx.intact("maxpool2_bwd").cpu().reshape(x.shape), go)


# ---------------------------------------------------------------------------------------------
# bilinear up2 / UpCat
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (2, 3), (7, 4), (16, 16)], ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("mode", ["filt", "bilinear"])
def test_upcat_small_and_odd_planes(A, hw, mode):
    """ops.UpCat: the upsampler writes through the concat's batch stride into its channel slice.  Planes down to one pixel
    (bil_src with scale 0, i1 == i0 at the border), odd sides, low planes that are no multiple of 4 elements; 16x16 takes the
    filtered fast path, the others up2_fwd_gen / up2_bwd_gen."""
    _, ops, dev = A
    H, W = hw
    B, C, Cs = 2, 3, 5
    g = _g(H * 10 + W)
    k = R.lowpass_kernel(math.pi / 2, 3, 2)
    lo, skip = torch.randn(B, C, H, W, generator=g), torch.randn(B, Cs, 2 * H, 2 * W, generator=g)
    lo_o, sk_o = lo.double().requires_grad_(True), skip.double().requires_grad_(True)
    up = R.filt_up2(lo_o, k.double()) if mode == "filt" else F.interpolate(lo_o, scale_factor=2, mode="bilinear", align_corners=True)
    yo = torch.cat([sk_o, up], dim=1)
    dy = torch.randn(yo.shape, generator=g)
    go = torch.autograd.grad(yo, [lo_o, sk_o], dy.double())
    lo_d, sk_d = lo.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    yd = ops.UpCat.apply(lo_d, sk_d, ops.Taps(k), mode)
    gd = torch.autograd.grad(yd, [lo_d, sk_d], dy.to(dev))
    assert torch.equal(yd.detach()[:, :Cs].cpu(), skip)                         # the neighbouring channels, bit for bit
    check(f"UpCat {mode} fwd vs fp64", yd.detach()[:, Cs:].cpu(), up.detach(), 2e-6, hw)
    check(f"UpCat {mode} bwd vs fp64", gd[0].cpu(), go[0], 2e-6, hw)
    assert torch.equal(gd[1].cpu(), dy[:, :Cs])


@pytest.mark.parametrize("hw", [(1, 1), (1, 5), (2, 3), (7, 4), (16, 16)], ids=lambda p: f"{p[0]}x{p[1]}")
def test_bilinear_direct_strided_and_guarded(A, hw):
    """afd_bilinear_up2_fwd / _bwd called directly with a batch stride wider than C planes: the other channels of the concat
    buffer and the bands around it keep their sentinel."""
    afdm, _, dev = A
    L = afdm.lib()
    H, W = hw
    B, C, Cs = 3, 3, 2
    plane = 4 * H * W
    bs = (Cs + C) * plane
    g = _g(H * 7 + W)
    x = torch.randn(B, C, H, W, generator=g)
    xo = x.double().requires_grad_(True)
    yo = F.interpolate(xo, scale_factor=2, mode="bilinear", align_corners=True)
    dy = torch.randn(B, Cs + C, 2 * H, 2 * W, generator=g)
    (go,) = torch.autograd.grad(yo, xo, dy[:, Cs:].double())
    xs = Guarded(x.numel(), dev, 1, x)
    out = Guarded(B * bs, dev, 0)
    L.afd_bilinear_up2_fwd(xs.ptr, out.ptr + 4 * Cs * plane, B, C, H, W, bs, _s())
    o = out.intact("bilinear_up2_fwd").reshape(B, Cs + C, 2 * H, 2 * W)
    assert bool((o[:, :Cs] == SENTINEL).all())
    check("bilinear fwd vs fp64 (direct, strided)", o[:, Cs:].cpu(), yo.detach(), 2e-6, hw)
    ds = Guarded(dy.numel(), dev, 0, dy)
    dx = Guarded(x.numel(), dev, 1)
    L.afd_bilinear_up2_bwd(ds.ptr + 4 * Cs * plane, dx.ptr, B, C, H, W, bs, _s())
    check("bilinear bwd vs fp64 (direct, strided)", dx.intact("bilinear_up2_bwd").cpu().reshape(x.shape), go, 2e-6, hw)


# ---------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------
COL_ROWS = (1, 7, 8, 9, 16, 17, 24, 25, 257)          # i + 8 < rows, step 16: 0, 1 and more trips; a remainder row or none


@pytest.mark.parametrize("cols", [1, 5, 16, 33])
def test_column_sums_every_trip_count(A, cols):
    """colsum_k (afd_colsum, afd_colsum_strided with stride > cols) and colsum2_k (afd_colsum2): 8 row groups, each walks its
    rows two at a time (`i + 8 < rows`, step 16) and takes a last single row (`i < rows`); columns beyond a multiple of 32 and a
    second workgroup (33 columns; 2 * 33 = 66 in colsum2: three).  accumulate 0 overwrites a pre-filled output, 1 adds."""
    afdm, _, dev = A
    L = afdm.lib()
    for rows in COL_ROWS:
        g = _g(rows * 100 + cols)
        stride = cols + 3
        wide = torch.randn(rows, stride, generator=g)
        two = torch.randn(rows, 2, cols, generator=g)
        pre = torch.randn(2, cols, generator=g)
        wd, td = Guarded(wide.numel(), dev, 1, wide), Guarded(two.numel(), dev, 1, two)
        dense = Guarded(rows * cols, dev, 0, wide[:, :cols].contiguous())
        for acc in (0, 1):
            runs = []
            for rep in range(2):
                o1, o2 = Guarded(cols, dev, 1, pre[0]), Guarded(cols, dev, 1, pre[0])
                oa, ob = Guarded(cols, dev, 1, pre[0]), Guarded(cols, dev, 0, pre[1])
                L.afd_colsum(dense.ptr, o1.ptr, rows, cols, acc, _s())
                L.afd_colsum_strided(wd.ptr, stride, o2.ptr, rows, cols, acc, _s())
                L.afd_colsum2(td.ptr, oa.ptr, ob.ptr, rows, cols, acc, _s())
                runs.append([o.intact((rows, cols, acc)).cpu() for o in (o1, o2, oa, ob)])
            assert all(torch.equal(a, b) for a, b in zip(*runs)), (rows, cols, acc)        # deterministic
            assert torch.equal(runs[0][0], runs[0][1])                                      # same kernel, same order
            terms = [wide[:, :cols], wide[:, :cols], two[:, 0], two[:, 1]]
            pres = [pre[0], pre[0], pre[0], pre[1]]
            for name, got, t, p in zip(("colsum", "colsum_strided", "colsum2 a", "colsum2 b"), runs[0], terms, pres):
                want = t.double().sum(0) + (p.double() if acc else 0)
                scale = (t.double().pow(2).sum(0) + (p.double().pow(2) if acc else 0)).sqrt()
                sums_ok(name, got, want, scale, 1e-6, (rows, cols, acc))
                if cols >= 16:            # (one or five sums of signed values can cancel: their own norm is no scale for 1e-6)
                    check(f"{name} vs fp64", got, want, 1e-6, (rows, cols, acc))


# ---------------------------------------------------------------------------------------------
# SiLU -> Linear
# ---------------------------------------------------------------------------------------------
SL_B = (1, 8, 9, 24, 25, 33, 57)           # dW: `b + 24 < B` step 32 -> 0, 1, 2 trips (B <= 32, 33, 57) then `b < B` step 8;
SL_N = (1, 7, 8, 9, 24, 33)                # bias row: `b + 8 < B` step 16 -> 0, 1, 2+ trips; N: ragged groups of 8, second 32-block


def _silu_case(B, K, N, has_bias):
    g = _g(B * 10000 + K * 100 + N)
    temb = torch.randn(B, K, generator=g)
    temb[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0])              # must stay finite
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g) if has_bias else None
    dout = torch.randn(B, N, generator=g)
    t, wd, dd = temb.double(), w.double(), dout.double()
    a, ag = silu64(t), silu_grad64(t)
    want = {"out": a @ wd.T + (bias.double() if has_bias else 0), "dw": dd.T @ a, "db": dd.sum(0), "dtemb": (dd @ wd) * ag}
    scale = {"out": ((a * a) @ (wd * wd).T + (bias.double() ** 2 if has_bias else 0)).sqrt(), "dw": ((dd * dd).T @ (a * a)).sqrt(),
             "db": (dd * dd).sum(0).sqrt(), "dtemb": ((dd * dd) @ (wd * wd)).sqrt() * ag.abs()}
    return temb, w, bias, dout, want, scale


@pytest.mark.parametrize("K", [32, 100, 256])
def test_silu_linear_every_batch_loop_trip(A, K):
    """silu_linear_fwd_k, silu_linear_dw_k (with its bias row block) and silu_linear_dx_k, called directly: every trip count of
    the two unrolled batch loops with every remainder, ragged groups of eight outputs, K below and beyond a 32-column block and a
    64-lane stride, bias present and absent, accumulate 0 and 1; dtemb adds into its buffer."""
    afdm, _, dev = A
    L = afdm.lib()
    for B in SL_B:
        for N in SL_N:
            if N > (K + 31) // 32 * 32:
                continue
            for has_bias in (True, False):
                temb, w, bias, dout, want, scale = _silu_case(B, K, N, has_bias)
                tag = (B, K, N, has_bias)
                ts, ws, ds = Guarded(B * K, dev, 1, temb), Guarded(N * K, dev, 1, w), Guarded(B * N, dev, 1, dout)
                bs = Guarded(N, dev, 1, bias) if has_bias else None
                out = Guarded(B * N, dev, 1)
                L.afd_silu_linear_fwd(ts.ptr, ws.ptr, bs.ptr if has_bias else None, out.ptr, B, K, N, _s())
                o = out.intact(("silu_linear_fwd", tag)).cpu().reshape(B, N)
                assert bool(torch.isfinite(o).all())
                check("SiLU->Linear fwd vs fp64", o, want["out"], TOL, tag)
                sums_ok("SiLU->Linear fwd", o, want["out"], scale["out"], TOL, tag)
                for acc in (0, 1):
                    dw = Guarded(N * K, dev, 1, torch.full((N * K,), 0.5))
                    db = Guarded(N, dev, 1, torch.full((N,), -0.25)) if has_bias else None
                    dt = Guarded(B * K, dev, 1, torch.full((B * K,), 0.125))
                    L.afd_silu_linear_bwd(ts.ptr, ws.ptr, ds.ptr, dw.ptr, db.ptr if has_bias else None, dt.ptr, B, K, N, acc, _s())
                    gw = dw.intact(("dw", tag, acc)).cpu().reshape(N, K)
                    gt = dt.intact(("dtemb", tag, acc)).cpu().reshape(B, K)
                    assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gt).all())
                    check("SiLU->Linear dW vs fp64", gw, want["dw"] + 0.5 * acc, TOL, (tag, acc))
                    sums_ok("SiLU->Linear dW", gw, want["dw"] + 0.5 * acc, (scale["dw"] ** 2 + 0.25 * acc).sqrt(), TOL, (tag, acc))
                    check("SiLU->Linear dtemb vs fp64", gt, want["dtemb"] + 0.125, TOL, (tag, acc))
                    sums_ok("SiLU->Linear dtemb", gt, want["dtemb"] + 0.125, (scale["dtemb"] ** 2 + 0.125 ** 2).sqrt(), TOL, (tag, acc))
                    if has_bias:
                        gb = db.intact(("db", tag, acc)).cpu()
                        if N >= 16:       # (a few sums of signed values can cancel, as in the column sums: measured 1.3e-5 at N = 1
                            #                where db = 0.02 is what is left of 25 terms of norm 5; per output it is 3e-7)
                            check("SiLU->Linear dbias vs fp64", gb, want["db"] - 0.25 * acc, TOL, (tag, acc))
                        sums_ok("SiLU->Linear dbias", gb, want["db"] - 0.25 * acc, (scale["db"] ** 2 + 0.0625 * acc).sqrt(), TOL, (tag, acc))
                for s in (ts, ws, ds):
                    s.intact(("inputs", tag))


def test_silu_linear_autograd_and_documented_refusal(A):
    afdm, ops, dev = A
    for has_bias in (True, False):
        temb, w, bias, dout, want, _ = _silu_case(57, 100, 33, has_bias)
        dl = [t.to(dev).requires_grad_(True) for t in (temb, w, bias) if t is not None]
        yd = ops.SiluLinear.apply(dl[0], dl[1], dl[2] if has_bias else None)
        gd = torch.autograd.grad(yd, dl, dout.to(dev))
        check("SiLU->Linear fwd vs fp64", yd.detach().cpu(), want["out"], TOL, ("ops", has_bias))
        for name, a in zip(("dtemb", "dw", "db"), gd):
            check(f"SiLU->Linear {name} vs fp64 (ops)", a.cpu(), want[name], TOL, has_bias)
    # the bias row rides in the dW grid, which has ceil(K / 32) column blocks: a bias with more 32-blocks than that is refused
    temb, w, bias, dout, _, _ = _silu_case(3, 32, 33, True)
    dl = [t.to(dev).requires_grad_(True) for t in (temb, w, bias)]
    yd = ops.SiluLinear.apply(*dl)
    with pytest.raises(afdm.AfdError, match="N > K is not covered"):
        torch.autograd.grad(yd, dl, dout.to(dev))


# ---------------------------------------------------------------------------------------------
# the batched forward and the gather of tabulated rows
# ---------------------------------------------------------------------------------------------
WIDTHS = (3, 8, 13, 64, 128, 256, 5, 1)


def _layers(n, K, g):
    ws = [torch.randn(N, K, generator=g) / math.sqrt(K) for N in WIDTHS[:n]]
    bs = [None if i % 3 == 1 else torch.randn(N, generator=g) for i, N in enumerate(WIDTHS[:n])]
    return ws, bs


@pytest.mark.parametrize("n_layers", [1, 2, 6, 8])
@pytest.mark.parametrize("K", [100, 256])
def test_silu_linear_batched_layer_sets(A, n_layers, K):
    """silu_linear_fwd_batched_k: a wave owns eight consecutive outputs of the concatenated row, so with widths (3, 8, 13, ...)
    a group straddles up to three layers and the last group is ragged (3 -> one group of 3; 3 + 8 -> 11; ... + 5 + 1 -> 478);
    every second-of-three layer has no bias.  Each layer against fp64."""
    _, ops, dev = A
    g = _g(n_layers * 1000 + K)
    B = 5
    temb = torch.randn(B, K, generator=g)
    temb[0, :4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    ws, bs = _layers(n_layers, K, g)
    outs = ops.silu_linear_batched(temb.to(dev), [(w.to(dev), None if b is None else b.to(dev)) for w, b in zip(ws, bs)])
    assert len(outs) == n_layers
    a = silu64(temb.double())
    for i, (o, w, b) in enumerate(zip(outs, ws, bs)):
        want = a @ w.double().T + (0 if b is None else b.double())
        scale = ((a * a) @ (w.double() ** 2).T + (0 if b is None else b.double() ** 2)).sqrt()
        assert tuple(o.shape) == (B, WIDTHS[i]) and bool(torch.isfinite(o).all())
        check("SiLU->Linear batched fwd vs fp64", o.cpu(), want, TOL, (n_layers, K, i))
        sums_ok("SiLU->Linear batched fwd", o.cpu(), want, scale, TOL, (n_layers, K, i))


def test_silu_linear_batched_rows_do_not_depend_on_the_batch_and_nine_layers_raise(A):
    """The tabulated sampling path computes every timestep's row once (B = 1000) and gathers: a row's result must not depend on
    the batch it sits in."""
    afdm, ops, dev = A
    g = _g(77)
    K = 256
    temb = torch.randn(1000, K, generator=g).to(dev)
    ws, bs = _layers(8, K, g)
    layers = [(w.to(dev), None if b is None else b.to(dev)) for w, b in zip(ws, bs)]
    full = ops.silu_linear_batched(temb, layers)
    rows = torch.tensor([0, 1, 7, 8, 499, 998, 999], device=dev)
    part = ops.silu_linear_batched(temb[rows].contiguous(), layers)
    for f, p in zip(full, part):
        assert torch.equal(f[rows], p)
    one = ops.silu_linear_batched(temb[999:1000].contiguous(), layers)
    assert all(torch.equal(f[999:1000], o) for f, o in zip(full, one))
    with pytest.raises(afdm.AfdError, match="1..8 layers"):
        ops.silu_linear_batched(temb[:2].contiguous(), layers + layers[:1])


@pytest.mark.parametrize("n_tables", [1, 3, 8])
def test_gather_rows_batched_clamps_and_copies(A, n_tables):
    """gather_rows_batched_k: out_i[b] = table_i[clamp(idx[b], 0, rows - 1)] (the header states the clamp), tables of odd widths
    found by their offsets in the concatenated row; bit copies."""
    afdm, ops, dev = A
    g = _g(n_tables)
    rows = 37
    tables = [torch.randn(rows, N, generator=g) for N in (7, 1, 33, 5, 64, 3, 129, 9)[:n_tables]]
    td = [t.to(dev) for t in tables]
    for B in (1, 7, 300):
        idx = torch.randint(0, rows, (B,), generator=g)
        edge = torch.tensor([0, rows - 1, -1, rows, -(2 ** 40), 2 ** 40, rows + 5])
        idx[:min(B, 7)] = edge[:min(B, 7)] if B > 1 else edge[2:3]
        outs = ops.gather_rows_batched(idx.to(dev), td)
        for o, t in zip(outs, tables):
            assert torch.equal(o.cpu(), t[idx.clamp(0, rows - 1)]), (n_tables, B)
    idx = torch.tensor([rows], device=dev)                                      # B = 1 at the upper edge too
    assert all(torch.equal(o.cpu(), t[rows - 1:rows]) for o, t in zip(ops.gather_rows_batched(idx, td), tables))
    if n_tables == 8:
        with pytest.raises(afdm.AfdError, match="1..8 tables"):
            ops.gather_rows_batched(idx, td + td[:1])


# ---------------------------------------------------------------------------------------------
# the output end: 1x1 convolutions with <= 4 output channels (csrc/ends.hip)
# ---------------------------------------------------------------------------------------------
def _ends_case(afdm, ops, dev, B, Cin, Cout, H, W, offset=0, images=None, seed=0):
    """ops.conv(x, w, bias) forward and dgrad against fp64, by the rule (outc_fwd_k / outc_dgrad_k when HW % 4 == 0 and the
    pointers are 16-byte aligned) and with those kernels switched off (afd_debug_conv_path 93)."""
    g = _g(seed + B * 1000 + Cin * 10 + Cout + H)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) / math.sqrt(Cin)
    bias = torch.randn(Cout, generator=g)
    dy = torch.randn(B, Cout, H, W, generator=g)
    sel = slice(None) if images is None else torch.tensor(images)
    xo = x[sel].double().requires_grad_(True)
    yo = F.conv2d(xo, w.double(), bias.double())
    (go,) = torch.autograd.grad(yo, xo, dy[sel].double())
    xb = torch.zeros(x.numel() + 8, device=dev)
    db = torch.zeros(dy.numel() + 8, device=dev)
    xv, dv = xb[offset:offset + x.numel()].view(x.shape), db[offset:offset + dy.numel()].view(dy.shape)
    xv.copy_(x), dv.copy_(dy)
    assert xv.data_ptr() % 16 == 4 * offset and xv.is_contiguous() and dv.is_contiguous()
    wd, bd = w.to(dev), bias.to(dev)
    tag = (B, Cin, Cout, H, W, offset)
    for path, mode in (("rule", 92), ("ends off", 93)):
        afdm.lib().afd_debug_conv_path(mode)
        try:
            xd = xv.detach().requires_grad_(True)
            yd = ops.conv(xd, wd, bd)
            (gd,) = torch.autograd.grad(yd, xd, dv)
        finally:
            afdm.lib().afd_debug_conv_path(92)
        check(f"outc 1x1 fwd vs fp64 [{path}]", yd.detach()[sel].cpu(), yo.detach(), TOL, tag)
        check(f"outc 1x1 dgrad vs fp64 [{path}]", gd[sel].cpu(), go, TOL, tag)
        for i in range(yo.shape[0]):                                           # per image: a bad tile must not hide in the batch
            assert rel_l2(yd.detach()[sel][i].cpu(), yo.detach()[i]) < TOL and rel_l2(gd[sel][i].cpu(), go[i]) < TOL, (tag, path, i)


@pytest.mark.parametrize("Cout", [1, 2, 3, 4])
def test_output_end_1x1_channel_counts_and_ragged_grids(A, Cout):
    """outc_fwd_k<COUT> / outc_dgrad_k<COUT> at every COUT; Cin below, at and beyond the weight loop's unroll of 4 and the LDS
    copy's 256-thread stride; B * HW / 4 = 3, 27, 192 float4 pixels: never a multiple of the 256-thread workgroup."""
    afdm, ops, dev = A
    for Cin in (1, 5, 32, 33):
        for S in (2, 6, 16):
            _ends_case(afdm, ops, dev, 3, Cin, Cout, S, S)


def test_output_end_1x1_falls_back_when_not_vectorisable(A):
    """HW % 4 != 0 (3x3 planes) and a 4-byte-offset input / gradient: ends_fwd / ends_dgrad decline, the general kernels serve
    the layer, with scalar accesses."""
    afdm, ops, dev = A
    _ends_case(afdm, ops, dev, 3, 5, 3, 3, 3)
    _ends_case(afdm, ops, dev, 3, 5, 3, 6, 6, offset=1)
    _ends_case(afdm, ops, dev, 2, 33, 4, 16, 16, offset=1)


def test_output_end_1x1_second_grid_stride_trip(A):
    """The grid is capped at 4096 workgroups of 256 threads x 4 pixels: 65 planes of 256x256 are 4 259 840 pixels, so image 64
    is served by the second trip.  Images 0, 63 and 64 against fp64."""
    afdm, ops, dev = A
    assert 65 * 256 * 256 > 4 * 4096 * 256
    _ends_case(afdm, ops, dev, 65, 2, 3, 256, 256, images=[0, 63, 64])
