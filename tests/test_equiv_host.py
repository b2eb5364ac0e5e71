"""CPU-side tests of the equivariance scores (EQ-T / EQ-R): the transform table against the maps ndimage.shift / ndimage.rotate
imply, the validity mask's pixel counts, the empty-mask error, the row layout, the dB combination on hand numbers, every
argument check of Diffusion.equivariance (all raised before a device is touched), the C ABI of the three new entry points
with their argument checks (which return before any launch), and an fp64 numpy restatement of the spline (prefilter +
interpolation, used by the GPU tests as the reference) against scipy."""
import ctypes
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, L, I, DBL = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double


def _diff(T=100, size=32):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=size, device="cpu")


def _model(c=1):
    import afdm
    return afdm.UNet(c_in=c, c_out=c, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)


# ---- the fp64 restatement of the periodic cubic spline (scipy.ndimage's order-3 'grid-wrap' arithmetic) -----------------------
POLE = math.sqrt(3.0) - 2.0


def spline3_prefilter64(x):
    """Cubic B-spline coefficients of every (H, W) plane of x, periodic, in fp64: gain 6, pole sqrt(3) - 2, causal then
    anti-causal recursion along axis -2, then along axis -1."""
    c = np.array(x, dtype=np.float64)
    for axis in (-2, -1):
        c = np.moveaxis(c, axis, -1)
        n, z = c.shape[-1], POLE
        if n > 1:
            c = c * ((1.0 - z) * (1.0 - 1.0 / z))
            zi = z ** np.arange(1, n)
            c[..., 0] = (c[..., 0] + (zi * c[..., :0:-1]).sum(-1)) / (1.0 - z ** n)
            for i in range(1, n):
                c[..., i] += z * c[..., i - 1]
            c[..., n - 1] = (c[..., n - 1] + (zi * c[..., :n - 1]).sum(-1)) * (z / (z ** n - 1.0))
            for i in range(n - 2, -1, -1):
                c[..., i] = z * (c[..., i + 1] - c[..., i])
        c = np.moveaxis(c, -1, axis)
    return np.ascontiguousarray(c)


def _weights(f):
    w0 = (1.0 - f) ** 3 / 6.0
    w1 = (f * f * (f - 2.0) * 3.0 + 4.0) / 6.0
    w2 = ((1.0 - f) ** 2 * ((1.0 - f) - 2.0) * 3.0 + 4.0) / 6.0
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]


def spline3_affine64(coef, a):
    """The spline with coefficients coef (..., H, W) at M o + off for every output pixel o, wrapped into the period, in fp64."""
    H, W = coef.shape[-2:]
    oy, ox = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    cy = np.mod(a[0] * oy + a[1] * ox + a[4], H)
    cx = np.mod(a[2] * oy + a[3] * ox + a[5], W)
    fy, fx = np.floor(cy), np.floor(cx)
    wy, wx = _weights(cy - fy), _weights(cx - fx)
    out = np.zeros(coef.shape, dtype=np.float64)
    for i in range(4):
        yy = (fy.astype(np.int64) - 1 + i) % H
        for j in range(4):
            xx = (fx.astype(np.int64) - 1 + j) % W
            out += coef[..., yy, xx] * wy[i] * wx[j]
    return out


def test_restatement_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    d = _diff()
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 32, 32))
    x /= np.abs(x).max()                                                   # unit scale
    tab = d.equivariance_transforms([("translate", 0, 0), ("translate", 0.5, 0.25), ("translate", -1.75, 3.0), ("translate", 8, 8),
                                     ("rotate", 10), ("rotate", 45), ("rotate", 90), ("rotate", -123.4)]).numpy()
    coef = spline3_prefilter64(x)
    worst = 0.0
    for a in tab:
        got = spline3_affine64(coef, a)
        for p in range(x.shape[0]):
            want = ndimage.affine_transform(x[p], a[:4].reshape(2, 2), offset=a[4:], order=3, mode="grid-wrap", output=np.float64)
            worst = max(worst, float(np.abs(got[p] - want).max()))
    print(f"fp64 restatement vs scipy.ndimage.affine_transform: worst |diff| = {worst:.2e}")
    assert worst <= 1e-13                                                  # both are fp64 spline evaluations of unit-scale data
    assert float(np.abs(spline3_affine64(coef, tab[0]) - x).max()) <= 1e-14    # the identity reproduces the samples


# ---- the transform table ------------------------------------------------------------------------------------------------------
def test_transform_table_rows():
    from afdm import ops
    d = _diff()
    specs = [("translate", 0.5, -3), ("rotate", 10), ("rotate", 90.0), ("translate", 0, 0), ["rotate", -33.3]]
    tab = d.equivariance_transforms(specs)
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (5, 6)
    assert tab[0].tolist() == [1.0, 0.0, 0.0, 1.0, -0.5, 3.0] and tab[3].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    for row, deg in ((1, 10), (2, 90.0), (4, -33.3)):
        m, off = ops.rotate_affine(deg, 32, 32)                            # what rotate_spline3_wrap passes to the kernel
        assert tab[row].tolist() == [m[0, 0], m[0, 1], m[1, 0], m[1, 1], off[0], off[1]]
        c, s = math.cos(np.deg2rad(deg)), math.sin(np.deg2rad(deg))        # ndimage.rotate: rot = [[c, s], [-s, c]], axes (2, 3)
        rot = np.array([[c, s], [-s, c]])
        ctr = np.array([15.5, 15.5])
        assert tab[row].tolist() == list(rot.ravel()) + list(ctr - rot @ ctr)
    d64 = _diff(size=64)
    assert d64.equivariance_transforms([("rotate", 90)])[0, 4:].tolist() != tab[2, 4:].tolist()     # the offset follows img_size


def test_transform_table_is_what_ndimage_shift_and_rotate_compute():
    ndimage = pytest.importorskip("scipy.ndimage")
    d = _diff()
    x = np.random.default_rng(1).standard_normal((32, 32)).astype(np.float32)
    for spec in (("translate", 0.5, 0.25), ("translate", -1.75, 3.0), ("translate", 0.0, 0.125), ("translate", 2, -5),
                 ("rotate", 10), ("rotate", 45), ("rotate", -77.0)):
        a = d.equivariance_transforms([spec])[0].numpy()
        got = ndimage.affine_transform(x, a[:4].reshape(2, 2), offset=a[4:], order=3, mode="grid-wrap")
        if spec[0] == "translate":
            want = ndimage.shift(x, spec[1:], mode="grid-wrap")
        else:
            want = ndimage.rotate(x, spec[1], reshape=False, mode="grid-wrap")
        assert np.array_equal(got, want), spec


@pytest.mark.parametrize("bad", [[], None, "rotate", [("scale", 2.0)], [("rotate",)], [("rotate", 1, 2)], [("translate", 1)],
                                 [("translate", float("nan"), 0)], [("rotate", float("inf"))], [("rotate", "x")], [(3, 1.0)],
                                 [("translate", True, 0)], [()]])
def test_transform_table_rejects(bad):
    with pytest.raises(ValueError, match="equivariance_transforms"):
        _diff().equivariance_transforms(bad)


# ---- the mask -------------------------------------------------------------------------------------------------------------------
def test_mask_counts():
    d = _diff()
    specs = [("translate", 0, 0), ("rotate", 10), ("rotate", 45), ("translate", 0.5, 0.5), ("translate", 8, 8), ("rotate", 90)]
    tab = d.equivariance_transforms(specs).numpy()
    masks = [d.equivariance_mask(a, 32, 32, 4.0) for a in tab]
    assert all(m.dtype == np.bool_ and m.shape == (32, 32) for m in masks)
    # rotate 90: cos(pi / 2) = 6e-17 in fp64 puts 18 sources of the 576 a hair outside the band; the device decides alike
    assert [int(m.sum()) for m in masks] == [576, 512, 464, 529, 256, 558]
    assert masks[0][4:28, 4:28].all() and masks[0].sum() == 24 * 24
    assert masks[4][12:28, 12:28].all()                                    # translate (8, 8): sources 4 .. 19 -> outputs 12 .. 27
    assert int(d.equivariance_mask(tab[0], 32, 32, 0).sum()) == 1024 and int(d.equivariance_mask(tab[0], 32, 32, 15).sum()) == 4
    assert int(d.equivariance_mask(tab[3], 32, 32, 0.0).sum()) == 31 * 31
    assert int(d.equivariance_mask(tab[0], 16, 48, 2.5).sum()) == 10 * 42   # 3 .. 12 and 3 .. 44


def test_empty_mask_raises_before_any_device_work():
    d, m = _diff(), _model(1)
    x = torch.zeros(2, 1, 32, 32)
    with pytest.raises(ValueError, match="leaves no pixel"):
        d.equivariance(m, x, 5, [("translate", 0, 0), ("translate", 40, 0)])
    with pytest.raises(ValueError, match="leaves no pixel"):
        d.equivariance(m, x, 5, [("rotate", 10)], margin=16)
    assert m.training and m._t_range is None


# ---- rows and the combination -------------------------------------------------------------------------------------------------
def test_rows_are_image_major_then_timestep_then_transform():
    d = _diff()
    img, j, k = d.equivariance_rows(2, 2, 3)
    assert img.tolist() == [0] * 6 + [1] * 6 and j.tolist() == [0, 0, 0, 1, 1, 1] * 2 and k.tolist() == [0, 1, 2] * 4
    assert all(v.dtype == np.int64 for v in (img, j, k))
    assert (img * 2 + j).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]   # the source field of each row
    img, j, k = d.equivariance_rows(3, 1, 1)
    assert img.tolist() == [0, 1, 2] and j.tolist() == [0, 0, 0] and k.tolist() == [0, 0, 0]


def test_combine_on_hand_numbers():
    d = _diff()
    n, J, K, C = 2, 1, 3, 2
    # elements per row: transform 0 -> 2 * 10, transform 1 -> 2 * 4, transform 2 -> 2 * 5
    sums = np.array([[20.0, 80.0, 20], [0.0, 8.0, 8], [1.0, 10.0, 10],
                     [60.0, 240.0, 20], [0.0, 24.0, 8], [3.0, 10.0, 10]])
    r = d.equivariance_combine(n, J, K, C, sums, peak=2.0)
    assert all(v.dtype == torch.float64 and v.device.type == "cpu" for v in r.values())
    assert r["count"].tolist() == [10.0, 4.0, 5.0]
    assert r["mse"].shape == (2, 1, 3) and r["mse"][:, 0].tolist() == [[1.0, 0.0, 0.1], [3.0, 0.0, 0.3]]
    assert r["power"][:, 0].tolist() == [[4.0, 1.0, 1.0], [12.0, 3.0, 1.0]]
    assert r["eq_db"].shape == (1, 3) and r["snr_db"].shape == (1, 3)
    assert math.isclose(float(r["eq_db"][0, 0]), 10 * math.log10(4.0 / 2.0), rel_tol=1e-15)
    assert math.isclose(float(r["snr_db"][0, 0]), 10 * math.log10(8.0 / 2.0), rel_tol=1e-15)
    assert r["eq_db"][0, 1] == math.inf and r["snr_db"][0, 1] == math.inf    # mse == 0
    assert math.isclose(float(r["eq_db"][0, 2]), 10 * math.log10(4.0 / 0.2), rel_tol=1e-14)
    assert math.isclose(float(r["snr_db"][0, 2]), 10 * math.log10(1.0 / 0.2), rel_tol=1e-14)
    r1 = d.equivariance_combine(n, J, K, C, sums, peak=1.0)
    assert math.isclose(float(r1["eq_db"][0, 0]), 10 * math.log10(1.0 / 2.0), rel_tol=1e-15) and torch.equal(r1["snr_db"], r["snr_db"])
    bad = sums.copy()
    bad[3, 2] = 18
    with pytest.raises(ValueError, match="same, non-zero number"):
        d.equivariance_combine(n, J, K, C, bad)


# ---- equivariance's argument checks: all before any device work ---------------------------------------------------------------
def test_equivariance_rejects_bad_requests_before_touching_a_device():
    d, m = _diff(21), _model(1)
    x = torch.zeros(2, 1, 32, 32)
    tr = [("translate", 1, 0), ("rotate", 10)]
    with pytest.raises(ValueError, match="fp32"):
        d.equivariance(m, x.double(), 5, tr)
    with pytest.raises(ValueError, match="fp32"):
        d.equivariance(m, x.numpy(), 5, tr)
    with pytest.raises(ValueError, match="must have shape"):
        d.equivariance(m, torch.zeros(1, 32, 32), 5, tr)
    with pytest.raises(ValueError, match="must have shape"):
        d.equivariance(m, torch.zeros(2, 1, 16, 16), 5, tr)
    with pytest.raises(ValueError, match="do not match"):
        d.equivariance(m, torch.zeros(2, 3, 32, 32), 5, tr)
    for t in (0, 21, -1, 2.5, True, [], [3, 0], [3, 21], [3, 2.0], "5", None):
        with pytest.raises(ValueError, match="t must be"):
            d.equivariance(m, x, t, tr)
    with pytest.raises(ValueError, match="equivariance_transforms"):
        d.equivariance(m, x, 5, [])
    with pytest.raises(ValueError, match="equivariance_transforms"):
        d.equivariance(m, x, 5, [("shear", 1.0)])
    for margin in (-1, float("nan"), float("inf"), "4", True):
        with pytest.raises(ValueError, match="margin"):
            d.equivariance(m, x, 5, tr, margin=margin)
    for peak in (0, -2.0, float("nan"), None):
        with pytest.raises(ValueError, match="peak"):
            d.equivariance(m, x, 5, tr, peak=peak)
    for batch in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="batch"):
            d.equivariance(m, x, 5, tr, batch=batch)
    with pytest.raises(ValueError, match="noise_source"):
        d.equivariance(m, x, 5, tr, noise_source="reference")
    with pytest.raises(ValueError, match="label embedding"):
        d.equivariance(m, x, 5, tr, labels=[1, 2])
    assert m.training and m._t_range is None


def test_tasks_export_equivariance_results():
    import afdm
    import modules.ddpm_tasks as mt
    assert callable(afdm.equivariance_results) and mt.equivariance_results is afdm.equivariance_results


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_equivariance_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_spline3_prefilter_wrap"] == (ctypes.c_int, [P, P, L, I, I, P])
    assert sigs["afd_affine_spline3_wrap_rows"] == (ctypes.c_int, [P, L, P, P, L, P, P, L, I, I, I, P])
    assert sigs["afd_eq_terms"] == (ctypes.c_int, [P, L, P, P, L, P, P, DBL, P, L, I, I, I, P])
    assert sigs["afd_affine_spline3_wrap"] == (ctypes.c_int, [P, P, L, I, I, P, P, P, P])       # unchanged


def test_equivariance_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_double * 8192)()
    base = ctypes.addressof(buf)
    at = lambda i: base + 8 * i                                          # 8-byte slots
    # prefilter: 2 planes of 4 x 4 (x: 16 slots, coef: 32 slots)
    with pytest.raises(afdm.AfdError, match="afd_spline3_prefilter_wrap: .*NULL"):
        lib.afd_spline3_prefilter_wrap(None, at(100), 2, 4, 4, None)
    with pytest.raises(afdm.AfdError, match="afd_spline3_prefilter_wrap: .*NULL"):
        lib.afd_spline3_prefilter_wrap(at(0), None, 2, 4, 4, None)
    for planes, H, W in ((0, 4, 4), (2, 0, 4), (2, 4, -1)):
        with pytest.raises(afdm.AfdError, match="afd_spline3_prefilter_wrap: .*positive"):
            lib.afd_spline3_prefilter_wrap(at(0), at(100), planes, H, W, None)
    for o in (at(0), at(15)):
        with pytest.raises(afdm.AfdError, match="afd_spline3_prefilter_wrap: coef must not overlap"):
            lib.afd_spline3_prefilter_wrap(at(0), o, 2, 4, 4, None)
    # rows: 2 source fields of C = 2 planes of 4 x 4 (coef: 64 slots), K = 3 (18 slots), 5 rows (out: 5 * 32 floats = 80 slots)
    coef, img, aff, k, out, g = at(0), at(100), at(200), at(300), at(400), at(600)
    args = [coef, 2, img, aff, 3, k, out, 5, 2, 4, 4, None]
    for i in (0, 2, 3, 5, 6):
        bad = list(args)
        bad[i] = None
        with pytest.raises(afdm.AfdError, match="afd_affine_spline3_wrap_rows: no pointer may be NULL"):
            lib.afd_affine_spline3_wrap_rows(*bad)
    for i, v in ((1, 0), (4, 0), (7, 0), (7, -2), (8, 0), (9, 0), (10, -4)):
        bad = list(args)
        bad[i] = v
        with pytest.raises(afdm.AfdError, match="afd_affine_spline3_wrap_rows: .*positive"):
            lib.afd_affine_spline3_wrap_rows(*bad)
    for o in (coef, at(63), img, at(104), aff, at(217), k, at(304)):
        bad = list(args)
        bad[6] = o
        with pytest.raises(afdm.AfdError, match="afd_affine_spline3_wrap_rows: out must not overlap"):
            lib.afd_affine_spline3_wrap_rows(*bad)
    # terms: the same operands, g: 5 rows of 32 floats (80 slots), out: 15 slots
    args = [coef, 2, img, aff, 3, k, g, 4.0, out, 5, 2, 4, 4, None]
    for i in (0, 2, 3, 5, 6, 8):
        bad = list(args)
        bad[i] = None
        with pytest.raises(afdm.AfdError, match="afd_eq_terms: no pointer may be NULL"):
            lib.afd_eq_terms(*bad)
    for i, v in ((1, 0), (4, -1), (9, 0), (10, 0), (11, 0), (12, 0)):
        bad = list(args)
        bad[i] = v
        with pytest.raises(afdm.AfdError, match="afd_eq_terms: .*positive"):
            lib.afd_eq_terms(*bad)
    for v in (-0.5, float("nan"), float("inf")):
        bad = list(args)
        bad[7] = v
        with pytest.raises(afdm.AfdError, match="afd_eq_terms: margin"):
            lib.afd_eq_terms(*bad)
    for o in (coef, at(63), img, aff, k, g, at(679)):
        bad = list(args)
        bad[8] = o
        with pytest.raises(afdm.AfdError, match="afd_eq_terms: out must not overlap"):
            lib.afd_eq_terms(*bad)
