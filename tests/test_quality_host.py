"""PSNR and SSIM of image pairs, host side: the C ABI's two entry points and their argument checks, the pure-torch image_quality on
cpu tensors (the oracle of tests/test_gpu_quality.py) against a brute force over windows written here in numpy, the exact
identities (a == b, symmetry, constant planes, integer sums), the region's semantics, the window, every refusal, the public names
and the eval_restoration key of ddpm_run.

The SSIM gate, derived rather than measured: a weighted moment is a sum of K^2 products of magnitude at most L^2 with weights that
add up to 1, so two summation orders differ by at most gamma = (K^2 + 2) 2^-53 L^2 each, 1.4e-14 L^2 at K = 11.  Both factors of
SSIM's numerator are bounded by the matching factors of its denominator, which are at least c1 = 1e-4 L^2 and c2 = 9e-4 L^2, so
an SSIM value moves by at most about 2 (4 gamma / c1 + 4 gamma / c2) = 1.2e-9 per implementation: the gate is 5e-9 absolute.
The pixel sums of float32 images are fp64 sums of at most 4096 non-negative terms: 1e-13 relative."""
import ctypes
import math

import numpy as np
import pytest
import torch

SSIM_GATE = 5e-9
SUM_GATE = 1e-13
ORACLE_CASES = (((2, 3, 32, 32), 11), ((1, 1, 11, 17), 11), ((1, 2, 7, 7), 7), ((2, 2, 6, 9), 1))


def _pair(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8), torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.rand(shape, generator=g) * 2 - 1, torch.rand(shape, generator=g) * 2 - 1


def _brute(a, b, win, c1, c2, region=None):
    """(out (n, C, 5), map): a loop over the windows, each window's moments one weighted sum over its K x K taps."""
    a, b, win = a.numpy().astype(np.float64), b.numpy().astype(np.float64), win.numpy()
    n, C, H, W = a.shape
    K = win.shape[0]
    Ho, Wo, half = H - K + 1, W - K + 1, (K - 1) // 2
    w2 = np.outer(win, win)
    inside = np.ones((n, H, W), dtype=bool) if region is None else np.broadcast_to(np.asarray(region) != 0, (n, H, W))
    out, ssim_map = np.zeros((n, C, 5)), np.zeros((n, C, Ho, Wo))
    d = a - b
    out[:, :, 0] = (d * d * inside[:, None]).sum((-2, -1))
    out[:, :, 1] = (np.abs(d) * inside[:, None]).sum((-2, -1))
    out[:, :, 2] = inside.sum((-2, -1))[:, None]
    for i in range(Ho):
        for j in range(Wo):
            pa, pb = a[:, :, i:i + K, j:j + K], b[:, :, i:i + K, j:j + K]
            ma, mb = (w2 * pa).sum((-2, -1)), (w2 * pb).sum((-2, -1))
            maa, mbb, mab = (w2 * pa * pa).sum((-2, -1)), (w2 * pb * pb).sum((-2, -1)), (w2 * pa * pb).sum((-2, -1))
            vaa, vbb, vab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
            s = ((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (vaa + vbb + c2))
            ssim_map[:, :, i, j] = s
            centre = inside[:, i + half, j + half][:, None]
            out[:, :, 3] += np.where(centre, s, 0.0)
            out[:, :, 4] += centre
    return out, ssim_map


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg, it, db = ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double
    want = (it, [vp, vp, lg, it, it, it, vp, it, db, db, vp, lg, vp, vp, vp])
    for name in ("afd_pair_quality_u8", "afd_pair_quality_f32"):
        assert sigs[name] == want, name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))


@pytest.mark.parametrize("fn", ("afd_pair_quality_u8", "afd_pair_quality_f32"))
def test_entry_points_reject_bad_arguments_without_a_gpu(fn):
    from afdm import AfdError, lib
    call = getattr(lib(), fn)
    f32 = fn.endswith("f32")
    win = np.full(15, 1 / 15)
    rows, C, H, W, K = 4, 3, 32, 24, 11
    # non-NULL, aligned, far apart: nothing on the device side is dereferenced before the checks pass
    good = {"a": 1 << 24, "b": 2 << 24, "planes": rows * C, "C": C, "H": H, "W": W, "win": win.ctypes.data, "K": K, "region": 3 << 24,
            "region_rows": rows, "out": 4 << 24, "map": 5 << 24}

    def bad(match, **kw):
        g = dict(good, **kw)
        with pytest.raises(AfdError, match=match):
            call(g["a"], g["b"], g["planes"], g["C"], g["H"], g["W"], g["win"], g["K"], 1e-4, 9e-4, g["region"], g["region_rows"], g["out"],
                 g["map"], None)

    for name in ("a", "b", "win", "out"):
        bad("must not be NULL", **{name: None})
    for name in ("planes", "C"):
        for v in (0, -3):
            bad("planes and C must be positive", **{name: v})
    bad("planes must be a multiple of C", planes=rows * C + 1)
    for name in ("H", "W"):
        for v in (0, 65, -1):
            bad(r"H and W must lie in \[1, 64\]", **{name: v})
    for v in (0, -1, 2, 10, 16, 17):
        bad(r"K must be odd and lie in \[1, 15\]", K=v)
    bad(r"K must be at most min\(H, W\)", K=15, W=13)
    bad(r"K must be at most min\(H, W\)", K=11, H=10)
    for v in (0, 2, rows + 1, -1):
        bad("region_rows must be 1 or planes / C", region_rows=v)
    bad("region_rows must be 1 or planes / C", region_rows=2, region=None)
    bad("out must be 8-byte aligned", out=good["out"] + 4)
    bad("ssim_map must be 8-byte aligned", map=good["map"] + 4)
    if f32:
        bad("a must be 4-byte aligned", a=good["a"] + 2)
        bad("b must be 4-byte aligned", b=good["b"] + 1)
    planes = rows * C
    ends = {"a": planes * H * W * (4 if f32 else 1), "b": planes * H * W * (4 if f32 else 1), "region": rows * H * W}
    for o in ("out", "map"):
        for name, size in ends.items():
            bad(f"must not overlap {name}", **{o: good[name] + size - 8})
            bad(f"must not overlap {name}", **{o: good[name]})
    bad("must not overlap region", out=good["region"] + H * W - 8, region_rows=1)
    bad("must not overlap each other", map=good["out"] + planes * 5 * 8 - 8)
    bad("must not overlap each other", out=good["map"] + planes * (H - K + 1) * (W - K + 1) * 8 - 8)


# ---- the window --------------------------------------------------------------------------------------------------------------------
def test_gaussian_window_sums_to_one_and_is_symmetric():
    from afdm import gaussian_window
    for size in (1, 3, 5, 7, 9, 11, 13, 15):
        for sigma in (0.5, 1.5, 4.0, None):
            w = gaussian_window(size, sigma)
            assert w.dtype == torch.float64 and tuple(w.shape) == (size,) and bool((w > 0).all())
            assert abs(math.fsum(w.tolist()) - 1.0) <= 2.0 ** -52, (size, sigma)
            assert torch.equal(w, w.flip(0)), (size, sigma)
    w = gaussian_window()
    g = np.exp(-(np.arange(11) - 5.0) ** 2 / (2 * 1.5 ** 2))
    assert np.allclose(w.numpy(), g / g.sum(), rtol=1e-15, atol=0)
    assert torch.equal(gaussian_window(5, None), torch.full((5,), 0.2, dtype=torch.float64))
    for size in (0, 2, 10, 17, -1, 11.0, True, "11"):
        with pytest.raises(ValueError, match="size must be an odd int"):
            gaussian_window(size)
    for sigma in (0, -1.0, float("nan"), float("inf"), "1.5"):
        with pytest.raises(ValueError, match="sigma must be a positive number"):
            gaussian_window(11, sigma)


# ---- the cpu path against the brute force -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.uint8, torch.float32), ids=("u8", "f32"))
@pytest.mark.parametrize("shape,K", ORACLE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"K{v}")
def test_cpu_path_against_a_brute_force_over_windows(shape, K, dtype):
    from afdm import gaussian_window, image_quality, pair_sums
    a, b = _pair(shape, dtype, 3)
    L = 255.0 if dtype == torch.uint8 else 2.0
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    win = gaussian_window(K, 1.5)
    g = torch.Generator().manual_seed(5)
    region = (torch.rand((shape[0],) + shape[2:], generator=g) < 0.4).to(torch.uint8)
    for reg in (None, region):
        want, want_map = _brute(a, b, win, c1, c2, None if reg is None else reg.numpy())
        got, got_map = pair_sums(a, b, win, c1, c2, None if reg is None else reg.unsqueeze(1), want_map=True)
        got, got_map = got.numpy(), got_map.numpy()
        assert got.shape == want.shape and got_map.shape == want_map.shape == shape[:2] + (shape[2] - K + 1, shape[3] - K + 1)
        if dtype == torch.uint8:
            assert np.array_equal(got[..., :3], want[..., :3])
        else:
            assert np.all(np.abs(got[..., :2] - want[..., :2]) <= SUM_GATE * want[..., :2]) and np.array_equal(got[..., 2], want[..., 2])
        assert np.array_equal(got[..., 4], want[..., 4])
        e_map = np.abs(got_map - want_map).max()
        e_mean = (np.abs(got[..., 3] - want[..., 3]) / np.maximum(want[..., 4], 1)).max()
        print(f"cpu path against the brute force {shape} K={K} {dtype} region={reg is not None}: map {e_map:.3e}, mean {e_mean:.3e}")
        assert e_map <= SSIM_GATE and e_mean <= SSIM_GATE
        # the dict on top of the sums
        r = image_quality(a, b, window=K, region=None if reg is None else reg.unsqueeze(1), return_map=True)
        pixels, windows = want[..., 2].sum(1), want[..., 4].sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            mse = want[..., 0].sum(1) / pixels
            assert np.allclose(r["mse"].numpy(), mse, rtol=1e-13, atol=0, equal_nan=True)
            assert np.allclose(r["mae"].numpy(), want[..., 1].sum(1) / pixels, rtol=1e-13, atol=0, equal_nan=True)
            assert np.allclose(r["psnr"].numpy(), 10 * np.log10(L * L / mse), rtol=1e-12, atol=0, equal_nan=True)
            assert np.allclose(r["ssim"].numpy(), want[..., 3].sum(1) / windows, rtol=0, atol=SSIM_GATE, equal_nan=True)
            assert np.allclose(r["ssim_channels"].numpy(), want[..., 3] / want[..., 4], rtol=0, atol=SSIM_GATE, equal_nan=True)
        assert np.array_equal(r["pixels"].numpy(), pixels) and np.array_equal(r["windows"].numpy(), windows)
        assert np.array_equal(r["ssim_map"].numpy(), got_map)
        assert set(r) == {"mse", "mae", "psnr", "ssim", "ssim_channels", "pixels", "windows", "ssim_map"}
        assert all(v.dtype == torch.float64 for v in r.values())


# ---- exact identities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (torch.uint8, torch.float32), ids=("u8", "f32"))
def test_an_image_against_itself_is_exactly_one(dtype):
    from afdm import image_quality, psnr, ssim
    for shape, K in (((2, 3, 32, 32), 11), ((1, 1, 64, 64), 15), ((1, 2, 9, 13), 3), ((1, 1, 5, 5), 1)):
        a = _pair(shape, dtype, 11)[0]
        r = image_quality(a, a.clone(), window=K, return_map=True)
        assert bool((r["ssim_map"] == 1.0).all()) and bool((r["ssim"] == 1.0).all()) and bool((r["ssim_channels"] == 1.0).all())
        assert bool((r["mse"] == 0).all()) and bool((r["mae"] == 0).all()) and bool(torch.isposinf(r["psnr"]).all())
        assert torch.equal(psnr(a, a, window=K), r["psnr"]) and torch.equal(ssim(a, a, window=K), r["ssim"])
        assert "ssim_map" not in image_quality(a, a, window=K)


@pytest.mark.parametrize("dtype", (torch.uint8, torch.float32), ids=("u8", "f32"))
def test_symmetric_in_its_two_images(dtype):
    from afdm import image_quality
    a, b = _pair((2, 3, 24, 31), dtype, 13)
    r, s = image_quality(a, b, return_map=True), image_quality(b, a, return_map=True)
    for key in r:
        assert torch.equal(r[key], s[key]), key


def test_constant_planes_have_the_closed_form():
    from afdm import image_quality
    for p, q, L in ((0.25, -0.5, 2.0), (0.75, 0.75, 2.0), (-1.0, 1.0, 2.0), (0.3, 0.1, 1.0)):
        a, b = torch.full((1, 2, 20, 17), p), torch.full((1, 2, 20, 17), q)
        p, q = float(a[0, 0, 0, 0]), float(b[0, 0, 0, 0])                 # the fp32 values
        r = image_quality(a, b, data_range=L)
        c1 = (0.01 * L) ** 2
        assert float(r["ssim"]) == pytest.approx((2 * p * q + c1) / (p * p + q * q + c1), abs=1e-12)
        if p != q:
            assert float(r["psnr"]) == pytest.approx(20 * math.log10(L / abs(p - q)), abs=1e-9)
    a, b = torch.full((1, 1, 16, 16), 200, dtype=torch.uint8), torch.full((1, 1, 16, 16), 50, dtype=torch.uint8)
    r = image_quality(a, b)
    c1 = (0.01 * 255) ** 2
    assert float(r["ssim"]) == pytest.approx((2 * 200 * 50 + c1) / (200 ** 2 + 50 ** 2 + c1), abs=1e-12)
    assert float(r["psnr"]) == pytest.approx(20 * math.log10(255 / 150), abs=1e-12) and float(r["mse"]) == 150.0 ** 2 and float(r["mae"]) == 150.0


def test_uint8_sums_are_the_integers():
    from afdm import gaussian_window, pair_sums
    a, b = _pair((3, 2, 64, 64), torch.uint8, 17)
    g = torch.Generator().manual_seed(19)
    region = (torch.rand(3, 1, 64, 64, generator=g) < 0.5).to(torch.uint8)
    d = a.long() - b.long()
    for reg in (None, region):
        out, _ = pair_sums(a, b, gaussian_window(), 6.5025, 58.5225, reg)
        m = torch.ones_like(d) if reg is None else reg.long().expand_as(d)
        assert torch.equal(out[..., 0], (d * d * m).sum((-2, -1)).double())
        assert torch.equal(out[..., 1], (d.abs() * m).sum((-2, -1)).double())
        assert torch.equal(out[..., 2], m.sum((-2, -1)).double())


# ---- the region --------------------------------------------------------------------------------------------------------------------
def test_region_counts_windows_by_their_centre_and_broadcasts():
    from afdm import image_quality
    a, b = _pair((3, 2, 32, 32), torch.float32, 23)
    full = image_quality(a, b, return_map=True)
    # one pixel: exactly the window centred on it, if there is one
    one = torch.zeros(32, 32)
    one[9, 20] = 1
    r = image_quality(a, b, region=one)
    assert torch.equal(r["pixels"], torch.full((3,), 2.0, dtype=torch.float64)) and torch.equal(r["windows"], r["pixels"])
    assert torch.equal(r["ssim_channels"], full["ssim_map"][:, :, 9 - 5, 20 - 5])
    d = a[:, :, 9, 20].double() - b[:, :, 9, 20].double()
    assert torch.allclose(r["mse"], (d * d).sum(1) / 2, rtol=1e-15, atol=0)
    border = torch.zeros(32, 32)
    border[2, 16] = 1                                        # no window is centred in the cropped border
    r = image_quality(a, b, region=border)
    assert torch.equal(r["windows"], torch.zeros(3, dtype=torch.float64)) and bool(torch.isnan(r["ssim"]).all())
    assert bool(torch.isfinite(r["psnr"]).all()) and torch.equal(r["pixels"], torch.full((3,), 2.0, dtype=torch.float64))
    # the whole image as a region is no region; one mask serves all images, in any broadcastable shape
    ones = image_quality(a, b, region=torch.ones(1, 1, 32, 32), return_map=True)
    for key in full:
        assert torch.equal(ones[key], full[key]), key
    hole = torch.zeros(32, 32, dtype=torch.uint8)
    hole[8:24, 8:24] = 1
    shared = image_quality(a, b, region=hole)
    for reg in (hole.numpy(), hole.bool().view(1, 32, 32), hole.float().expand(3, 1, 32, 32)):
        r = image_quality(a, b, region=reg)
        for key in shared:
            assert torch.equal(r[key], shared[key]), key
    assert torch.equal(shared["pixels"], torch.full((3,), 512.0, dtype=torch.float64)) and torch.equal(shared["windows"], shared["pixels"])
    assert torch.allclose(shared["ssim_channels"], full["ssim_map"][:, :, 3:19, 3:19].mean((-2, -1)), rtol=0, atol=1e-14)
    # a mask per image
    per = torch.zeros(3, 1, 32, 32)
    per[0, 0, 8:24, 8:24] = 1
    per[2] = 1
    r = image_quality(a, b, region=per)
    assert r["pixels"].tolist() == [512.0, 0.0, 2048.0] and r["windows"].tolist() == [512.0, 0.0, 968.0]
    assert float(r["psnr"][0]) == float(shared["psnr"][0]) and float(r["ssim"][2]) == float(full["ssim"][2])
    assert math.isnan(float(r["psnr"][1])) and math.isnan(float(r["ssim"][1])) and math.isnan(float(r["mse"][1]))
    assert bool(torch.isnan(r["ssim_channels"][1]).all())


def test_a_nan_stays_in_its_own_image_and_outside_a_region_out_of_the_pixel_sums():
    from afdm import image_quality
    a, b = _pair((3, 2, 16, 16), torch.float32, 29)
    clean = image_quality(a, b, window=5)
    a[1, 0, 7, 7] = float("nan")
    r = image_quality(a, b, window=5)
    for key in ("mse", "mae", "psnr", "ssim"):
        assert math.isnan(float(r[key][1])) and float(r[key][0]) == float(clean[key][0]) and float(r[key][2]) == float(clean[key][2]), key
    assert math.isnan(float(r["ssim_channels"][1, 0])) and float(r["ssim_channels"][1, 1]) == float(clean["ssim_channels"][1, 1])
    away = torch.zeros(16, 16)
    away[12:, 12:] = 1                                       # neither the pixel nor a window that holds it
    assert bool(torch.isfinite(image_quality(a, b, window=5, region=away)["psnr"]).all())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_image_quality_refuses_what_it_does_not_take():
    from afdm import image_quality
    a, b = _pair((2, 3, 16, 16), torch.float32, 31)
    u = _pair((2, 3, 16, 16), torch.uint8, 31)[0]
    for args, kw, match in (((a, b[:1]), {}, "same shape, dtype and device"), ((a, u), {}, "same shape, dtype and device"),
                            ((a, b[:, :2]), {}, "same shape, dtype and device"), ((a.double(), b.double()), {}, "uint8 or float32"),
                            ((a[0], b[0]), {}, "4-D"), ((a[:0], b[:0]), {}, "non-empty"), ((a.tolist(), b), {}, "uint8 or float32"),
                            ((torch.zeros(1, 1, 65, 8), torch.zeros(1, 1, 65, 8)), {"window": 3}, r"H and W must lie in \[1, 64\]"),
                            ((torch.zeros(1, 1, 8, 65), torch.zeros(1, 1, 8, 65)), {"window": 3}, r"H and W must lie in \[1, 64\]"),
                            ((a[..., :9], b[..., :9]), {}, "larger than min"), ((a, b), {"window": 17}, "odd int"),
                            ((a, b), {"window": 4}, "odd int"), ((a, b), {"window": torch.ones(3)}, "1-D float64"),
                            ((a, b), {"window": torch.ones(4, dtype=torch.float64)}, "odd length"),
                            ((a, b), {"window": torch.ones(17, dtype=torch.float64)}, "odd length"), ((a, b), {"sigma": 0.0}, "sigma"),
                            ((a, b), {"data_range": 0}, "data_range"), ((a, b), {"data_range": -1.0}, "data_range"),
                            ((a, b), {"data_range": float("nan")}, "data_range"), ((a, b), {"k1": -0.01}, "k1"),
                            ((a, b), {"region": torch.full((16, 16), 2)}, "region must hold 0 or 1"),
                            ((a, b), {"region": torch.full((16, 16), 0.5)}, "region must hold 0 or 1"),
                            ((a, b), {"region": torch.ones(15, 16)}, "does not broadcast"),
                            ((a, b), {"region": torch.ones(2, 3, 16, 16)}, "does not broadcast"),
                            ((a, b), {"region": torch.ones(3, 1, 16, 16)}, "does not broadcast")):
        with pytest.raises(ValueError, match=match):
            image_quality(*args, **kw)
    w = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)
    r = image_quality(a, b, window=w)                        # a window of weights is taken as it is
    assert tuple(image_quality(a, b, window=w, return_map=True)["ssim_map"].shape) == (2, 3, 14, 14) and bool(torch.isfinite(r["ssim"]).all())


# ---- the package and ddpm_run's key -----------------------------------------------------------------------------------------------
def test_public_names_and_the_eval_restoration_key():
    import afdm
    from afdm import tasks
    for name in ("gaussian_window", "image_quality", "pair_sums", "psnr", "ssim", "restoration_results"):
        assert callable(getattr(afdm, name)), name
    assert afdm.image_quality is afdm.quality.image_quality and afdm.ops.pair_quality.__doc__
    base = {"image_size": 32}
    cfg = tasks._restoration_cfg(dict(base, eval_restoration={"n": 4}))
    assert cfg == {"n": 4, "mask": "center", "factor": 4, "tasks": ("inpaint", "superres"), "steps": None, "eta": 0.0, "window": 11, "sigma": 1.5}
    cfg = tasks._restoration_cfg(dict(base, eval_restoration={"n": 2, "tasks": "superres", "factor": 16, "steps": 5, "eta": 0.5, "window": 7,
                                                              "sigma": None, "mask": "half"}))
    assert cfg["tasks"] == ("superres",) and cfg["factor"] == 16 and cfg["window"] == 7 and cfg["sigma"] is None
    for bad, match in (({}, "needs n"), ({"n": 4, "k": 3}, "needs n"), (4, "needs n"), ({"n": 0}, "n must be an int >= 1"),
                       ({"n": True}, "n must be an int >= 1"), ({"n": 2, "tasks": ("deblur",)}, "tasks must be some of"),
                       ({"n": 2, "tasks": ()}, "tasks must be some of"), ({"n": 2, "factor": 3}, "factor must be a power of two"),
                       ({"n": 2, "factor": 32}, "factor must be at most image_size / 2"), ({"n": 2, "window": 8}, "size must be an odd int"),
                       ({"n": 2, "sigma": -1}, "sigma must be a positive number"), ({"n": 2, "mask": "left"}, "mask must be"),
                       ({"n": 2, "mask": np.ones((16, 16))}, "mask must be"), ({"n": 2, "mask": np.full((32, 32), 2)}, "mask must be")):
        with pytest.raises(ValueError, match=match):
            tasks._restoration_cfg(dict(base, eval_restoration=bad))
    with pytest.raises(ValueError, match="at most 64 x 64"):
        tasks._restoration_cfg({"image_size": 128, "eval_restoration": {"n": 2}})
    centre, half = tasks._restoration_mask("center", 32), tasks._restoration_mask("half", 32)
    assert centre.dtype == np.uint8 and centre.sum() == 1024 - 256 and not centre[8:24, 8:24].any() and centre[7].all() and centre[:, 24].all()
    assert half[:, :16].all() and not half[:, 16:].any()
    own = np.zeros((32, 32), dtype=np.int64)
    own[::2] = 1
    assert np.array_equal(tasks._restoration_mask(own, 32), own) and tasks._restoration_mask(torch.from_numpy(own), 32).dtype == np.uint8
    # a malformed key fails before anything is trained or written
    with pytest.raises(ValueError, match="eval_restoration"):
        afdm.ddpm_run({"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1, "device": "cuda",
                       "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "nowhere.csv", "eval_restoration": {"n": 0}})
