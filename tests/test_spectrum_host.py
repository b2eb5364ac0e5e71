"""Power spectra of image sets, host side: the C ABI's three entry points and their argument checks, the workspace bound, the
pure-torch power_spectrum on cpu tensors (the oracle of tests/test_gpu_spectrum.py) against numpy's rfft2, Parseval, the bins,
the window, compare_spectra, the public names and the eval_spectrum key of ddpm_run."""
import ctypes

import numpy as np
import pytest
import torch

ENTRY_POINTS = ("afd_spectrum_workspace_bytes", "afd_power_spectrum_u8", "afd_power_spectrum_f32")
SHAPES = ((1, 1, 1), (1, 2, 2), (3, 5, 7), (3, 16, 16), (1, 17, 33), (2, 8, 32), (3, 32, 32), (1, 64, 64), (1, 63, 64))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg, sz, it = ctypes.c_void_p, ctypes.c_long, ctypes.c_size_t, ctypes.c_int
    tail = [lg, lg, lg, lg, vp, vp, it, vp, lg, vp, vp, vp, sz, vp]
    want = {"afd_spectrum_workspace_bytes": (sz, [lg, lg, lg, lg]), "afd_power_spectrum_u8": (it, [vp, vp] + tail),
            "afd_power_spectrum_f32": (it, [vp] + tail)}
    for name in ENTRY_POINTS:
        assert name in sigs, name
        assert sigs[name] == want[name], name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))          # exported by the library, wrapped by the binding


@pytest.mark.parametrize("fn", ("afd_power_spectrum_u8", "afd_power_spectrum_f32"))
def test_entry_points_reject_bad_arguments_before_any_launch(fn):
    from afdm import AfdError, lib
    L = lib()
    call = getattr(L, fn)
    f32 = fn.endswith("f32")
    n, C, H, W, R = 8, 3, 32, 32, 17
    Wh = W // 2 + 1
    need = L.afd_spectrum_workspace_bytes(n, C, H, W)
    assert need > 0
    # non-NULL, aligned, far apart: nothing is dereferenced before the checks pass
    good = {"images": 1 << 24, "table": 2 << 24, "n": n, "C": C, "H": H, "W": W, "win_h": 3 << 24, "win_w": 4 << 24, "remove_mean": 1,
            "bins": 5 << 24, "R": R, "power": 6 << 24, "radial": 7 << 24, "workspace": 8 << 24, "bytes": need}

    def bad(match, **kw):
        a = dict(good, **kw)
        head = (a["images"],) if f32 else (a["images"], a["table"])
        with pytest.raises(AfdError, match=match):
            call(*head, a["n"], a["C"], a["H"], a["W"], a["win_h"], a["win_w"], a["remove_mean"], a["bins"], a["R"], a["power"], a["radial"],
                 a["workspace"], a["bytes"], None)

    for name in ("images", "workspace") + (() if f32 else ("table",)):
        bad(f"{name} must not be NULL", **{name: None})
    bad("power and radial must not both be NULL", power=None, radial=None)
    bad("bins must not be NULL when radial is given", bins=None)
    for v in (0, -2):
        bad("R must be positive when radial is given", R=v)
    for name in ("n", "C"):
        for v in (0, -3):
            bad("n and C must be positive", **{name: v})
    for name in ("H", "W"):
        for v in (0, 65, -1):
            bad(r"H and W must lie in \[1, 64\]", **{name: v})
    bad(r"n must be below 2\^31", n=1 << 31, bytes=1 << 40)
    for name in ("power", "radial", "win_h", "win_w", "workspace"):
        bad(f"{name} must be 8-byte aligned", **{name: good[name] + 4})
    bad("bins must be 4-byte aligned", bins=good["bins"] + 2)
    if f32:
        bad("images must be 4-byte aligned", images=good["images"] + 2)
    else:
        bad("table must be 4-byte aligned", table=good["table"] + 1)
    bad("workspace too small", bytes=need - 1)
    bad("workspace too small", bytes=0)
    ends = {"images": n * C * H * W * (4 if f32 else 1), "win_h": H * 8, "win_w": W * 8, "bins": H * Wh * 4}
    if not f32:
        ends["table"] = C * 256 * 4
    for out in ("power", "radial", "workspace"):
        for name, size in ends.items():
            bad(f"must not overlap {name}", **{out: good[name] + size - 8})
            bad(f"must not overlap {name}", **{out: good[name]})
    bad("must not overlap each other", radial=good["power"] + C * H * Wh * 8 - 8)
    bad("must not overlap each other", workspace=good["power"] + 8)
    bad("must not overlap each other", workspace=good["radial"] - need + 8)
    # an output that is not asked for is not looked at: a NULL power, and bins / R without radial
    with pytest.raises(AfdError, match="workspace too small"):
        head = (good["images"],) if f32 else (good["images"], good["table"])
        call(*head, n, C, H, W, None, None, 0, None, 0, good["power"], None, good["workspace"], need - 8, None)


def test_workspace_is_positive_monotone_and_bounded():
    from afdm import lib
    ws = lib().afd_spectrum_workspace_bytes
    assert ws(1, 1, 1, 1) == 8
    for C, H, W in SHAPES:
        sizes = [ws(n, C, H, W) for n in (1, 2, 3, 17, 257, 1000, 50000, 10 ** 6, 2 ** 31 - 1)]
        assert all(s > 0 and s % 8 == 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[3]          # monotone in n ...
        assert sizes[-1] == sizes[-2] == sizes[-3] <= 768 * H * (W // 2 + 1) * 8             # ... up to a bound that n does not move
        assert sizes[0] == C * H * (W // 2 + 1) * 8                                           # one partial per channel for one image
    assert ws(50000, 3, 32, 32) == 256 * 3 * 32 * 17 * 8
    for bad in ((0, 1, 8, 8), (-1, 1, 8, 8), (1, 0, 8, 8), (1, 1, 0, 8), (1, 1, 8, 0), (1, 1, 65, 8), (1, 1, 8, 65), (1 << 31, 1, 8, 8),
                (1, 1 << 31, 8, 8), (1 << 30, 1 << 11, 8, 8)):
        assert ws(*bad) == 0, bad


# ---- the cpu oracle against numpy ------------------------------------------------------------------------------------------------
def _images(kind, n, chw, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "u8":
        return torch.randint(0, 256, (n,) + chw, generator=g, dtype=torch.uint8)
    return torch.randn((n,) + chw, generator=g)


def _numpy_processed(images, table, window, remove_mean):
    """The fp64 planes that are transformed: table, mean, window, as the specification words them."""
    from afdm.spectrum import hann_window
    x = images.numpy()
    n, C, H, W = x.shape
    if table is not None:
        x = np.stack([table.numpy()[c][x[:, c]] for c in range(C)], axis=1)
    x = x.astype(np.float64)
    if remove_mean:
        x = x - x.mean(axis=(-2, -1), keepdims=True)
    if window is not None:
        x = x * (hann_window(H).numpy()[:, None] * hann_window(W).numpy()[None, :])
    return x


def _m(W):
    m = np.full(W // 2 + 1, 2.0)
    m[0] = 1.0
    if W % 2 == 0:
        m[W // 2] = 1.0
    return m


@pytest.mark.parametrize("chw", SHAPES)
def test_cpu_power_spectrum_against_numpy_and_parseval(chw):
    from afdm.data import normalisation_table
    from afdm.spectrum import power_spectrum, spectrum_bins
    C, H, W = chw
    table = normalisation_table(C, mean=[0.4, 0.5, 0.6][:C], std=[0.5, 0.25, 0.3][:C])
    bins, counts, R = spectrum_bins(H, W)
    for kind in ("u8", "f32"):
        images = _images(kind, 5, chw, 7)
        tab = table if kind == "u8" else None
        for window in ("hann", None):
            for remove_mean in (True, False):
                got = power_spectrum(images, tab, window=window, remove_mean=remove_mean)
                x = _numpy_processed(images, tab, window, remove_mean)
                want = (np.abs(np.fft.rfft2(x)) ** 2).mean(0)
                power = got["power"].numpy()
                assert got["power"].dtype == torch.float64 and power.shape == (C, H, W // 2 + 1) and got["n"] == 5
                assert np.linalg.norm(power - want) <= 1e-13 * np.linalg.norm(want) + 1e-300
                assert np.all(np.abs(power - want) <= 1e-12 * want.max() + 1e-11 * want)
                # Parseval: the full spectrum's energy, the mirrored half counted, is H W times the planes' energy
                energy = (x ** 2).sum(axis=(-2, -1)).mean(0)
                assert np.allclose((power * _m(W)).sum(axis=(-2, -1)), H * W * energy, rtol=1e-12, atol=1e-12 * H * W * energy.max() + 1e-300)
                radial = np.zeros((C, R))
                for r in range(R):
                    sel = bins.numpy() == r
                    radial[:, r] = (want * _m(W))[:, sel].sum(-1) / counts[r].item()
                assert got["radial"].shape == (C, R) and np.allclose(got["radial"].numpy(), radial, rtol=1e-12, atol=1e-12 * radial.max() + 1e-300)
                assert torch.equal(got["counts"], counts)


def test_default_table_and_the_dataset_method():
    from afdm.data import DeviceDataset, normalisation_table
    from afdm.spectrum import power_spectrum
    images = _images("u8", 6, (3, 8, 8), 1)
    a, b = power_spectrum(images), power_spectrum(images, normalisation_table(3))
    assert torch.equal(a["power"], b["power"]) and torch.equal(a["radial"], b["radial"])
    ds = DeviceDataset(images, mean=[0.1, 0.2, 0.3], std=0.7, device="cpu")
    for n in (None, 4):
        for window in ("hann", None):
            got = ds.power_spectrum(window=window, remove_mean=False, n=n)
            want = power_spectrum(images[:n], ds.table, window=window, remove_mean=False)
            assert torch.equal(got["power"], want["power"]) and got["n"] == (6 if n is None else n)
    fs = DeviceDataset(images.float() / 255, device="cpu")
    assert torch.equal(fs.power_spectrum()["power"], power_spectrum(images.float() / 255)["power"])
    for bad in (0, 7, -1, 2.0, True):
        with pytest.raises(ValueError, match="power_spectrum: n must be None or an int"):
            ds.power_spectrum(n=bad)


def test_a_constant_plane_and_a_single_wave():
    from afdm.spectrum import power_spectrum
    H, W = 12, 10
    flat = torch.full((2, 1, H, W), 0.75)
    p = power_spectrum(flat, window=None, remove_mean=False)["power"][0]
    assert p[0, 0].item() == pytest.approx((0.75 * H * W) ** 2, rel=1e-14)
    rest = p.clone()
    rest[0, 0] = 0
    assert rest.abs().max().item() <= 1e-24 * p[0, 0].item()
    assert power_spectrum(flat, window=None, remove_mean=True)["power"].abs().max().item() == 0.0
    y, x = torch.arange(H, dtype=torch.float64).view(H, 1), torch.arange(W, dtype=torch.float64).view(1, W)
    for u0, v0 in ((3, 2), (0, 4), (5, 0), (9, 5), (6, 5)):
        wave = torch.cos(2 * np.pi * (u0 * y / H + v0 * x / W)).float().view(1, 1, H, W)
        p = power_spectrum(wave, window=None, remove_mean=False)["power"][0]
        # a real wave is two conjugate coefficients of H W / 2 each; where the two coincide (both indices their own mirror image)
        # it is one of H W
        own = (2 * u0) % H == 0 and (2 * v0) % W == 0
        peak = (H * W) ** 2 if own else (H * W / 2) ** 2
        assert p[u0, v0].item() == pytest.approx(peak, rel=1e-6)                   # (the wave was rounded to fp32)
        rest = p.clone()
        rest[u0, v0] = 0
        if v0 == 0 or 2 * v0 == W:                                                 # the mirror lies inside the rfft2 half as well
            assert rest[(H - u0) % H, v0].item() == pytest.approx(0.0 if own else peak, rel=1e-6)
            rest[(H - u0) % H, v0] = 0
        assert rest.max().item() <= 1e-12 * peak


@pytest.mark.parametrize("hw", ((1, 1), (2, 2), (5, 7), (16, 16), (17, 33), (8, 32), (32, 32), (64, 64), (63, 64), (64, 3)))
def test_spectrum_bins(hw):
    from afdm.spectrum import spectrum_bins
    H, W = hw
    bins, counts, R = spectrum_bins(H, W)
    Wh, M = W // 2 + 1, min(H, W)
    assert bins.dtype == torch.int32 and tuple(bins.shape) == (H, Wh) and R == M // 2 + 1
    assert counts.dtype == torch.float64 and tuple(counts.shape) == (R,)
    assert bins[0, 0] == 0 and int(bins.min()) >= -1 and int(bins.max()) == R - 1
    assert bool((counts >= 1).all())
    m = torch.from_numpy(_m(W)).view(1, Wh).expand(H, Wh)
    assert counts.sum().item() == m[bins >= 0].sum().item()                       # the kept coefficients of the full spectrum
    if M >= 4:
        assert bins[H // 2, Wh - 1] == -1 and counts.sum().item() < H * W         # the corners are left out
    for u in range(1, H):
        assert torch.equal(bins[u], bins[H - u])                                   # symmetric under u -> H - u
    # the definition, coefficient by coefficient
    for u in (0, 1 % H, H // 2, H - 1):
        for v in (0, 1 % Wh, Wh - 1):
            fu = u if u <= H // 2 else u - H
            r = int(np.floor(np.sqrt((fu * M / H) ** 2 + (v * M / W) ** 2) + 0.5))
            assert bins[u, v].item() == (r if r < R else -1), (u, v)
    for bad in ((0, 4), (4, 0), (2.0, 4), (True, 4)):
        with pytest.raises(ValueError, match="spectrum_bins"):
            spectrum_bins(*bad)


def test_hann_window():
    from afdm.spectrum import hann_window
    assert hann_window(1).tolist() == [1.0]
    assert hann_window(2).numpy() == pytest.approx([0.5, 0.5], abs=1e-15)
    w = hann_window(32)
    j = np.arange(32)
    assert w.dtype == torch.float64 and np.allclose(w.numpy(), 0.5 - 0.5 * np.cos(2 * np.pi * (j + 0.5) / 32), rtol=0, atol=1e-15)
    assert torch.allclose(w, w.flip(0), rtol=0, atol=1e-15) and w.min().item() > 0 and w.max().item() < 1
    assert w.sum().item() == pytest.approx(16.0, abs=1e-13)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError, match="hann_window"):
            hann_window(bad)


def test_compare_spectra():
    from afdm.spectrum import compare_spectra
    counts = torch.tensor([1.0, 8.0, 12.0, 16.0, 10.0])
    ref = {"radial": torch.tensor([[5.0, 4.0, 2.0, 1.0, 1.0], [7.0, 1.0, 1.0, 0.0, 2.0]], dtype=torch.float64), "counts": counts}
    gen = {"radial": torch.tensor([[50.0, 4.0, 20.0, 0.1, 1.0], [7.0, 10.0, 1.0, 3.0, 0.2]], dtype=torch.float64), "counts": counts}
    db, lsd, hf = compare_spectra(ref, gen)
    want = np.array([[10.0, 0.0, 10.0, -10.0, 0.0], [0.0, 10.0, 0.0, np.nan, -10.0]])
    assert tuple(db.shape) == (2, 5) and np.allclose(db.numpy(), want, rtol=0, atol=1e-12, equal_nan=True)
    assert lsd == pytest.approx(np.sqrt(400.0 / 7.0), rel=1e-12)                   # seven bins r >= 1 with a value, four of them +-10 dB
    # R = 5: the upper half of the band is r > 2, the energy is radial * counts with r = 0 left out
    share = lambda rad: sum(rad[c][r] * counts[r].item() for c in range(2) for r in (3, 4)) / \
        sum(rad[c][r] * counts[r].item() for c in range(2) for r in (1, 2, 3, 4))       # noqa: E731
    assert hf == pytest.approx(share(gen["radial"].tolist()) / share(ref["radial"].tolist()), rel=1e-12)
    same = compare_spectra(ref, ref)
    assert same[1] == 0.0 and same[2] == 1.0 and bool(torch.isnan(same[0][1, 3])) and int(torch.isnan(same[0]).sum()) == 1
    with pytest.raises(ValueError, match="compare_spectra: ref and gen must come from planes of one shape"):
        compare_spectra(ref, {"radial": gen["radial"][:, :4], "counts": counts[:4]})


# ---- validation and names -----------------------------------------------------------------------------------------------------------
def test_every_argument_error_names_its_argument():
    from afdm.spectrum import power_spectrum
    u8 = torch.zeros(4, 3, 8, 8, dtype=torch.uint8)
    for bad in (u8.long(), u8.double(), [[[[0]]]]):
        with pytest.raises(ValueError, match="power_spectrum: images must be a uint8 or float32 tensor"):
            power_spectrum(bad)
    for bad in (u8[0], u8[:0], u8.reshape(4, 192)):
        with pytest.raises(ValueError, match="power_spectrum: images must be a non-empty 4-D"):
            power_spectrum(bad)
    for bad in (torch.zeros(1, 1, 65, 8), torch.zeros(1, 1, 8, 65)):
        with pytest.raises(ValueError, match=r"power_spectrum: H and W must lie in \[1, 64\]"):
            power_spectrum(bad)
    for bad in ("hamming", "none", 1):
        with pytest.raises(ValueError, match="power_spectrum: window must be 'hann' or None"):
            power_spectrum(u8, window=bad)
    for bad in (torch.zeros(2, 256), torch.zeros(3, 256, dtype=torch.float64), [0.0] * 256):
        with pytest.raises(ValueError, match=r"power_spectrum: table must be a float32 tensor of shape \(3, 256\)"):
            power_spectrum(u8, bad)
    with pytest.raises(ValueError, match="power_spectrum: table goes with uint8 images only"):
        power_spectrum(u8.float(), torch.zeros(3, 256))


def test_public_names():
    import afdm
    import modules.utils as U
    from afdm import ops, spectrum, tasks
    for name in ("power_spectrum", "compare_spectra", "spectrum_bins", "hann_window"):
        assert getattr(afdm, name) is getattr(spectrum, name) is getattr(U, name)
    assert callable(ops.power_spectrum) and ops.power_spectrum is not spectrum.power_spectrum
    assert callable(U.DeviceDataset.power_spectrum)
    assert afdm.spectrum_results is tasks.spectrum_results


def test_eval_spectrum_key_check():
    from afdm.tasks import _spectrum_cfg
    p = {"gen_total": 8, "image_size": 32}
    assert _spectrum_cfg(dict(p, eval_spectrum={"n": 4})) == {"n": 4, "window": "hann"}
    assert _spectrum_cfg(dict(p, eval_spectrum={"n": 8, "window": None})) == {"n": 8, "window": None}
    for bad in ({}, {"window": "hann"}, {"n": 4, "Window": None}, {"n": 4, "window": None, "k": 2}, 4, [4]):
        with pytest.raises(ValueError, match="eval_spectrum needs n"):
            _spectrum_cfg(dict(p, eval_spectrum=bad))
    for bad in (0, 9, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="eval_spectrum n must be"):
            _spectrum_cfg(dict(p, eval_spectrum={"n": bad}))
    for bad in ("hamming", "None", 0, False):
        with pytest.raises(ValueError, match="eval_spectrum window must be"):
            _spectrum_cfg(dict(p, eval_spectrum={"n": 4, "window": bad}))
    with pytest.raises(ValueError, match="eval_spectrum takes images of at most 64 x 64"):
        _spectrum_cfg({"gen_total": 8, "image_size": 128, "eval_spectrum": {"n": 4}})
