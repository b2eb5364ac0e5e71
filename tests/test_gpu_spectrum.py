"""Power spectra on the GPU: afd_power_spectrum_u8 / afd_power_spectrum_f32 through the C ABI and through power_spectrum /
DeviceDataset.power_spectrum, against the pure-torch fp64 rfft2 on the cpu (pinned to numpy by tests/test_spectrum_host.py), and
ddpm_run with params["eval_spectrum"] and spectrum_results on its checkpoint.

Gates: rel-L2 of power and of radial below 1e-12, and per coefficient |got - want| <= 1e-12 max(want) + 1e-11 want.  An fp64
matrix-form DFT with sequential accumulation, written in numpy as a stand-in for the kernel, reached 4e-16 rel-L2 and 3e-14 per
coefficient (on the smooth images) on this grid, except for the DC coefficient after mean removal, whose true value is 0: hence
the max(want) term.  The gates keep about three orders of margin over that for another summation order and the device's
sin / cos; any fp32 step (1e-7 or worse) fails them."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import note, rel_l2

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1, 1), (1, 2, 2), (3, 5, 7), (3, 16, 16), (1, 17, 33), (2, 8, 32), (3, 32, 32), (1, 64, 64), (1, 63, 64))
NS = (1, 3, 257)
SETTINGS = (("hann", True), ("hann", False), (None, True), (None, False))
REL_L2, ABS_MAX, REL_EACH = 1e-12, 1e-12, 1e-11
CANARY = -7777.0


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _u8(shape, seed, values=None):
    g = torch.Generator().manual_seed(seed)
    if values is None:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.tensor(values, dtype=torch.uint8)[torch.randint(0, len(values), shape, generator=g)]


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _smooth(shape, seed):
    """White noise shaped by 1 / (1e-3 + f^2), f in cycles per pixel: the power falls by five decades from DC to the corner."""
    H, W = shape[-2:]
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    fu, fv = torch.fft.fftfreq(H, dtype=torch.float64).view(H, 1), torch.fft.fftfreq(W, dtype=torch.float64).view(1, W)
    x = torch.fft.ifft2(torch.fft.fft2(noise) / (1e-3 + fu * fu + fv * fv)).real
    return (x / x.abs().amax()).float()


def _gates(family, got, want, detail):
    """got, want: fp64 tensors of one shape.  Notes the rel-L2 and the per-coefficient error over its allowance, then asserts."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape and got.dtype == torch.float64, detail
    e = rel_l2(got, want)
    allow = ABS_MAX * want.max() + REL_EACH * want
    each = float(((got - want).abs() / allow.clamp_min(1e-300)).max()) if float(want.max()) > 0 else float((got - want).abs().max())
    print(f"{family} {detail}: rel-L2 {e:.3e}, worst |got - want| / allowance {each:.3e}")
    note(f"spectrum {family} rel-L2 (gate 1e-12)", e, detail)
    note(f"spectrum {family} per-coefficient error / allowance (gate 1)", each, detail)
    assert e < REL_L2, (family, detail, e)
    assert bool(((got - want).abs() <= allow).all()), (family, detail, each)


def _abi(afdm, images, table, win_h, win_w, remove_mean, bins, R, fill=0xFF, want_power=True, ws_fill=None):
    """The C ABI with raw pointers.  Outputs sit inside longer buffers whose other elements must come back untouched; the workspace
    is pre-filled with the byte `fill` (or with ws_fill, a uint8 tensor to copy from)."""
    L = afdm.lib()
    n, C, H, W = images.shape
    Wh = W // 2 + 1
    dev = images.device
    need = L.afd_spectrum_workspace_bytes(n, C, H, W)
    assert 0 < need <= 64 << 20
    ws = torch.full((need + 64,), fill, device=dev, dtype=torch.uint8)
    if ws_fill is not None:
        ws.copy_(ws_fill[:need + 64])
    power = torch.full((C * H * Wh + 32,), CANARY, device=dev, dtype=torch.float64) if want_power else None
    radial = torch.full((C * R + 32,), CANARY, device=dev, dtype=torch.float64) if bins is not None else None
    p = afdm.ops._p
    tail = (n, C, H, W, p(win_h), p(win_w), int(remove_mean), p(bins), R if bins is not None else 0, p(power), p(radial), ws.data_ptr(), need,
            afdm.ops._stream())
    if images.dtype == torch.uint8:
        L.afd_power_spectrum_u8(images.data_ptr(), table.data_ptr(), *tail)
    else:
        L.afd_power_spectrum_f32(images.data_ptr(), *tail)
    assert bool((ws[need:] == (fill if ws_fill is None else ws_fill[need:need + 64].to(dev))).all())
    if power is not None:
        assert bool((power[C * H * Wh:] == CANARY).all())
        power = power[:C * H * Wh].view(C, H, Wh)
    if radial is not None:
        assert bool((radial[C * R:] == CANARY).all())
        radial = radial[:C * R].view(C, R)
    return power, radial


def _device_args(afdm, dev, H, W, window):
    bins, counts, R = afdm.spectrum_bins(H, W)
    wh = afdm.hann_window(H).to(dev) if window else None
    ww = afdm.hann_window(W).to(dev) if window else None
    return wh, ww, bins.to(dev), counts, R


# ---- 1. the grid against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", SHAPES)
def test_the_grid_against_the_cpu_oracle(A, chw):
    """Every n, both element types, two kinds of data each, window and mean removal on and off: the C ABI with the workspace
    pre-filled with 0xFF and with 0x00, and power_spectrum / DeviceDataset.power_spectrum."""
    afdm, dev = A
    C, H, W = chw
    table = afdm.data.normalisation_table(C, mean=[0.4, 0.5, 0.6][:C], std=[0.5, 0.25, 0.3][:C])
    for n in NS:
        sets = {"u8 random": _u8((n,) + chw, 100 + n), "u8 0/127/128/255": _u8((n,) + chw, 200 + n, (0, 127, 128, 255)),
                "f32 randn": _randn((n,) + chw, 300 + n), "f32 smooth": _smooth((n,) + chw, 400 + n)}
        for kind, images in sets.items():
            u8 = images.dtype == torch.uint8
            tab = table if u8 else None
            on_dev, tab_dev = images.to(dev), table.to(dev) if u8 else None
            store = afdm.DeviceDataset(images, mean=[0.4, 0.5, 0.6][:C], std=[0.5, 0.25, 0.3][:C], device=dev) if u8 else None
            for window, remove_mean in SETTINGS:
                detail = f"{chw} n={n} {kind} window={window} remove_mean={remove_mean}"
                want = afdm.power_spectrum(images, tab, window=window, remove_mean=remove_mean)
                wh, ww, bins, counts, R = _device_args(afdm, dev, H, W, window)
                first = None
                for fill in (0xFF, 0x00):
                    power, radial = _abi(afdm, on_dev, tab_dev, wh, ww, remove_mean, bins, R, fill=fill)
                    _gates("power (C ABI)", power, want["power"], detail)
                    _gates("radial (C ABI)", radial.cpu() / counts, want["radial"], detail)
                    if first is None:
                        first = (power, radial)
                    assert torch.equal(first[0], power) and torch.equal(first[1], radial), detail
                got = store.power_spectrum(window=window, remove_mean=remove_mean) if u8 else \
                    afdm.power_spectrum(on_dev, window=window, remove_mean=remove_mean)
                assert got["power"].is_cuda and got["n"] == n and torch.equal(got["counts"].cpu(), want["counts"])
                assert torch.equal(got["power"], first[0]) and torch.equal(got["radial"], first[1] / counts.to(dev)), detail
                _gates("power (Python)", got["power"], want["power"], detail)
                _gates("radial (Python)", got["radial"], want["radial"], detail)


@pytest.mark.parametrize("n,chw", ((1001, (3, 8, 8)), (2050, (1, 4, 6)), (2, (1500, 2, 3))))
def test_slices_of_several_images_and_more_channels_than_workgroups(A, n, chw):
    """n above the number of slices (256 for three channels, 768 for one), so a workgroup walks several images and the last slice
    is short; C above 768, so every channel has one workgroup that walks all images."""
    afdm, dev = A
    images = _u8((n,) + chw, 5)
    for window, remove_mean in SETTINGS[:2]:
        want = afdm.power_spectrum(images, window=window, remove_mean=remove_mean)
        got = afdm.power_spectrum(images.to(dev), window=window, remove_mean=remove_mean)
        _gates("power (slices)", got["power"], want["power"], f"{chw} n={n}")
        _gates("radial (slices)", got["radial"], want["radial"], f"{chw} n={n}")
    f32 = _smooth((n,) + chw, 6)
    _gates("power (slices)", afdm.power_spectrum(f32.to(dev))["power"], afdm.power_spectrum(f32)["power"], f"{chw} n={n} f32")


# ---- 2. the same bits from call to call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,chw", ((257, (3, 32, 32)), (3, (1, 63, 64)), (1000, (2, 5, 7))))
def test_two_calls_give_equal_bits_whatever_the_workspace_held(A, n, chw):
    afdm, dev = A
    C, H, W = chw
    wh, ww, bins, counts, R = _device_args(afdm, dev, H, W, "hann")
    table = afdm.data.normalisation_table(C).to(dev)
    for images in (_u8((n,) + chw, 11).to(dev), _randn((n,) + chw, 12).to(dev)):
        tab = table if images.dtype == torch.uint8 else None
        need = afdm.lib().afd_spectrum_workspace_bytes(n, C, H, W)
        junk = torch.randint(0, 256, (need + 64,), generator=torch.Generator().manual_seed(13), dtype=torch.uint8).to(dev)
        runs = [_abi(afdm, images, tab, wh, ww, True, bins, R, fill=0xFF), _abi(afdm, images, tab, wh, ww, True, bins, R, fill=0x00),
                _abi(afdm, images, tab, wh, ww, True, bins, R, ws_fill=junk), _abi(afdm, images, tab, wh, ww, True, bins, R, fill=0xFF)]
        for power, radial in runs[1:]:
            assert torch.equal(power.view(torch.int64), runs[0][0].view(torch.int64))
            assert torch.equal(radial.view(torch.int64), runs[0][1].view(torch.int64))
        # one output at a time: the same bits
        only_radial = _abi(afdm, images, tab, wh, ww, True, bins, R, want_power=False)
        only_power = _abi(afdm, images, tab, wh, ww, True, None, 0)
        assert only_radial[0] is None and torch.equal(only_radial[1].view(torch.int64), runs[0][1].view(torch.int64))
        assert only_power[1] is None and torch.equal(only_power[0].view(torch.int64), runs[0][0].view(torch.int64))
        got = afdm.ops.power_spectrum(images, tab, wh, ww, True, bins, R, want_power=False)
        assert got[0] is None and torch.equal(got[1], runs[0][1])
        got = afdm.ops.power_spectrum(images, tab, wh, ww, True)
        assert got[1] is None and torch.equal(got[0], runs[0][0])


# ---- 3. views that start inside an allocation ----------------------------------------------------------------------------------------
def _offset_view(t, dev, skip_bytes):
    """A contiguous copy of t on the device that starts skip_bytes into its allocation."""
    flat = t.contiguous().view(-1).view(torch.uint8)
    buf = torch.empty(flat.numel() + 64, device=dev, dtype=torch.uint8)
    view = buf[skip_bytes:skip_bytes + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == skip_bytes
    return view.view(t.dtype).view(t.shape)


@pytest.mark.parametrize("chw", ((3, 5, 7), (3, 32, 32)))
def test_images_that_start_inside_their_allocation(A, chw):
    afdm, dev = A
    C, H, W = chw
    n = 17
    wh, ww, bins, counts, R = _device_args(afdm, dev, H, W, "hann")
    table = afdm.data.normalisation_table(C).to(dev)
    for images, skip in ((_u8((n,) + chw, 21), 1), (_randn((n,) + chw, 22), 4)):
        tab = table if images.dtype == torch.uint8 else None
        want = afdm.power_spectrum(images, None, window="hann", remove_mean=True)
        aligned = _abi(afdm, images.to(dev), tab, wh, ww, True, bins, R)
        moved = _abi(afdm, _offset_view(images, dev, skip), tab, wh, ww, True, bins, R)
        assert torch.equal(moved[0], aligned[0]) and torch.equal(moved[1], aligned[1])
        _gates("power (offset view)", moved[0], want["power"], f"{chw} skip={skip}")
        got = afdm.power_spectrum(_offset_view(images, dev, skip))
        assert torch.equal(got["power"], aligned[0])


# ---- 4. other bin maps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", ((3, 5, 7), (1, 63, 64)))
def test_radial_with_left_out_coefficients_and_with_one_bin(A, chw):
    afdm, dev = A
    C, H, W = chw
    Wh = W // 2 + 1
    images = _smooth((5,) + chw, 31)
    want = afdm.power_spectrum(images, window=None, remove_mean=False)["power"]
    m = afdm.spectrum.mirror_weights(W)
    g = torch.Generator().manual_seed(32)
    maps = {"random with -1": (torch.randint(-1, 5, (H, Wh), generator=g, dtype=torch.int32), 5),
            "one bin": (torch.zeros(H, Wh, dtype=torch.int32), 1),
            "one bin, half left out": ((torch.arange(H * Wh).view(H, Wh) % 2 - 1).to(torch.int32), 1),
            "nothing kept": (torch.full((H, Wh), -1, dtype=torch.int32), 3),
            "more bins than coefficients": (torch.arange(H * Wh, dtype=torch.int32).view(H, Wh) * 2, 2 * H * Wh + 7)}
    for name, (bins, R) in maps.items():
        ref = torch.zeros(C, R, dtype=torch.float64)
        keep = bins >= 0
        ref.index_add_(1, bins[keep].long(), (want * m)[:, keep])
        power, radial = _abi(afdm, images.to(dev), None, None, None, False, bins.to(dev), R)
        _gates("radial (other maps)", radial, ref, f"{chw} {name}")
        if name == "nothing kept":
            assert bool((radial == 0).all())
        if name == "one bin":
            assert rel_l2(radial[:, 0].cpu(), (power.cpu() * m).sum(dim=(-2, -1))) < REL_L2


# ---- 5. NaN -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,remove_mean", ((None, False), ("hann", True)))
def test_a_nan_pixel_makes_exactly_its_channel_nan(A, window, remove_mean):
    afdm, dev = A
    for chw, at in (((3, 17, 33), (1, 1, 16, 32)), ((3, 32, 32), (2, 1, 0, 0)), ((3, 5, 7), (0, 1, 4, 6))):
        images = _randn((3,) + chw, 41)
        clean = afdm.power_spectrum(images.to(dev), window=window, remove_mean=remove_mean)
        images[at] = float("nan")
        got = afdm.power_spectrum(images.to(dev), window=window, remove_mean=remove_mean)
        for key in ("power", "radial"):
            assert bool(torch.isnan(got[key][1]).all()), (chw, key)
            assert torch.equal(got[key][0], clean[key][0]) and torch.equal(got[key][2], clean[key][2]), (chw, key)
            assert not bool(torch.isnan(clean[key]).any())


# ---- 6. ddpm_run --------------------------------------------------------------------------------------------------------------------
def test_ddpm_run_with_eval_spectrum(A, tmp_path, monkeypatch):
    from PIL import Image
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    runs = {}
    for key in ("plain", "spectrum"):
        wd = tmp_path / key
        wd.mkdir()
        np.savetxt(wd / "mnist.csv", arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "spectrum":
            params["eval_spectrum"] = {"n": 3}
        out = afdm.ddpm_run(params)
        run_dir = os.path.join("runs", "DDPM_Uncondtional_MNIST_3")
        runs[key] = (out, open(os.path.join(run_dir, "settings_MNIST_3.txt")).read().replace(str(wd), ""), str(wd / run_dir))
    (po, pt, pdir), (so, st, sdir) = runs["plain"], runs["spectrum"]
    assert "spectrum" not in po and pt == st and po["loss_all"] == so["loss_all"]
    assert not [f for f in os.listdir(pdir) if f.startswith("spectrum")]
    res = so["spectrum"]
    names = {"power_train", "power_gen", "radial_train", "radial_gen", "counts", "db", "lsd", "hf_ratio"}
    with np.load(os.path.join(sdir, "spectrum_MNIST_3.npz")) as z:
        assert set(z.files) == names == set(res)
        for name in z.files:
            assert z[name].dtype == np.float64 and np.array_equal(z[name], res[name], equal_nan=True)
    assert res["power_gen"].shape == res["power_train"].shape == (1, 32, 17) and res["radial_gen"].shape == res["db"].shape == (1, 17)
    # the saved samples and the training tensors, on the cpu
    monkeypatch.chdir(tmp_path / "spectrum")
    args = afdm.argument(dataset_path="mnist.csv", batch_size=8)
    train = afdm.get_data_MNIST(args)[1].tensors[0]
    saved = torch.stack([torch.from_numpy(np.array(Image.open(os.path.join(so["gen_dir"], f"image_{i}.png")))) for i in range(3)])
    ref, gen = afdm.power_spectrum(train[:3]), afdm.power_spectrum(saved.view(3, 1, 32, 32))
    _gates("power (ddpm_run)", torch.from_numpy(res["power_train"]), ref["power"], "train")
    _gates("power (ddpm_run)", torch.from_numpy(res["power_gen"]), gen["power"], "gen")
    _gates("radial (ddpm_run)", torch.from_numpy(res["radial_train"]), ref["radial"], "train")
    _gates("radial (ddpm_run)", torch.from_numpy(res["radial_gen"]), gen["radial"], "gen")
    db, lsd, hf = afdm.compare_spectra(ref, gen)
    assert np.allclose(res["db"], db.numpy(), rtol=0, atol=1e-9) and res["lsd"] == pytest.approx(lsd, abs=1e-9)
    assert res["hf_ratio"] == pytest.approx(hf, rel=1e-9) and np.array_equal(res["counts"], ref["counts"].numpy())
    with pytest.raises(ValueError, match="eval_spectrum n must be"):
        afdm.ddpm_run(dict(params, eval_spectrum={"n": 5}))      # more than gen_total: fails before any training
    # the same from the checkpoint: the training side has the run's bits, the samples' side is the spectrum of what was drawn
    data = {"args": afdm.argument(image_size=32, image_channels=1, device="cuda", noise_steps=6), "unet_v": 3, "seed": 42,
            "f_settings": {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2},
            "modelpath": so["modelpath"]}
    drawn = []
    sample = afdm.Diffusion.sample

    def spy(self, *a, **k):
        drawn.append(sample(self, *a, **k))
        return drawn[-1]
    monkeypatch.setattr(afdm.Diffusion, "sample", spy)
    r = afdm.spectrum_results(data, train, 3)
    assert set(r) == names and np.array_equal(r["power_train"], res["power_train"]) and np.array_equal(r["radial_train"], res["radial_train"])
    assert len(drawn) == 1 and drawn[0][0].dtype == torch.uint8 and tuple(drawn[0][0].shape) == (3, 1, 32, 32)
    gen = afdm.power_spectrum(drawn[0][0].cpu())
    _gates("power (spectrum_results)", torch.from_numpy(r["power_gen"]), gen["power"], "gen")
    _gates("radial (spectrum_results)", torch.from_numpy(r["radial_gen"]), gen["radial"], "gen")
    with pytest.raises(ValueError, match="spectrum_results: n must be an int in"):
        afdm.spectrum_results(data, train, 17)
