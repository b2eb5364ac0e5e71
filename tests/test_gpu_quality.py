"""PSNR and SSIM of image pairs on the GPU: afd_pair_quality_u8 / afd_pair_quality_f32 through image_quality / pair_sums, against
the pure-torch fp64 path on the cpu (pinned to a brute force over windows by tests/test_quality_host.py), and ddpm_run with
params["eval_restoration"] and restoration_results on its checkpoint.

Gates.  The pixel sums and every count are bit-equal for uint8 (exact integers); for float32 the sums of squared and of absolute
differences are fp64 sums of at most 4096 non-negative terms in another order: 1e-13 relative.  SSIM, derived rather than
measured: a weighted moment is a sum of K^2 products of magnitude at most L^2 under weights that add up to 1, so an implementation
is off by at most gamma = (K^2 + 2) 2^-53 L^2 (1.4e-14 L^2 at K = 11); both factors of the numerator are bounded by the matching
factors of the denominator, which are at least c1 = 1e-4 L^2 and c2 = 9e-4 L^2; an SSIM value therefore moves by at most about
2 (4 gamma / c1 + 4 gamma / c2) = 1.2e-9 per implementation, and the gate is 5e-9 absolute, for every element of the map and for
every plane's mean.  The near-flat planes (a constant plus 1e-4 of noise) cancel in the variances and stay under the same bound."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import note

pytestmark = pytest.mark.gpu
SSIM_GATE = 5e-9
SUM_GATE = 1e-13
CASES = (((3, 3, 32, 32), 11), ((2, 1, 64, 64), 11), ((2, 2, 11, 17), 11), ((1, 1, 15, 15), 15), ((5, 3, 13, 64), 3), ((2, 2, 9, 12), 1),
         ((1, 1, 64, 64), 15))
DTYPES = (torch.uint8, torch.float32)
_ids = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"K{v}" if isinstance(v, int) else str(v).split(".")[-1])


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


@functools.lru_cache(maxsize=None)
def _case(shape, K, dtype, flat=False):
    """(a, b, region, the cpu path's sums and map without and with the region): made once, never written."""
    g = torch.Generator().manual_seed(1000 * shape[2] + 10 * shape[3] + K)
    if dtype == torch.uint8:
        a, b = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) for _ in range(2))
    elif flat:
        a, b = (0.37 + 1e-4 * (torch.rand(shape, generator=g) * 2 - 1) for _ in range(2))
    else:
        a, b = (torch.rand(shape, generator=g) * 2 - 1 for _ in range(2))
    region = (torch.rand((shape[0], 1) + shape[2:], generator=g) < 0.4).to(torch.uint8)
    import afdm
    L = 255.0 if dtype == torch.uint8 else 2.0
    win = afdm.gaussian_window(K, 1.5)
    c = ((0.01 * L) ** 2, (0.03 * L) ** 2)
    return a, b, region, win, c, afdm.pair_sums(a, b, win, *c, None, True), afdm.pair_sums(a, b, win, *c, region, True)


def _compare(what, got, want, u8):
    (out, ssim_map), (ref, ref_map) = got, want
    out, ssim_map = out.cpu(), ssim_map.cpu()
    assert out.shape == ref.shape and ssim_map.shape == ref_map.shape and out.dtype == ssim_map.dtype == torch.float64
    assert torch.equal(out[..., 2], ref[..., 2]) and torch.equal(out[..., 4], ref[..., 4]), what
    if u8:
        assert torch.equal(out[..., :2], ref[..., :2]), what
        e_sum = 0.0
    else:
        e_sum = float(((out[..., :2] - ref[..., :2]).abs() / ref[..., :2].clamp_min(1e-300)).max())
    e_map = float((ssim_map - ref_map).abs().max())
    e_mean = float(((out[..., 3] - ref[..., 3]).abs() / ref[..., 4].clamp_min(1)).max())
    print(f"{what}: pixel sums {e_sum:.3e} relative, ssim map {e_map:.3e}, plane means {e_mean:.3e}")
    note("image quality: ssim against the cpu path (absolute)", max(e_map, e_mean), what)
    assert e_sum <= SUM_GATE and e_map <= SSIM_GATE and e_mean <= SSIM_GATE, what


# ---- 1. the device against the cpu path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,K", CASES, **_ids)
def test_the_device_against_the_cpu_path(A, shape, K, dtype):
    afdm, dev = A
    a, b, region, win, c, plain, masked = _case(shape, K, dtype)
    u8 = dtype == torch.uint8
    _compare(f"{shape} K={K} {dtype}", afdm.pair_sums(a.to(dev), b.to(dev), win, *c, None, True), plain, u8)
    _compare(f"{shape} K={K} {dtype} region", afdm.pair_sums(a.to(dev), b.to(dev), win, *c, region.to(dev), True), masked, u8)
    first = region[:1]                                       # one mask for all images
    want = afdm.pair_sums(a, b, win, *c, first, True)
    _compare(f"{shape} K={K} {dtype} shared region", afdm.pair_sums(a.to(dev), b.to(dev), win, *c, first.to(dev), True), want, u8)
    # without the map the sums have the same bits
    out, none = afdm.pair_sums(a.to(dev), b.to(dev), win, *c, region.to(dev))
    assert none is None and torch.equal(out, afdm.pair_sums(a.to(dev), b.to(dev), win, *c, region.to(dev), True)[0])


@pytest.mark.parametrize("shape,K", (((2, 1, 32, 32), 11), ((1, 2, 20, 33), 7)), **_ids)
def test_near_flat_planes_stay_under_the_bound(A, shape, K):
    afdm, dev = A
    a, b, region, win, c, plain, masked = _case(shape, K, torch.float32, True)
    _compare(f"near-flat {shape} K={K}", afdm.pair_sums(a.to(dev), b.to(dev), win, *c, None, True), plain, False)
    _compare(f"near-flat {shape} K={K} region", afdm.pair_sums(a.to(dev), b.to(dev), win, *c, region.to(dev), True), masked, False)


def test_the_dict_on_the_device(A):
    afdm, dev = A
    a, b, region, _, _, _, _ = _case((3, 3, 32, 32), 11, torch.uint8)
    for reg in (None, region):
        got = afdm.image_quality(a.to(dev), b.to(dev), region=None if reg is None else reg.to(dev), return_map=True)
        want = afdm.image_quality(a, b, region=reg, return_map=True)
        assert set(got) == set(want)
        for key in ("mse", "mae", "pixels", "windows"):
            assert got[key].device.type == "cuda" and torch.equal(got[key].cpu(), want[key]), key
        assert torch.allclose(got["psnr"].cpu(), want["psnr"], rtol=1e-14, atol=0)
        for key in ("ssim", "ssim_channels", "ssim_map"):
            assert float((got[key].cpu() - want[key]).abs().max()) <= SSIM_GATE, key
    assert torch.equal(afdm.psnr(a.to(dev), b.to(dev)), afdm.image_quality(a.to(dev), b.to(dev))["psnr"])
    assert torch.equal(afdm.ssim(a.to(dev), b.to(dev), window=7), afdm.image_quality(a.to(dev), b.to(dev), window=7)["ssim"])
    # a cpu region beside device images, and device images that are views
    got = afdm.image_quality(a.to(dev)[:, :2], b.to(dev)[:, :2], region=region)
    assert torch.equal(got["mse"].cpu(), afdm.image_quality(a[:, :2], b[:, :2], region=region)["mse"])


# ---- 2. exact identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,K", CASES, **_ids)
def test_both_dtypes_give_the_same_bits_on_the_same_integers(A, shape, K):
    afdm, dev = A
    a, b, region, _, _, _, _ = _case(shape, K, torch.uint8)
    for reg in (None, region.to(dev)):
        u = afdm.image_quality(a.to(dev), b.to(dev), window=K, region=reg, return_map=True)
        f = afdm.image_quality(a.to(dev).float(), b.to(dev).float(), data_range=255, window=K, region=reg, return_map=True)
        for key in u:
            assert torch.equal(u[key].view(torch.int64), f[key].view(torch.int64)), key


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
@pytest.mark.parametrize("shape,K", CASES, **_ids)
def test_an_image_against_itself_is_exactly_one(A, shape, K, dtype):
    afdm, dev = A
    a = _case(shape, K, dtype)[0].to(dev)
    r = afdm.image_quality(a, a.clone(), window=K, return_map=True)
    assert bool((r["ssim_map"] == 1.0).all()) and bool((r["ssim"] == 1.0).all()) and bool((r["ssim_channels"] == 1.0).all())
    assert bool((r["mse"] == 0).all()) and bool(torch.isposinf(r["psnr"]).all())


@pytest.mark.parametrize("dtype", DTYPES, **_ids)
def test_two_calls_and_a_replayed_graph_give_equal_bits(A, dtype):
    afdm, dev = A
    for shape, K in (((3, 3, 32, 32), 11), ((5, 3, 13, 64), 3)):
        a, b, region, win, c, _, _ = _case(shape, K, dtype)
        a, b, region = a.to(dev), b.to(dev), region.to(dev).view(shape[0], *shape[2:]).contiguous()
        first = afdm.ops.pair_quality(a, b, win, *c, region, True)
        again = afdm.ops.pair_quality(a, b, win, *c, region, True)
        assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(first, again))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            afdm.ops.pair_quality(a, b, win, *c, region, True)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            held = afdm.ops.pair_quality(a, b, win, *c, region, True)
        for t in held:
            t.fill_(-7777.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x.view(torch.int64), y.view(torch.int64)) for x, y in zip(first, held))


# ---- 3. the region and NaN ----------------------------------------------------------------------------------------------------------
def test_the_centre_hole_at_32(A):
    afdm, dev = A
    from afdm.tasks import _restoration_mask
    a, b, _, _, _, _, _ = _case((3, 3, 32, 32), 11, torch.uint8)
    hole = torch.from_numpy(1 - _restoration_mask("center", 32))
    got, want = afdm.image_quality(a.to(dev), b.to(dev), region=hole), afdm.image_quality(a, b, region=hole)
    assert got["pixels"].tolist() == [768.0] * 3 and got["windows"].tolist() == [768.0] * 3
    assert torch.equal(got["mse"].cpu(), want["mse"]) and torch.equal(got["mae"].cpu(), want["mae"])
    assert float((got["ssim_channels"].cpu() - want["ssim_channels"]).abs().max()) <= SSIM_GATE
    empty = afdm.image_quality(a.to(dev), b.to(dev), region=torch.zeros(32, 32))
    assert empty["pixels"].tolist() == [0.0] * 3 and bool(torch.isnan(empty["psnr"]).all()) and bool(torch.isnan(empty["ssim"]).all())


def test_a_nan_reaches_its_own_plane_only(A):
    afdm, dev = A
    a, b, _, win, c, _, _ = _case((3, 3, 32, 32), 11, torch.float32)
    a, b = a.to(dev), b.to(dev)
    clean, clean_map = afdm.pair_sums(a, b, win, *c, None, True)
    bad = a.clone()
    bad[1, 2, 9, 30] = float("nan")
    out, ssim_map = afdm.pair_sums(bad, b, win, *c, None, True)
    hit = torch.zeros(3, 3, dtype=torch.bool, device=dev)
    hit[1, 2] = True
    assert torch.equal(out[~hit], clean[~hit]) and torch.equal(ssim_map[~hit], clean_map[~hit])
    assert bool(torch.isnan(out[1, 2, [0, 1, 3]]).all()) and out[1, 2, 2] == 1024 and out[1, 2, 4] == 484
    nan_windows = torch.isnan(ssim_map[1, 2])
    assert int(nan_windows.sum()) == 10 * 2 and bool(nan_windows[:10, 20:].all())      # windows of rows 0..9 and columns 20..21 hold pixel (9, 30)
    away = torch.zeros(32, 32)
    away[20:, :16] = 1
    r = afdm.image_quality(bad, b, region=away)
    assert bool(torch.isfinite(r["psnr"]).all()) and bool(torch.isfinite(r["ssim"]).all())


# ---- 4. ddpm_run --------------------------------------------------------------------------------------------------------------------
def test_ddpm_run_with_eval_restoration(A, tmp_path, monkeypatch):
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    cfg = {"n": 4, "steps": 3, "factor": 4}
    runs = {}
    for key in ("plain", "restoration"):
        wd = tmp_path / key
        wd.mkdir()
        np.savetxt(wd / "mnist.csv", arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "restoration":
            params["eval_restoration"] = cfg
        out = afdm.ddpm_run(params)
        run_dir = os.path.join("runs", "DDPM_Uncondtional_MNIST_3")
        files = {}
        for root, _, names in os.walk(wd):
            for f in names:
                path = os.path.join(root, f)
                files[os.path.relpath(path, wd)] = open(path, "rb").read().replace(str(wd).encode(), b"")
        runs[key] = (out, files, str(wd / run_dir))
    (po, pf, _), (so, sf, sdir) = runs["plain"], runs["restoration"]
    # exactly one more file, and everything else as it was
    written = os.path.join("runs", "DDPM_Uncondtional_MNIST_3", "restoration_MNIST_3.json")
    assert set(sf) - set(pf) == {written} and not set(pf) - set(sf)
    same = [f for f in pf if not f.endswith(".pt")]
    assert all(pf[f] == sf[f] for f in same), [f for f in same if pf[f] != sf[f]]
    assert "restoration" not in po and set(so) - set(po) == {"restoration"} and po["loss_all"] == so["loss_all"]
    assert torch.equal(po["sample"], so["sample"])
    res = so["restoration"]
    assert json.load(open(os.path.join(sdir, "restoration_MNIST_3.json"))) == json.loads(json.dumps(res))
    assert set(res) == {"n", "window", "sigma", "inpaint", "superres"} and res["n"] == 4 and res["window"] == 11 and res["sigma"] == 1.5
    assert set(res["inpaint"]) == {"mask", "hole_pixels", "psnr", "ssim", "psnr_hole", "ssim_hole"} and res["inpaint"]["hole_pixels"] == 256
    assert set(res["superres"]) == {"factor", "psnr", "ssim", "psnr_reference", "ssim_reference", "consistency_psnr"}
    for task in ("inpaint", "superres"):
        for key, val in res[task].items():
            if isinstance(val, dict):
                assert set(val) == {"mean", "std", "values"} and len(val["values"]) == 4, (task, key)
                assert val["mean"] == pytest.approx(np.mean(val["values"]), rel=1e-12) and val["std"] == pytest.approx(np.std(val["values"]), abs=1e-9)
    assert all(math.isfinite(x) for x in res["superres"]["consistency_psnr"]["values"])
    assert all(-1.0 <= x <= 1.0 for key in ("ssim", "ssim_hole") for x in res["inpaint"][key]["values"])
    # the scores are those of what the samplers returned: the same tasks from the checkpoint, the samplers' outputs kept
    monkeypatch.chdir(tmp_path / "restoration")
    train = afdm.get_data_MNIST(afdm.argument(dataset_path="mnist.csv", batch_size=8))[1].tensors[0]
    store = afdm.DeviceDataset(train, device="cuda")
    data = {"args": afdm.argument(image_size=32, image_channels=1, device="cuda", noise_steps=6), "unet_v": 3, "seed": 42,
            "f_settings": {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2},
            "modelpath": so["modelpath"]}
    kept = {}
    inpaint, ilvr = afdm.Diffusion.inpaint, afdm.Diffusion.ilvr

    def spy_inpaint(self, model, images, mask, **k):
        kept["inpaint"] = (images, torch.as_tensor(mask), inpaint(self, model, images, mask, **k))
        return kept["inpaint"][2]

    def spy_ilvr(self, model, reference, **k):
        kept["ilvr"] = (reference, ilvr(self, model, reference, **k))
        return kept["ilvr"][1]
    monkeypatch.setattr(afdm.Diffusion, "inpaint", spy_inpaint)
    monkeypatch.setattr(afdm.Diffusion, "ilvr", spy_ilvr)
    r = afdm.restoration_results(data, store, 4, steps=3)
    for task in ("inpaint", "superres"):
        for key, val in res[task].items():
            if isinstance(val, dict):
                assert r[task][key]["values"] == pytest.approx(val["values"], rel=1e-9, abs=1e-9), (task, key)
            else:
                assert r[task][key] == val, (task, key)
    pixels = store.pixels(4)
    images, mask, (filled, _) = kept["inpaint"]
    assert tuple(mask.shape) == (32, 32) and int(mask.sum()) == 1024 - 256 and filled.dtype == torch.uint8
    whole, hole = afdm.image_quality(filled.cpu(), pixels.cpu()), afdm.image_quality(filled.cpu(), pixels.cpu(), region=1 - mask)
    assert r["inpaint"]["psnr"]["values"] == pytest.approx(whole["psnr"].tolist(), rel=1e-12)
    assert r["inpaint"]["psnr_hole"]["values"] == pytest.approx(hole["psnr"].tolist(), rel=1e-12)
    assert r["inpaint"]["ssim"]["values"] == pytest.approx(whole["ssim"].tolist(), abs=SSIM_GATE)
    assert r["inpaint"]["ssim_hole"]["values"] == pytest.approx(hole["ssim"].tolist(), abs=SSIM_GATE)
    known = mask.bool().expand(4, 1, 32, 32)
    for i in range(4):                                       # with the known pixels reproduced, the hole alone cannot score better
        if torch.equal(filled[i].cpu()[known[i]], pixels[i].cpu()[known[i]]):
            assert r["inpaint"]["psnr_hole"]["values"][i] <= r["inpaint"]["psnr"]["values"][i]
    reference, (sample, _, sample_float) = kept["ilvr"]
    got = afdm.image_quality(sample.cpu(), pixels.cpu())
    base = afdm.image_quality(afdm.ops.quantize_u8(reference).cpu(), pixels.cpu())
    assert r["superres"]["psnr"]["values"] == pytest.approx(got["psnr"].tolist(), rel=1e-12)
    assert r["superres"]["ssim_reference"]["values"] == pytest.approx(base["ssim"].tolist(), abs=SSIM_GATE)
    assert r["superres"]["psnr_reference"]["values"] == pytest.approx(base["psnr"].tolist(), rel=1e-12)
    with pytest.raises(ValueError, match="restoration_results: n must be an int in"):
        afdm.restoration_results(data, store, 17)
    with pytest.raises(ValueError, match="eval_restoration n must lie in"):
        afdm.ddpm_run(dict(params, eval_restoration={"n": 17}))
