"""GPU tests of the equivariance scores: the row-wise resampler bit for bit against the single-transform kernel and torch.roll,
the device path of shift_2d_matrix against a scipy fixture, the fused comparison kernel against the fp64 restatement (and run
twice for identical bits), a pointwise model (exactly equivariant up to one fp32 rounding), a model with a planted defect
(closed form), the real UNet against a hand-composed pipeline, the conditional UNet, the model state after an exception, and
ddpm_run's eval_equivariance."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, note
from test_equiv_host import spline3_affine64, spline3_prefilter64

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
# UNet test: worst relative difference of mse / power between Diffusion.equivariance and the hand-composed pipeline, measured
# on the first run of this test on an MI355X (variants 3 and 0); the gate is ten times that, floored at 1e-9
UNET_MEASURED = 4.2e-7
UNET_GATE = max(10 * UNET_MEASURED, 1e-9)


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    iv = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(iv), b.view(iv))


def _single(ops, x, spec, a):
    """One transform of a whole batch through the single-transform kernel (afd_affine_spline3_wrap)."""
    if spec[0] == "rotate":
        return ops.rotate_spline3_wrap(x, spec[1])
    return ops.affine_spline3_wrap(x, a[:4].reshape(2, 2), a[4:])


class _Fn(torch.nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x, t):
        return self.fn(x, t)


class _FixedNoise:
    """noise_fn that hands out consecutive rows of one fixed tensor: the same eps per (image, t) whatever the chunking."""

    def __init__(self, eps):
        self.eps, self.at = eps, 0

    def __call__(self, shape):
        z = self.eps[self.at:self.at + shape[0]]
        self.at += shape[0]
        assert tuple(z.shape) == tuple(shape)
        return z


def _restated(diff, f, g_rows, src, k, aff, margin):
    """mse, power, count per row in numpy fp64 from the definitions: f (n_src, C, H, W) base outputs, g_rows (rows, C, H, W)."""
    coef = spline3_prefilter64(f)
    H, W = f.shape[-2:]
    mse, power, count = [], [], []
    for r in range(len(k)):
        ref = spline3_affine64(coef[src[r]], aff[k[r]])
        m = diff.equivariance_mask(aff[k[r]], H, W, margin)
        d = g_rows[r].astype(np.float64) - ref
        cnt = int(m.sum())
        count.append(cnt)
        mse.append(float((d * d)[:, m].sum()) / (f.shape[1] * cnt))
        power.append(float((ref * ref)[:, m].sum()) / (f.shape[1] * cnt))
    return np.array(mse), np.array(power), np.array(count)


SPECS = [("rotate", 10), ("translate", 0.5, 0.25), ("rotate", 45), ("translate", -1.75, 3.0), ("rotate", 90), ("translate", 8, 8),
         ("rotate", -33.3), ("translate", 0, 0)]


# ---- 1. the row-wise resampler -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("size", [32, 64])
def test_rows_are_the_single_transform_kernel_bit_for_bit(A, C, size):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=10, img_size=size, device=dev)
    g = torch.Generator().manual_seed(size + C)
    n_src, rows = 5, 23
    x = torch.randn(n_src, C, size, size, generator=g).to(dev)
    aff = diff.equivariance_transforms(SPECS)
    img = torch.randint(0, n_src, (rows,), generator=g)
    k = torch.randint(0, len(SPECS), (rows,), generator=g)
    k[:len(SPECS)] = torch.randperm(len(SPECS), generator=g)            # every transform at least once
    coef = ops.spline3_prefilter_wrap(x)
    assert coef.dtype == torch.float64 and coef.shape == x.shape
    got = ops.affine_spline3_wrap_rows(coef, img.to(dev), aff.to(dev), k.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (rows, C, size, size)
    whole = [_single(ops, x, sp, aff[i].numpy()) for i, sp in enumerate(SPECS)]
    for r in range(rows):
        assert _same_bits(got[r], whole[int(k[r])][int(img[r])]), (r, SPECS[int(k[r])])
    with pytest.raises(afdm.AfdError, match="img must lie"):
        ops.affine_spline3_wrap_rows(coef, img.to(dev) + n_src, aff.to(dev), k.to(dev))
    with pytest.raises(afdm.AfdError, match="k must lie"):
        ops.affine_spline3_wrap_rows(coef, img.to(dev), aff.to(dev), k.to(dev) - 1)


def test_whole_pixel_translate_rows_are_a_roll(A):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=10, img_size=32, device=dev)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 3, 32, 32, generator=g).to(dev)
    shifts = [(0, 0), (1, 0), (0, -1), (8, 8), (-5, 13), (31, -32), (40, 3)]
    aff = diff.equivariance_transforms([("translate", dy, dx) for dy, dx in shifts]).to(dev)
    img = torch.arange(3).repeat_interleave(len(shifts)).to(dev)
    k = torch.arange(len(shifts)).repeat(3).to(dev)
    got = ops.affine_spline3_wrap_rows(ops.spline3_prefilter_wrap(x), img, aff, k)
    for r in range(len(k)):
        dy, dx = shifts[int(k[r])]
        assert torch.equal(got[r], torch.roll(x[int(img[r])], shifts=(dy, dx), dims=(1, 2))), (r, dy, dx)


def test_fractional_shift_on_the_device_against_the_scipy_fixture(A):
    afdm, dev = A
    gold = load_golden("shift.npz")
    x = torch.from_numpy(gold["x"]).to(dev)
    for (v, h), want in zip(gold["shifts"], gold["out"]):
        got = afdm.Diffusion.shift_2d_matrix(x, float(h), float(v), dev)
        assert got.is_cuda and got.dtype == torch.float32
        diff_ulp = (got.cpu().view(torch.int32) - torch.from_numpy(want).view(torch.int32)).abs().max().item()
        print(f"fractional shift ({v}, {h}) vs scipy: worst difference {diff_ulp} ulp")
        assert _same_bits(got.cpu(), torch.from_numpy(want)), (v, h, diff_ulp)
    # whole-pixel shifts stay a roll
    assert torch.equal(afdm.Diffusion.shift_2d_matrix(x, 3, -2, dev), torch.roll(x, shifts=(-2, 3), dims=(2, 3)))


# ---- 2. the comparison kernel against fp64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", [4.0, 0.0, 2.5])
def test_terms_kernel_against_fp64(A, margin):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=10, img_size=32, device=dev)
    g = torch.Generator().manual_seed(11)
    n_src, C, rows = 4, 3, 29
    f = torch.randn(n_src, C, 32, 32, generator=g)
    gr = torch.randn(rows, C, 32, 32, generator=g)                      # independent of f: d of order 1
    aff = diff.equivariance_transforms(SPECS)
    img = torch.randint(0, n_src, (rows,), generator=g)
    k = torch.randint(0, len(SPECS), (rows,), generator=g)
    k[:len(SPECS)] = torch.arange(len(SPECS))
    coef = ops.spline3_prefilter_wrap(f.to(dev))
    args = (coef, img.to(dev), aff.to(dev), k.to(dev), gr.to(dev), margin)
    out = ops.eq_terms(*args)
    out2 = ops.eq_terms(*args)
    assert out.dtype == torch.float64 and tuple(out.shape) == (rows, 3)
    assert _same_bits(out, out2)                                        # deterministic
    mse, power, count = _restated(diff, f.numpy(), gr.numpy(), img.numpy(), k.numpy(), aff.numpy(), margin)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 2], count * C), (got[:, 2], count * C)     # exact, the 90 degree rotation included
    rel_d = np.abs(got[:, 0] / got[:, 2] - mse) / mse
    rel_r = np.abs(got[:, 1] / got[:, 2] - power) / power
    worst = float(max(rel_d.max(), rel_r.max()))
    note("equivariance: terms kernel vs fp64 (relative, per row)", worst, margin)
    print(f"terms vs fp64 (margin {margin}): sum d^2 worst {rel_d.max():.2e}, sum ref^2 worst {rel_r.max():.2e}; counts {sorted(set(count))}")
    assert worst < 1e-10
    if margin == 4.0:
        by_k = {int(kk): int(c) for kk, c in zip(k.numpy(), count)}
        assert [by_k[i] for i in (0, 2, 4, 5, 7)] == [512, 464, 558, 256, 576]     # rotations whose mask cuts the corners


# ---- 3. a pointwise model --------------------------------------------------------------------------------------------------------
def test_pointwise_model_is_equivariant_up_to_one_rounding(A):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=100, img_size=32, device=dev)
    g = torch.Generator().manual_seed(3)
    n, ts = 5, [7, 60]
    x0 = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    eps = torch.randn(n * len(ts), 3, 32, 32, generator=g).to(dev)
    model = _Fn(lambda x, t: 0.5 * x)
    specs = [("translate", 3, -2), ("translate", 0.5, 0.5), ("rotate", 10), ("rotate", 45)]
    r = diff.equivariance(model, x0, ts, specs, batch=256, noise_fn=_FixedNoise(eps))
    # g = 0.5 fl32(S x) and r = 0.5 (S x) exactly (a power of two passes through the linear prefilter and the interpolation
    # unchanged), so |d| <= 2^-25 |S x| per element and mse <= (2^-24 max |S x|)^2 with a factor of 4 to spare
    img0 = torch.arange(n).repeat_interleave(len(ts)).to(dev)
    t0 = torch.tensor(ts).repeat(n).to(dev)
    xt = ops.noise_images_gather(x0.to(dev), img0, eps, t0, diff.alpha_hat)
    aff = diff.equivariance_transforms(specs).numpy()
    sx_max = max(float(_single(ops, xt, sp, aff[i]).abs().max()) for i, sp in enumerate(specs))
    bound = (2.0 ** -24 * sx_max) ** 2
    worst = float(r["mse"].max())
    note("equivariance: pointwise model, mse / its rounding bound", worst / bound)
    print(f"pointwise model: worst mse {worst:.3e} <= bound {bound:.3e} (max |S x| {sx_max:.3f}); eq_db {r['eq_db'].tolist()}")
    assert worst <= bound
    assert float(r["eq_db"].min()) >= 10 * math.log10(4.0 / bound)        # about 135 dB at this scale; the bound, not a measurement
    assert r["count"].tolist() == [float(diff.equivariance_mask(a, 32, 32, 4.0).sum()) for a in diff.equivariance_transforms(specs)]
    r7 = diff.equivariance(model, x0, ts, specs, batch=7, noise_fn=_FixedNoise(eps))
    for key in r:
        assert _same_bits(r[key], r7[key]), key
    assert tuple(r["mse"].shape) == (n, 2, 4) and tuple(r["eq_db"].shape) == (2, 4) and tuple(r["count"].shape) == (4,)
    assert all(v.dtype == torch.float64 and v.device.type == "cpu" for v in r.values())


# ---- 4. a planted defect -----------------------------------------------------------------------------------------------------------
def test_planted_defect_matches_the_closed_form(A):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=100, img_size=32, device=dev)
    g = torch.Generator().manual_seed(4)
    n, ts = 4, [20]
    x0 = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    Pn = torch.randn(1, 3, 32, 32, generator=g)                         # a fixed pattern tied to absolute pixel coordinates
    Pd = Pn.to(dev)
    model = _Fn(lambda x, t: x + Pd)
    specs = [("translate", 0, 0), ("translate", 5, -3), ("translate", 0.5, 0.5), ("rotate", 10), ("rotate", 45)]
    r = diff.equivariance(model, x0, ts, specs, batch=6)
    aff = diff.equivariance_transforms(specs).numpy()
    coef = spline3_prefilter64(Pn.numpy()[0])
    worst = 0.0
    for kk, a in enumerate(aff[1:], start=1):
        m = diff.equivariance_mask(a, 32, 32, 4.0)
        d = Pn.numpy()[0].astype(np.float64) - spline3_affine64(coef, a)        # d = P - S P (+ fp32 rounding, 2^-24 of order 1)
        want = float((d * d)[:, m].sum()) / (3 * int(m.sum()))
        rel = float((np.abs(r["mse"][:, 0, kk].numpy() - want) / want).max())
        worst = max(worst, rel)
        print(f"planted defect, {specs[kk]}: mse {r['mse'][:, 0, kk].tolist()} vs closed form {want:.9f} (rel {rel:.2e})")
    note("equivariance: planted defect, mse vs closed form (relative)", worst)
    assert worst < 1e-6
    ident = float(r["mse"][:, 0, 0].max())                             # identity: d is pure fp32 rounding of x + P
    print(f"planted defect, identity: worst mse {ident:.3e}")
    assert ident <= (2.0 ** -23 * 8.0) ** 2 and float(r["eq_db"][0, 0]) > 110


# ---- 5. the real UNet against a hand-composed pipeline -------------------------------------------------------------------------
def _unet(afdm, dev, variant, num_classes=None, seed=42):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET) if variant else None, device=dev, variant=variant,
                     **kw).to(dev)


UNET_SPECS = [("translate", 3, -2), ("translate", 0.5, 0.5), ("rotate", 10), ("rotate", 45)]


@pytest.mark.parametrize("variant", [3, 0])
def test_unet_scores_equal_a_hand_composed_pipeline(A, variant):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    model = _unet(afdm, dev, variant)
    g = torch.Generator().manual_seed(6)
    n, ts = 3, [50, 600]
    J, K = len(ts), len(UNET_SPECS)
    x0 = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    eps = torch.randn(n * J, 3, 32, 32, generator=g).to(dev)
    r = diff.equivariance(model, x0, ts, UNET_SPECS, batch=8, noise_fn=_FixedNoise(eps))
    assert model.training and model._t_range is None
    aff = diff.equivariance_transforms(UNET_SPECS).numpy()
    img0 = torch.arange(n).repeat_interleave(J).to(dev)
    t0 = torch.tensor(ts).repeat(n).to(dev)
    model.eval()
    with torch.no_grad():
        xt = ops.noise_images_gather(x0.to(dev), img0, eps, t0, diff.alpha_hat)
        f = model(xt, t0).cpu().numpy()
        gk = [model(_single(ops, xt, sp, aff[i]), t0).cpu().numpy() for i, sp in enumerate(UNET_SPECS)]
    model.train()
    img, j, k = diff.equivariance_rows(n, J, K)
    src = img * J + j
    g_rows = np.stack([gk[k[q]][src[q]] for q in range(len(k))])
    mse, power, count = _restated(diff, f, g_rows, src, k, aff, 4.0)
    rel = max(float((np.abs(r["mse"].numpy().ravel() - mse) / mse).max()), float((np.abs(r["power"].numpy().ravel() - power) / power).max()))
    note(f"equivariance: UNet vs hand-composed pipeline (relative; measured {UNET_MEASURED:.1e}, gate {UNET_GATE:.1e})", rel, variant)
    print(f"UNet variant {variant}: worst relative difference {rel:.3e}; eq_db {r['eq_db'].tolist()}; snr_db {r['snr_db'].tolist()}")
    assert rel < UNET_GATE
    m, pw = mse.reshape(n, J, K).mean(0), power.reshape(n, J, K).mean(0)
    assert np.allclose(r["eq_db"].numpy(), 10 * np.log10(4.0 / m), rtol=0, atol=1e-6)
    assert np.allclose(r["snr_db"].numpy(), 10 * np.log10(pw / m), rtol=0, atol=1e-6)
    assert r["count"].tolist() == [float(c) for c in count[:K]]
    assert torch.isfinite(r["eq_db"]).all() and torch.isfinite(r["snr_db"]).all()


# ---- 6. the conditional UNet ---------------------------------------------------------------------------------------------------
def test_conditional_rows_equal_a_hand_loop(A):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    model = _unet(afdm, dev, 3, num_classes=10)
    g = torch.Generator().manual_seed(8)
    n, ts, batch = 3, [40, 700], 5
    J, K = len(ts), len(UNET_SPECS)
    x0 = torch.rand(n, 3, 32, 32, generator=g) * 2 - 1
    labels = torch.tensor([3, afdm.NULL_LABEL, 7])
    afdm.set_seed(9)
    r = diff.equivariance(model, x0, ts, UNET_SPECS, labels=labels, batch=batch)
    afdm.set_seed(9)
    aff = diff.equivariance_transforms(UNET_SPECS).to(dev)
    img, j, k = diff.equivariance_rows(n, J, K)
    src_d, k_d = torch.from_numpy(img * J + j).to(dev), torch.from_numpy(k).to(dev)
    t_d = torch.tensor(ts)[torch.from_numpy(j)].to(dev)
    y = labels.to(dev)
    img0 = torch.arange(n).repeat_interleave(J).to(dev)
    t0 = torch.tensor(ts).repeat(n).to(dev)
    cx, cf, sums = [], [], []
    model.eval()
    with torch.no_grad():
        for lo, hi in diff.bpd_chunks(n * J, batch):
            eps = torch.randn((hi - lo, 3, 32, 32), device=dev)
            xt = ops.noise_images_gather(x0.to(dev), img0[lo:hi], eps, t0[lo:hi], diff.alpha_hat)
            cx.append(ops.spline3_prefilter_wrap(xt))
            cf.append(ops.spline3_prefilter_wrap(model(xt, t0[lo:hi], y[img0[lo:hi]]).contiguous()))
        cx, cf = torch.cat(cx), torch.cat(cf)
        for lo, hi in diff.bpd_chunks(len(k), batch):
            sx = ops.affine_spline3_wrap_rows(cx, src_d[lo:hi], aff, k_d[lo:hi])
            gg = model(sx, t_d[lo:hi], y[src_d[lo:hi] // J]).contiguous()
            sums.append(ops.eq_terms(cf, src_d[lo:hi], aff, k_d[lo:hi], gg, 4.0))
    model.train()
    want = diff.equivariance_combine(n, J, K, 3, torch.cat(sums).cpu().numpy(), 2.0)
    for key in want:
        assert _same_bits(r[key], want[key]), key
    afdm.set_seed(9)
    other = diff.equivariance(model, x0, ts, UNET_SPECS, labels=torch.tensor([5, afdm.NULL_LABEL, 1]), batch=batch)
    assert _same_bits(other["mse"][1], r["mse"][1]) and not torch.equal(other["mse"][0], r["mse"][0])      # per-row labels
    assert model.training and model._t_range is None


# ---- 7. model state after an exception ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
def test_model_state_is_restored_after_an_exception(A, training):
    afdm, dev = A

    class Boom(afdm.UNet):
        calls = 0

        def forward(self, *a, **kw):
            Boom.calls += 1
            if Boom.calls == 2:
                raise RuntimeError("boom in the second forward")
            return super().forward(*a, **kw)

    afdm.set_seed(42)
    model = Boom(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    model.train(training)
    diff = afdm.Diffusion(noise_steps=21, img_size=32, device=dev)
    x0 = torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)) * 2 - 1
    with pytest.raises(RuntimeError, match="second forward"):
        diff.equivariance(model, x0, [3, 9], [("rotate", 10)], batch=8)
    assert Boom.calls == 2 and model.training == training and model._t_range is None


# ---- 8. ddpm_run ---------------------------------------------------------------------------------------------------------------
def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = p
    return out


def test_ddpm_run_eval_equivariance(A, tmp_path, monkeypatch):
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    runs = {}
    for key in ("plain", "eq"):
        wd = tmp_path / key
        wd.mkdir()
        csvp = wd / "mnist.csv"
        np.savetxt(csvp, arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "eq":
            params["eval_equivariance"] = {"N": 4, "t": [2, 9], "transforms": [("translate", 1, 0), ("translate", 0.5, 0.5),
                                                                              ("rotate", 15)]}
        runs[key] = (afdm.ddpm_run(params), _files(wd))
    out, files = runs["eq"]
    plain_out, plain_files = runs["plain"]
    eq_file = os.path.join("runs", "DDPM_Uncondtional_MNIST_3", "equivariance_MNIST_3.json")
    assert set(files) - set(plain_files) == {eq_file} and set(plain_files) <= set(files)
    assert "equivariance" not in plain_out and set(out) - set(plain_out) == {"equivariance"}
    tab = out["equivariance"]
    assert np.asarray(tab["eq_db"]).shape == (2, 3) and np.isfinite(tab["eq_db"]).all() and np.isfinite(tab["snr_db"]).all()
    saved = json.load(open(files[eq_file]))
    assert saved == json.loads(json.dumps(tab))
    assert saved["N"] == 4 and saved["t"] == [2, 9] and saved["margin"] == 4.0 and saved["peak"] == 2.0
    assert saved["transforms"] == [["translate", 1, 0], ["translate", 0.5, 0.5], ["rotate", 15]] and len(saved["count"]) == 3
