"""FID / KID on the GPU: afd_feature_moments_f32 and afd_poly_mmd_sums_f32 through the C ABI and through ops, FeatureStats,
kernel_distance, fidelity and DeviceDataset.feature_stats on device tensors, and ddpm_run with params["eval_fidelity"].

Integer-valued features make every partial sum an integer below 2^53, so those results are compared BIT FOR BIT with numpy int64
arithmetic, whatever the order of summation.  Random features are held to the standard forward-error bounds of fp64 sums, computed
here from the absolute values of the data (u = 2^-53); they cover the kernel and the fp64 oracle together, so nothing is measured:
    moments   |outer - oracle| <= 2 (n + 8) u (|X|^T |X|) per element, |sum - oracle| <= 2 (n + 8) u sum_r |X|
    MMD sums  |got - oracle|   <= 2 (3 (D + 2) + m^2) u sum_ij (gamma sum_d |a_id| |b_jd| + |coef0|)^degree
Every test here needs the two entry points, which the library did not have before this feature."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import note

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
CANARY = -7777.0


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _oracle():
    import afdm  # noqa: F401
    return sys.modules["afdm.fidelity"]


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _scaled(n, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, D, generator=g) * (0.2 + 1.3 * torch.rand(D, generator=g)) + (2 * torch.rand(D, generator=g) - 1)


def _bits(t):
    return t.contiguous().view(torch.int64)


def _moments_abi(afdm, X, sum_in=None, outer_in=None, fill=0xFF):
    """The C ABI with raw pointers: the outputs sit inside longer buffers whose other elements must come back untouched, and the
    workspace is pre-filled with the byte `fill`.  sum_in / outer_in: what the outputs hold before an accumulating call."""
    L = afdm.lib()
    n, D = X.shape
    need = L.afd_feature_moments_workspace_bytes(n, D)
    assert 0 < need <= 256 << 20
    ws = torch.full((need + 64,), fill, device=X.device, dtype=torch.uint8)
    s = torch.full((D + 16,), CANARY, device=X.device, dtype=torch.float64)
    o = torch.full((D * D + 16,), CANARY, device=X.device, dtype=torch.float64)
    if sum_in is not None:
        s[:D] = sum_in
        o[:D * D] = outer_in.reshape(-1)
    L.afd_feature_moments_f32(X.data_ptr(), n, D, s.data_ptr(), o.data_ptr(), int(sum_in is not None), ws.data_ptr(), need, afdm.ops._stream())
    assert bool((ws[need:] == fill).all()) and bool((s[D:] == CANARY).all()) and bool((o[D * D:] == CANARY).all())
    return s[:D].clone(), o[:D * D].view(D, D).clone()


def _mmd_abi(afdm, a, b, ia, ib, degree, gamma, coef0, fill=0xFF):
    L = afdm.lib()
    (na, D), nb, (S, m) = a.shape, b.shape[0], ia.shape
    need = L.afd_poly_mmd_workspace_bytes(S, m, D)
    assert 0 < need <= 64 << 20
    ws = torch.full((need + 64,), fill, device=a.device, dtype=torch.uint8)
    sums = torch.full((3 * S + 16,), CANARY, device=a.device, dtype=torch.float64)
    L.afd_poly_mmd_sums_f32(a.data_ptr(), na, b.data_ptr(), nb, D, ia.data_ptr(), ib.data_ptr(), S, m, degree, gamma, coef0, sums.data_ptr(),
                            ws.data_ptr(), need, afdm.ops._stream())
    assert bool((ws[need:] == fill).all()) and bool((sums[3 * S:] == CANARY).all())
    return sums[:3 * S].view(S, 3).clone()


# ---- 1. moments ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (1, 15, 16, 17, 33, 200))
def test_moments_of_integer_features_bit_for_bit(A, D):
    afdm, dev = A
    for n in (1, 3, 4, 5, 63, 64, 65, 1001):
        x = _ints((n, D), -8, 8, 1000 * D + n)
        xi = x.numpy().astype(np.int64)
        want_sum, want_outer = torch.from_numpy(xi.sum(0).astype(np.float64)), torch.from_numpy((xi.T @ xi).astype(np.float64))
        xd = x.to(dev)
        s, o = _moments_abi(afdm, xd)
        assert torch.equal(s.cpu(), want_sum) and torch.equal(o.cpu(), want_outer), (n, D)
        assert torch.equal(_bits(o), _bits(o.T)), (n, D)
        s2, o2 = afdm.ops.feature_moments(xd)
        assert torch.equal(_bits(s2), _bits(s)) and torch.equal(_bits(o2), _bits(o)), (n, D)
        if n >= 3:                                           # three uneven chunks, accumulating: the same bits
            cuts = (0, 1, 2 + (n - 3) // 3, n)
            sa = oa = None
            for lo, hi in zip(cuts, cuts[1:]):
                sa, oa = _moments_abi(afdm, xd[lo:hi], sa, oa)
            assert torch.equal(_bits(sa), _bits(s)) and torch.equal(_bits(oa), _bits(o)), (n, D)
            st = afdm.FeatureStats(D, dev)
            for lo, hi in zip(cuts, cuts[1:]):
                st.update(xd[lo:hi])
            assert st.n == n and torch.equal(_bits(st.sum), _bits(s)) and torch.equal(_bits(st.outer), _bits(o)), (n, D)


@pytest.mark.parametrize("n,D", ((257, 48), (2050, 200), (5, 300)))
def test_moments_of_random_features_within_the_fp64_bound(A, n, D):
    afdm, dev = A
    x = _scaled(n, D, 7 * n + D)
    x64 = x.numpy().astype(np.float64)
    want_sum, want_outer = x64.sum(0), x64.T @ x64
    bound_sum, bound_outer = 2 * (n + 8) * U * np.abs(x64).sum(0), 2 * (n + 8) * U * (np.abs(x64).T @ np.abs(x64))
    s, o = _moments_abi(afdm, x.to(dev))
    rs = float((np.abs(s.cpu().numpy() - want_sum) / bound_sum).max())
    ro = float((np.abs(o.cpu().numpy() - want_outer) / bound_outer).max())
    print(f"moments ({n}, {D}): worst error / bound: sum {rs:.3e}, outer {ro:.3e}")
    note("fidelity moments sum error / fp64 bound (gate 1)", rs, f"({n}, {D})")
    note("fidelity moments outer error / fp64 bound (gate 1)", ro, f"({n}, {D})")
    assert rs <= 1 and ro <= 1
    assert torch.equal(_bits(o), _bits(o.T))
    # FeatureStats / feature_stats on the device against the cpu path
    got, want = afdm.feature_stats(x.to(dev), batch=100), afdm.feature_stats(x, batch=100)
    assert got.sum.is_cuda and got.n == want.n == n
    assert bool(((got.outer.cpu() - want.outer).abs() <= torch.from_numpy(bound_outer)).all())
    # cov = (outer - sum sum^T / n) / (n - 1): the two bounds carried through, plus 8 u of the terms' magnitudes for its own roundings
    big_s = np.abs(want_sum) + bound_sum
    bound_cov = (bound_outer + (np.outer(big_s, bound_sum) + np.outer(bound_sum, big_s)) / n
                 + 8 * U * (np.abs(want_outer) + np.outer(big_s, big_s) / n)) / (n - 1)
    assert bool(((got.cov().cpu() - want.cov()).abs() <= torch.from_numpy(bound_cov)).all())
    assert bool(((got.mean().cpu() - want.mean()).abs() <= torch.from_numpy(bound_sum / n + 2 * U * big_s / n)).all())


# ---- 2. the same bits from call to call -----------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_whatever_the_workspace_held(A):
    afdm, dev = A
    x = _scaled(2050, 200, 21).to(dev)
    first = _moments_abi(afdm, x, fill=0x00)
    for fill in (0xFF, 0x7F):
        again = _moments_abi(afdm, x, fill=fill)
        assert torch.equal(_bits(again[0]), _bits(first[0])) and torch.equal(_bits(again[1]), _bits(first[1]))
    a, b = _randn((300, 200), 22).to(dev), _randn((211, 200), 23).to(dev)
    ia = torch.randint(0, 300, (7, 100), generator=torch.Generator().manual_seed(24)).to(dev)
    ib = torch.randint(0, 211, (7, 100), generator=torch.Generator().manual_seed(25)).to(dev)
    first = _mmd_abi(afdm, a, b, ia, ib, 3, 1.0 / 200, 1.0, fill=0x00)
    for fill in (0xFF, 0x7F):
        assert torch.equal(_bits(_mmd_abi(afdm, a, b, ia, ib, 3, 1.0 / 200, 1.0, fill=fill)), _bits(first))
    assert torch.equal(_bits(afdm.ops.poly_mmd_sums(a, b, ia, ib, 3, 1.0 / 200, 1.0)), _bits(first))


# ---- 3. views that start inside an allocation, and strided ones -----------------------------------------------------------------
def _offset_view(t, dev, skip_bytes):
    flat = t.contiguous().view(-1).view(torch.uint8)
    buf = torch.empty(flat.numel() + 64, device=dev, dtype=torch.uint8)
    view = buf[skip_bytes:skip_bytes + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == skip_bytes
    return view.view(t.dtype).view(t.shape)


def test_features_that_start_inside_their_allocation_or_are_strided(A):
    afdm, dev = A
    x = _scaled(65, 33, 31)
    s, o = afdm.ops.feature_moments(x.to(dev))
    moved = afdm.ops.feature_moments(_offset_view(x, dev, 4))
    assert torch.equal(_bits(moved[0]), _bits(s)) and torch.equal(_bits(moved[1]), _bits(o))
    wide = torch.zeros(65, 66)
    wide[:, ::2] = x
    strided = wide.to(dev)[:, ::2]
    assert not strided.is_contiguous()
    got = afdm.ops.feature_moments(strided)
    assert torch.equal(_bits(got[0]), _bits(s)) and torch.equal(_bits(got[1]), _bits(o))
    a, b = _randn((40, 17), 32), _randn((30, 17), 33)
    ia = torch.randint(0, 40, (3, 17), generator=torch.Generator().manual_seed(34)).to(dev)
    ib = torch.randint(0, 30, (3, 17), generator=torch.Generator().manual_seed(35)).to(dev)
    want = afdm.ops.poly_mmd_sums(a.to(dev), b.to(dev), ia, ib, 3, 0.1, 1.0)
    got = afdm.ops.poly_mmd_sums(_offset_view(a, dev, 4), _offset_view(b, dev, 12), ia, ib, 3, 0.1, 1.0)
    assert torch.equal(_bits(got), _bits(want))
    got = afdm.ops.poly_mmd_sums(a.T.contiguous().to(dev).T, b.to(dev), ia, ib, 3, 0.1, 1.0)
    assert torch.equal(_bits(got), _bits(want))


# ---- 4. NaN ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,r,c", ((70, 200, 33, 70), (5, 17, 4, 16), (130, 64, 0, 0)))
def test_a_nan_feature_makes_exactly_its_column_and_row_nan(A, n, D, r, c):
    afdm, dev = A
    x = _scaled(n, D, 41)
    clean_s, clean_o = afdm.ops.feature_moments(x.to(dev))
    x[r, c] = float("nan")
    s, o = afdm.ops.feature_moments(x.to(dev))
    want_s = torch.zeros(D, dtype=torch.bool)
    want_s[c] = True
    want_o = torch.zeros(D, D, dtype=torch.bool)
    want_o[c, :] = True
    want_o[:, c] = True
    assert torch.equal(torch.isnan(s).cpu(), want_s) and torch.equal(torch.isnan(o).cpu(), want_o)
    assert not bool(torch.isnan(clean_s).any()) and not bool(torch.isnan(clean_o).any())
    keep = ~want_o.to(dev)
    assert torch.equal(o[keep], clean_o[keep]) and torch.equal(s[~want_s.to(dev)], clean_s[~want_s.to(dev)])


def test_a_nan_row_reaches_only_the_subsets_that_index_it(A):
    afdm, dev = A
    a, b = _randn((40, 33), 42), _randn((30, 33), 43)
    g = torch.Generator().manual_seed(44)
    others = torch.tensor([i for i in range(40) if i != 5])
    ia = torch.stack([others[torch.randperm(39, generator=g)[:20]] for _ in range(4)])
    ia[0, 7] = 5
    ia[2, 19] = 5
    ib = torch.stack([torch.randperm(30, generator=g)[:20] for _ in range(4)])
    clean = afdm.ops.poly_mmd_sums(a.to(dev), b.to(dev), ia.to(dev), ib.to(dev), 3, 1 / 33, 1.0)
    a[5, 20] = float("nan")
    got = afdm.ops.poly_mmd_sums(a.to(dev), b.to(dev), ia.to(dev), ib.to(dev), 3, 1 / 33, 1.0)
    want = torch.zeros(4, 3, dtype=torch.bool)
    want[0, 0] = want[0, 2] = want[2, 0] = want[2, 2] = True
    assert torch.equal(torch.isnan(got).cpu(), want) and not bool(torch.isnan(clean).any())
    assert torch.equal(got.cpu()[~want], clean.cpu()[~want])


# ---- 5. MMD sums -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def int_sets():
    return {D: (_ints((300, D), -3, 3, 50 + D), _ints((211, D), -3, 3, 60 + D)) for D in (1, 17, 200)}


@pytest.mark.parametrize("m", (2, 15, 16, 17, 65, 100))
def test_mmd_sums_of_integer_features_bit_for_bit(A, int_sets, m):
    """gamma = coef0 = 1 and integer features: every kernel value and every partial sum is an integer below 2^53 (at most
    100^2 (9 * 200 + 1)^3 < 6e13).  This pins the i != j masks of the diagonal tiles, the doubling of the upper triangle, the gather
    (indices repeat within and across subsets) and the tails in m and D."""
    afdm, dev = A
    for D, (a, b) in int_sets.items():
        ai, bi = a.numpy().astype(np.int64), b.numpy().astype(np.int64)
        ad, bd = a.to(dev), b.to(dev)
        for S in (1, 3, 7):
            g = torch.Generator().manual_seed(1000 * m + 10 * S + D)
            ia, ib = torch.randint(0, 300, (S, m), generator=g), torch.randint(0, 211, (S, m), generator=g)
            for degree in (1, 2, 3):
                want = np.empty((S, 3), dtype=np.int64)
                for s in range(S):
                    x, y = ai[ia[s].numpy()], bi[ib[s].numpy()]
                    kxx, kyy, kxy = (x @ x.T + 1) ** degree, (y @ y.T + 1) ** degree, (x @ y.T + 1) ** degree
                    want[s] = (kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum())
                assert np.abs(want).max() < 2 ** 53
                got = _mmd_abi(afdm, ad, bd, ia.to(dev), ib.to(dev), degree, 1.0, 1.0)
                assert torch.equal(got.cpu(), torch.from_numpy(want.astype(np.float64))), (m, S, D, degree)
                assert torch.equal(_bits(afdm.ops.poly_mmd_sums(ad, bd, ia.to(dev), ib.to(dev), degree, 1.0, 1.0)), _bits(got))


@pytest.mark.parametrize("kind", ("randn", "abs"))
@pytest.mark.parametrize("m,S,D", ((100, 3, 200), (65, 2, 17), (17, 5, 333)))
def test_mmd_sums_of_random_features_within_the_fp64_bound(A, kind, m, S, D):
    afdm, dev = A
    F = _oracle()
    a, b = _randn((300, D), 71), _randn((211, D), 72)
    if kind == "abs":
        a, b = a.abs(), b.abs()
    g = torch.Generator().manual_seed(73)
    ia, ib = torch.randint(0, 300, (S, m), generator=g), torch.randint(0, 211, (S, m), generator=g)
    gamma, coef0, degree = 1.0 / D, 1.0, 3
    want = afdm.mmd_sums(a, b, ia, ib, degree, None, coef0)
    bound = 2 * (3 * (D + 2) + m * m) * U * F._mmd_sums_torch(a.abs(), b.abs(), ia, ib, degree, gamma, abs(coef0))
    got = afdm.mmd_sums(a.to(dev), b.to(dev), ia, ib, degree, None, coef0)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (S, 3)
    ratio = float(((got.cpu() - want).abs() / bound).max())
    print(f"MMD sums {kind} m={m} S={S} D={D}: worst error / bound {ratio:.3e}")
    note("fidelity MMD sums error / fp64 bound (gate 1)", ratio, f"{kind} m={m} S={S} D={D}")
    assert ratio <= 1


def test_an_index_out_of_range_is_refused_before_any_launch(A):
    afdm, dev = A
    a, b = _randn((40, 17), 81).to(dev), _randn((30, 17), 82).to(dev)
    ok = torch.zeros(2, 5, dtype=torch.long, device=dev)
    for bad_a, bad_b in ((40, 0), (-1, 0), (0, 30), (0, -7)):
        ia, ib = ok.clone(), ok.clone()
        ia[1, 3], ib[0, 4] = bad_a, bad_b
        with pytest.raises(afdm.AfdError, match="an index lies outside its array"):
            afdm.ops.poly_mmd_sums(a, b, ia, ib, 3, 0.1, 1.0)
        with pytest.raises(ValueError, match="index lies outside"):
            afdm.mmd_sums(a, b, ia, ib)
    for kw, match in (({"degree": 9}, "degree must be"), ({"ia": ok[:1]}, "ia and ib must have one shape"), ({"a": a.double()}, "a must be"),
                      ({"b": b[:, :16]}, "one row size"), ({"ib": ok.int()}, "ib must be")):
        args = dict({"a": a, "b": b, "ia": ok, "ib": ok, "degree": 3}, **kw)
        with pytest.raises(afdm.AfdError, match=match):
            afdm.ops.poly_mmd_sums(args["a"], args["b"], args["ia"], args["ib"], args["degree"], 0.1, 1.0)
    with pytest.raises(afdm.AfdError, match="sum and outer go together"):
        afdm.ops.feature_moments(a, sum=torch.zeros(17, dtype=torch.float64, device=dev))
    with pytest.raises(afdm.AfdError, match="features must be"):
        afdm.ops.feature_moments(a.cpu())


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def _u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_fidelity_on_the_device_against_the_cpu_path(A):
    """FID goes through two eigendecompositions of covariances formed with cancellation, so it is held to a relative 1e-9 (printed).
    A KID value is v = AA / (m (m - 1)) + BB / (m (m - 1)) - 2 AB / m^2, so its bound is the sums' bounds combined with the same
    weights, plus 8 u of the terms' magnitudes for the three divisions and two additions; the mean moves by at most the largest
    such bound, and so does the population standard deviation (it is 1-Lipschitz in the largest deviation of a value)."""
    afdm, dev = A
    F = _oracle()
    gen, ref = _u8((600, 3, 8, 8), 91), _u8((700, 3, 8, 8), 92)
    S, m, D = 5, 100, 192
    want = afdm.fidelity(gen, ref, "pixels", kid_subsets=S, kid_subset_size=m)
    got = afdm.fidelity(gen.to(dev), ref.to(dev), "pixels", kid_subsets=S, kid_subset_size=m)
    assert set(got) == set(want) == {"frechet_inception_distance", "kernel_inception_distance_mean", "kernel_inception_distance_std"}
    rel = abs(got["frechet_inception_distance"] - want["frechet_inception_distance"]) / want["frechet_inception_distance"]
    print(f"FID device {got['frechet_inception_distance']:.12g} cpu {want['frechet_inception_distance']:.12g}: relative difference {rel:.3e}")
    note("fidelity FID device against cpu, relative (gate 1e-9)", rel, "600 + 700 images of 3 x 8 x 8")
    assert rel <= 1e-9
    fg, fr = afdm.extract_features("pixels", gen)[0], afdm.extract_features("pixels", ref)[0]
    fgd, logits = afdm.extract_features("pixels", gen.to(dev))
    assert logits is None and fgd.is_cuda and torch.equal(fgd.cpu(), fg)
    ia, ib = (torch.from_numpy(t) for t in afdm.mmd_indices(600, 700, S, m, 2020))
    sums = F._mmd_sums_torch(fg, fr, ia, ib, 3, 1.0 / D, 1.0)
    sums_bound = 2 * (3 * (D + 2) + m * m) * U * F._mmd_sums_torch(fg.abs(), fr.abs(), ia, ib, 3, 1.0 / D, 1.0)
    w = torch.tensor([1.0 / (m * (m - 1)), 1.0 / (m * (m - 1)), 2.0 / (m * m)], dtype=torch.float64)
    bound = float(((sums_bound * w).sum(1) + 8 * U * (sums.abs() * w).sum(1)).max())
    for key in ("kernel_inception_distance_mean", "kernel_inception_distance_std"):
        print(f"{key}: device {got[key]:.12g} cpu {want[key]:.12g}, difference {abs(got[key] - want[key]):.3e}, bound {bound:.3e}")
        note("fidelity KID device against cpu / bound (gate 1)", abs(got[key] - want[key]) / bound, key)
        assert abs(got[key] - want[key]) <= bound
    kid = afdm.kernel_distance(fgd, afdm.extract_features("pixels", ref.to(dev))[0], subsets=S, subset_size=m)
    assert kid["values"].is_cuda and kid["mean"] == got["kernel_inception_distance_mean"]
    # the store's method: the same batches, the same bits
    store = afdm.DeviceDataset(ref, device=dev)
    st = store.feature_stats("pixels", batch=256)
    same = afdm.feature_stats(afdm.extract_features("pixels", ref.to(dev))[0], batch=256)
    assert st.n == 700 and st.sum.is_cuda and torch.equal(_bits(st.sum), _bits(same.sum)) and torch.equal(_bits(st.outer), _bits(same.outer))
    part, same = store.feature_stats("pixels", n=300, batch=128), afdm.feature_stats(fr[:300].to(dev), batch=128)
    assert part.n == 300 and torch.equal(_bits(part.sum), _bits(same.sum)) and torch.equal(_bits(part.outer), _bits(same.outer))
    back = afdm.FeatureStats.from_state(st.state(), device=dev)
    assert back.n == 700 and torch.equal(back.outer, st.outer) and afdm.frechet_distance(back, st) == pytest.approx(0, abs=1e-6)


def test_ddpm_run_with_eval_fidelity(A, tmp_path, monkeypatch):
    from PIL import Image
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    cfg = {"n": 16, "extractor": "pixels", "kid_subsets": 3, "kid_subset_size": 8}
    runs = {}
    for key in ("plain", "fidelity"):
        wd = tmp_path / key
        wd.mkdir()
        np.savetxt(wd / "mnist.csv", arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 8, "gen_total": 16, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "fidelity":
            params["eval_fidelity"] = dict(cfg)
        out = afdm.ddpm_run(params)
        run_dir = os.path.join("runs", "DDPM_Uncondtional_MNIST_3")
        runs[key] = (out, open(os.path.join(run_dir, "settings_MNIST_3.txt")).read().replace(str(wd), ""), str(wd / run_dir))
    (po, pt, pdir), (fo, ft, fdir) = runs["plain"], runs["fidelity"]
    assert "fidelity" not in po and pt == ft and po["loss_all"] == fo["loss_all"]
    assert not [f for f in os.listdir(pdir) if f.startswith("fidelity")]
    assert sorted(os.listdir(fdir)) == sorted(os.listdir(pdir) + ["fidelity_MNIST_3.json"])

    def saved(out):
        return torch.stack([torch.from_numpy(np.array(Image.open(os.path.join(out["gen_dir"], f"image_{i}.png")))) for i in range(16)])
    images = saved(fo)
    assert torch.equal(images, saved(po))                   # the same generated images with and without the key
    res = fo["fidelity"]
    keys = {"frechet_inception_distance", "kernel_inception_distance_mean", "kernel_inception_distance_std"}
    assert set(res) == keys and all(isinstance(v, float) and math.isfinite(v) for v in res.values())
    with open(os.path.join(fdir, "fidelity_MNIST_3.json")) as fh:
        written = json.load(fh)
    assert {k: written[k] for k in keys} == res and written["n"] == 16 and written["kid_subsets"] == 3 and written["kid_subset_size"] == 8
    # the saved samples against the training tensors, on the cpu (16 rows of 1024 features: the covariances are rank-deficient, where
    # FID carries sqrt(u)-sized noise per zero eigenvalue, so only KID is compared closely)
    monkeypatch.chdir(tmp_path / "fidelity")
    train = afdm.get_data_MNIST(afdm.argument(dataset_path="mnist.csv", batch_size=8))[1].tensors[0]
    pixels = afdm.DeviceDataset(train[:16], device="cpu").pixels()
    want = afdm.fidelity(images.view(16, 1, 32, 32), pixels, "pixels", kid_subsets=3, kid_subset_size=8)
    for key in ("kernel_inception_distance_mean", "kernel_inception_distance_std"):
        assert res[key] == pytest.approx(want[key], rel=1e-9, abs=1e-12), key
    # FID: an eigenvalue of the (1024 x 1024, rank 15) product comes back within D u |M|, |M| <= tr S_a tr S_b, so each of the D square
    # roots within sqrt(D u tr S_a tr S_b); D of them, doubled in the formula, on both sides of the comparison
    fs = [afdm.feature_stats(afdm.extract_features("pixels", x)[0]) for x in (images.view(16, 1, 32, 32), pixels)]
    tol = 4 * 1024 * math.sqrt(1024 * U * float(fs[0].cov().trace()) * float(fs[1].cov().trace()))
    print(f"ddpm_run FID {res['frechet_inception_distance']:.9g} cpu {want['frechet_inception_distance']:.9g} tolerance {tol:.3g}")
    assert abs(res["frechet_inception_distance"] - want["frechet_inception_distance"]) <= tol < 0.01 * want["frechet_inception_distance"]
    with pytest.raises(ValueError, match="eval_fidelity n must be"):
        afdm.ddpm_run(dict(params, eval_fidelity=dict(cfg, n=17)))      # more than gen_total: fails before any training
    data = {"args": afdm.argument(image_size=32, image_channels=1, device="cuda", noise_steps=6), "unet_v": 3, "seed": 42,
            "f_settings": {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2},
            "modelpath": fo["modelpath"]}
    r = afdm.fidelity_results(data, train, 16, "pixels", kid_subsets=3, kid_subset_size=8)
    assert set(r) == keys and all(math.isfinite(v) for v in r.values())
    with pytest.raises(ValueError, match="fidelity_results: n must be an int in"):
        afdm.fidelity_results(data, train, 17, "pixels")
