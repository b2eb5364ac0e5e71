"""FID, KID and Inception Score, host side: the C ABI's entry points and their argument checks (no GPU is touched), FeatureStats on
cpu tensors against numpy, frechet_distance against closed forms and a numpy-only oracle, kernel_distance's index draw and its
MMD^2 against a double loop, inception_score, extract_features and the eval_fidelity key of ddpm_run."""
import ctypes

import numpy as np
import pytest
import torch

ENTRY_POINTS = ("afd_feature_moments_workspace_bytes", "afd_feature_moments_f32", "afd_poly_mmd_workspace_bytes", "afd_poly_mmd_sums_f32")


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg, sz, it, db = ctypes.c_void_p, ctypes.c_long, ctypes.c_size_t, ctypes.c_int, ctypes.c_double
    want = {"afd_feature_moments_workspace_bytes": (sz, [lg, lg]),
            "afd_feature_moments_f32": (it, [vp, lg, lg, vp, vp, it, vp, sz, vp]),
            "afd_poly_mmd_workspace_bytes": (sz, [lg, lg, lg]),
            "afd_poly_mmd_sums_f32": (it, [vp, lg, vp, lg, lg, vp, vp, lg, lg, it, db, db, vp, vp, sz, vp])}
    for name in ENTRY_POINTS:
        assert name in sigs, name
        assert sigs[name] == want[name], name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))


def test_moments_reject_bad_arguments_before_any_launch():
    from afdm import AfdError, lib
    L = lib()
    n, D = 100, 48
    need = L.afd_feature_moments_workspace_bytes(n, D)
    assert need > 0 and need % 8 == 0
    good = {"X": 1 << 24, "n": n, "D": D, "sum": 2 << 24, "outer": 3 << 24, "accumulate": 0, "workspace": 4 << 24, "bytes": need}

    def bad(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(AfdError, match=match):
            L.afd_feature_moments_f32(a["X"], a["n"], a["D"], a["sum"], a["outer"], a["accumulate"], a["workspace"], a["bytes"], None)

    for name in ("X", "sum", "outer"):
        bad("X, sum and outer must not be NULL", **{name: None})
    bad("workspace must not be NULL", workspace=None)
    for name in ("n", "D"):
        for v in (0, -3):
            bad("n and D must be positive", **{name: v})
    bad(r"n must be below 2\^31", n=1 << 31, bytes=1 << 40)
    bad(r"D at most 2\^15", D=(1 << 15) + 1, bytes=1 << 40)
    for v in (2, -1):
        bad("accumulate must be 0 or 1", accumulate=v)
    bad("X must be 4-byte aligned", X=good["X"] + 2)
    for name in ("sum", "outer", "workspace"):
        bad("must be 8-byte aligned", **{name: good[name] + 4})
    bad("workspace too small", bytes=need - 1)
    bad("workspace too small", bytes=0)
    for out in ("sum", "outer", "workspace"):
        bad("must not overlap X", **{out: good["X"] + n * D * 4 - 8})
        bad("must not overlap X", **{out: good["X"]})
    bad("must not overlap each other", outer=good["sum"] + D * 8 - 8)
    bad("must not overlap each other", workspace=good["outer"] + 8)
    bad("must not overlap each other", workspace=good["sum"] - need + 8)


def test_mmd_sums_reject_bad_arguments_before_any_launch():
    from afdm import AfdError, lib
    L = lib()
    na, nb, D, S, m = 300, 211, 17, 3, 20
    need = L.afd_poly_mmd_workspace_bytes(S, m, D)
    assert need > 0 and need % 8 == 0
    good = {"A": 1 << 24, "na": na, "B": 2 << 24, "nb": nb, "D": D, "ia": 3 << 24, "ib": 4 << 24, "S": S, "m": m, "degree": 3, "gamma": 0.5,
            "coef0": 1.0, "sums": 5 << 24, "workspace": 6 << 24, "bytes": need}

    def bad(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(AfdError, match=match):
            L.afd_poly_mmd_sums_f32(a["A"], a["na"], a["B"], a["nb"], a["D"], a["ia"], a["ib"], a["S"], a["m"], a["degree"], a["gamma"],
                                    a["coef0"], a["sums"], a["workspace"], a["bytes"], None)

    for name in ("A", "B", "ia", "ib", "sums"):
        bad("A, B, ia, ib and sums must not be NULL", **{name: None})
    bad("workspace must not be NULL", workspace=None)
    for name in ("na", "nb", "D", "S"):
        for v in (0, -3):
            bad("na, nb, D and S must be positive", **{name: v})
    for v in (1, 0, -5):
        bad("m must be at least 2", m=v)
    bad(r"m must be at most", m=(1 << 16) + 1, bytes=1 << 40)
    for v in (0, 9, -1):
        bad(r"degree must lie in \[1, 8\]", degree=v)
    for name in ("A", "B"):
        bad("A and B must be 4-byte aligned", **{name: good[name] + 2})
    for name in ("ia", "ib", "sums", "workspace"):
        bad("must be 8-byte aligned", **{name: good[name] + 4})
    bad("workspace too small", bytes=need - 1)
    bad("workspace too small", bytes=0)
    ends = {"A": na * D * 4, "B": nb * D * 4, "ia": S * m * 8, "ib": S * m * 8}
    for out in ("sums", "workspace"):
        for name, size in ends.items():
            bad(f"must not overlap {name}", **{out: good[name] + (size - 8) // 8 * 8})
            bad(f"must not overlap {name}", **{out: good[name]})
    bad("must not overlap each other", workspace=good["sums"] + 8)
    bad("must not overlap each other", workspace=good["sums"] - need + 8)


def test_workspace_sizes():
    from afdm import lib
    L = lib()
    mom, mmd = L.afd_feature_moments_workspace_bytes, L.afd_poly_mmd_workspace_bytes
    assert mom(1, 1) == (64 * 64 + 64) * 8                     # one tile, one slab, and its column sums
    assert mom(50000, 2048) == 3 * (528 * 64 * 64 + 32 * 64) * 8          # 528 tiles on or above the diagonal, 2048 // 528 slabs
    assert mom(10 ** 6, 200) == mom(10 ** 5, 200) == 64 * (10 * 64 * 64 + 4 * 64) * 8     # at most 64 slabs, whatever n
    assert mmd(1, 2, 1) == 3 * 8 and mmd(100, 1000, 2048) == 100 * (2 * 136 + 256) * 8
    for bad in ((0, 1), (1, 0), (-1, 5), (1 << 31, 1), (1, (1 << 15) + 1)):
        assert mom(*bad) == 0, bad
    for bad in ((0, 2, 1), (1, 1, 1), (1, 2, 0), (1, (1 << 16) + 1, 1), (1 << 31, 2, 1)):
        assert mmd(*bad) == 0, bad


# ---- FeatureStats ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D", ((257, 48), (5, 30), (2, 1)))
def test_feature_stats_on_cpu_against_numpy(n, D):
    import afdm
    x = _randn((n, D), 1) * (0.2 + 1.3 * torch.rand(D, generator=torch.Generator().manual_seed(2))) + 0.5
    st = afdm.feature_stats(x)
    assert st.n == n and st.mean().dtype == torch.float64 and st.cov().dtype == torch.float64
    x64 = x.numpy().astype(np.float64)
    np.testing.assert_allclose(st.mean().numpy(), np.mean(x64, axis=0), rtol=1e-12, atol=1e-14)
    want = np.cov(x64, rowvar=False).reshape(D, D)
    np.testing.assert_allclose(st.cov().numpy(), want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()))
    with pytest.raises(ValueError, match="at least 2 rows"):
        afdm.feature_stats(x[:1]).cov()
    for bad in (x.double(), x[0], x[:, :0], "features"):
        with pytest.raises(ValueError, match="features must be"):
            afdm.feature_stats(bad)
    with pytest.raises(ValueError, match=f"\\(n, {D}\\) float32"):
        st.update(torch.zeros(3, D + 1))


def test_chunked_updates_equal_one_shot_and_state_round_trip(tmp_path):
    import afdm
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-8, 9, (1001, 33), generator=g).float()
    one = afdm.feature_stats(x)
    st = afdm.FeatureStats(33, "cpu")
    for a, b in ((0, 1), (1, 400), (400, 1001)):
        st.update(x[a:b])
    batched = afdm.feature_stats(x, batch=64)
    xi = x.numpy().astype(np.int64)
    for s in (one, st, batched):
        assert s.n == 1001
        assert np.array_equal(s.sum.numpy(), xi.sum(0).astype(np.float64)) and np.array_equal(s.outer.numpy(), (xi.T @ xi).astype(np.float64))
    state = st.state()
    assert set(state) == {"n", "sum", "outer"} and state["sum"].dtype == state["outer"].dtype == np.float64
    np.savez(tmp_path / "stats.npz", **state)
    with np.load(tmp_path / "stats.npz") as z:
        back = afdm.FeatureStats.from_state(z)
    assert back.n == st.n and torch.equal(back.sum, st.sum) and torch.equal(back.outer, st.outer) and torch.equal(back.cov(), st.cov())
    back.update(x[:7])
    assert back.n == 1008 and st.n == 1001
    with pytest.raises(ValueError, match="from_state"):
        afdm.FeatureStats.from_state({"n": 3, "sum": np.zeros(4), "outer": np.zeros((4, 5))})


# ---- frechet_distance --------------------------------------------------------------------------------------------------------------
def _orthogonal(D, seed):
    return torch.linalg.qr(torch.randn(D, D, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))[0]


def test_frechet_distance_of_identical_stats_is_zero():
    import afdm
    x = _randn((600, 48), 4)
    st = afdm.feature_stats(x)
    assert abs(afdm.frechet_distance(st, st)) <= 1e-9 * float(st.cov().trace())
    assert abs(afdm.frechet_distance(st, (st.mean(), st.cov()))) <= 1e-9 * float(st.cov().trace())


@pytest.mark.parametrize("D", (48, 200))
def test_frechet_distance_of_commuting_covariances(D):
    """S_a = Q diag(a) Q^T and S_b = Q diag(b) Q^T: the distance is sum (sqrt a - sqrt b)^2 + |mu_a - mu_b|^2.  Condition numbers are
    at most 4, so the eigenvalue errors are of the order D u, about 1e-13 at worst: the gate is 1e-12."""
    import afdm
    g = torch.Generator().manual_seed(D)
    Q = _orthogonal(D, 5)
    a, b = (0.5 + 1.5 * torch.rand(D, generator=g, dtype=torch.float64) for _ in range(2))
    mu_a, mu_b = (torch.randn(D, generator=g, dtype=torch.float64) for _ in range(2))
    want = float(((a.sqrt() - b.sqrt()) ** 2).sum() + ((mu_a - mu_b) ** 2).sum())
    got = afdm.frechet_distance((mu_a, (Q * a) @ Q.T), (mu_b, (Q * b) @ Q.T))
    print(f"commuting D={D}: relative error {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-12 * want
    assert afdm.frechet_distance((mu_b, (Q * b) @ Q.T), (mu_a, (Q * a) @ Q.T)) == pytest.approx(want, rel=1e-12)


def _frechet_numpy(xa, xb):
    """numpy only: tr sqrt from the eigenvalues of the (non-symmetric) product S_a S_b, real parts clipped at 0."""
    mu_a, mu_b = xa.mean(0), xb.mean(0)
    ca, cb = np.cov(xa, rowvar=False), np.cov(xb, rowvar=False)
    ev = np.clip(np.linalg.eigvals(ca @ cb).real, 0, None)
    return float(((mu_a - mu_b) ** 2).sum() + np.trace(ca) + np.trace(cb) - 2 * np.sqrt(ev).sum())


@pytest.mark.parametrize("D,n,tol", ((48, 24, 1e-6), (96, 48, 1e-6), (200, 100, 1e-6), (48, 144, 1e-12)))
def test_frechet_distance_of_sampled_data_against_numpy(D, n, tol):
    """n = D / 2 rows: rank-deficient covariances, where the numpy oracle's own zero eigenvalues carry sqrt(u)-sized noise (hence
    1e-6); n = 3 D: full rank, held to 1e-12."""
    import afdm
    xa, xb = _randn((n, D), 6) * 1.3 + 0.2, _randn((n, D), 7) * 0.8 - 0.1
    got = afdm.frechet_distance(afdm.feature_stats(xa), afdm.feature_stats(xb))
    want = _frechet_numpy(xa.numpy().astype(np.float64), xb.numpy().astype(np.float64))
    print(f"sampled D={D} n={n}: relative error {abs(got - want) / want:.2e}")
    assert np.isfinite(got) and abs(got - want) <= tol * want
    with pytest.raises(ValueError, match="different feature sizes"):
        afdm.frechet_distance(afdm.feature_stats(xa), afdm.feature_stats(xb[:, :-1].contiguous()))


# ---- kernel_distance ---------------------------------------------------------------------------------------------------------------
def test_the_index_draw_is_reproducible_and_in_the_stated_order():
    import afdm
    ia, ib = afdm.mmd_indices(50, 40, 3, 7, seed=2020)
    rng = np.random.RandomState(2020)
    for s in range(3):
        assert np.array_equal(ia[s], rng.choice(50, 7, replace=False)) and np.array_equal(ib[s], rng.choice(40, 7, replace=False))
    again = afdm.mmd_indices(50, 40, 3, 7, seed=2020)
    assert np.array_equal(ia, again[0]) and np.array_equal(ib, again[1]) and ia.dtype == np.int64
    assert not np.array_equal(ia, afdm.mmd_indices(50, 40, 3, 7, seed=2021)[0])
    assert all(len(set(row)) == 7 for row in ia) and ia.max() < 50 and ib.max() < 40


@pytest.mark.parametrize("degree,gamma,coef0", ((3, None, 1.0), (2, 0.25, 0.5), (1, 1.0, 0.0)))
def test_kernel_distance_against_a_double_loop(degree, gamma, coef0):
    import afdm
    D, m, S = 6, 5, 4
    fa, fb = _randn((11, D), 8), _randn((9, D), 9) + 0.3
    r = afdm.kernel_distance(fa, fb, subsets=S, subset_size=m, degree=degree, gamma=gamma, coef0=coef0, seed=7)
    ia, ib = afdm.mmd_indices(11, 9, S, m, seed=7)
    a, b, gm = fa.numpy().astype(np.float64), fb.numpy().astype(np.float64), 1.0 / D if gamma is None else gamma
    k = lambda x, y: (gm * float(np.dot(x, y)) + coef0) ** degree      # noqa: E731
    want = []
    for s in range(S):
        aa = sum(k(a[i], a[j]) for i in ia[s] for j in ia[s] if i != j)
        bb = sum(k(b[i], b[j]) for i in ib[s] for j in ib[s] if i != j)
        ab = sum(k(a[i], b[j]) for i in ia[s] for j in ib[s])
        want.append(aa / (m * (m - 1)) + bb / (m * (m - 1)) - 2 * ab / (m * m))
    assert tuple(r["values"].shape) == (S,) and r["values"].dtype == torch.float64
    np.testing.assert_allclose(r["values"].numpy(), want, rtol=0, atol=1e-13 * max(1.0, max(abs(w) for w in want)) * 100)
    assert r["mean"] == pytest.approx(np.mean(want), abs=1e-12) and r["std"] == pytest.approx(np.std(want), abs=1e-12)


def test_kernel_distance_argument_checks():
    import afdm
    fa, fb = _randn((11, 6), 8), _randn((9, 6), 9)
    with pytest.raises(ValueError, match="subset_size 10 exceeds the smaller feature set"):
        afdm.kernel_distance(fa, fb, subsets=2, subset_size=10)
    with pytest.raises(ValueError, match="subset_size 1000 exceeds"):
        afdm.kernel_distance(fa, fb)
    with pytest.raises(ValueError, match="fb must be"):
        afdm.kernel_distance(fa, _randn((9, 5), 1), subsets=2, subset_size=3)
    with pytest.raises(ValueError, match="subsets must be"):
        afdm.kernel_distance(fa, fb, subsets=0, subset_size=3)
    with pytest.raises(ValueError, match="degree must be"):
        afdm.kernel_distance(fa, fb, subsets=1, subset_size=3, degree=9)
    with pytest.raises(ValueError, match="index lies outside"):
        afdm.mmd_sums(fa, fb, torch.tensor([[0, 11]]), torch.tensor([[0, 1]]))
    same = afdm.kernel_distance(fa, fa, subsets=1, subset_size=11)
    assert same["std"] == 0.0 and same["mean"] == pytest.approx(float(same["values"][0]))


# ---- inception_score ---------------------------------------------------------------------------------------------------------------
def test_inception_score():
    import afdm
    assert afdm.inception_score(torch.zeros(37, 10), splits=5) == (1.0, 0.0)
    assert afdm.inception_score(torch.full((50, 1008), 3.25), splits=10) == (1.0, 0.0)
    K = 8
    onehot = torch.full((K * 20, K), -40.0)
    onehot[torch.arange(K * 20), torch.arange(K * 20) % K] = 40.0          # balanced classes in every split of 40
    mean, std = afdm.inception_score(onehot, splits=4)
    assert mean == pytest.approx(K, rel=1e-9) and std < 1e-9
    # n not divisible by splits: split k is rows [k n // splits, (k + 1) n // splits)
    logits = _randn((23, 7), 10) * 2
    mean, std = afdm.inception_score(logits, splits=4)
    lp = torch.log_softmax(logits.double(), 1).numpy()
    want = []
    for k in range(4):
        part = lp[k * 23 // 4:(k + 1) * 23 // 4]
        p = np.exp(part)
        want.append(np.exp((p * (part - np.log(p.mean(0, keepdims=True)))).sum(1).mean()))
    assert [len(lp[k * 23 // 4:(k + 1) * 23 // 4]) for k in range(4)] == [5, 6, 6, 6]
    assert mean == pytest.approx(np.mean(want), rel=1e-12) and std == pytest.approx(np.std(want), rel=1e-9)
    assert afdm.inception_score(logits.float(), splits=1)[1] == 0.0
    for bad in (0, 24, 2.0, True):
        with pytest.raises(ValueError, match="splits must be"):
            afdm.inception_score(logits, splits=bad)
    with pytest.raises(ValueError, match="logits must be"):
        afdm.inception_score(torch.zeros(5, dtype=torch.float32))


# ---- extract_features and fidelity ---------------------------------------------------------------------------------------------------
def _u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def test_extract_features():
    import afdm
    images = _u8((21, 3, 4, 5), 11)
    table = afdm.data.normalisation_table(3)
    f, logits = afdm.extract_features("pixels", images, batch=8)
    assert logits is None and f.dtype == torch.float32 and tuple(f.shape) == (21, 60)
    assert torch.equal(f, table[torch.arange(3).view(1, 3, 1, 1), images.long()].flatten(1))
    seen = []

    def both(x):
        assert x.dtype == torch.uint8 and x.dim() == 4
        seen.append(x.shape[0])
        flat = x.float().flatten(1)
        return flat[:, :7] * 2, flat[:, 7:12]

    f, logits = afdm.extract_features(both, images, batch=8)
    assert seen == [8, 8, 5] and torch.equal(f, images.float().flatten(1)[:, :7] * 2) and torch.equal(logits, images.float().flatten(1)[:, 7:12])
    for fn, match in ((lambda x: x.float(), "features must be"), (lambda x: x.double().flatten(1), "features must be"),
                      (lambda x: x.float().flatten(1)[:5], "features must be"), (lambda x: (x.float().flatten(1), x.flatten(1)), "logits must be"),
                      (lambda x: (x.float().flatten(1),) * 3, "features or \\(features, logits\\)")):
        with pytest.raises(ValueError, match=match):
            afdm.extract_features(fn, images, batch=8)
    for bad in (images.float(), images[0], "images"):
        with pytest.raises(ValueError, match="images must be"):
            afdm.extract_features("pixels", bad)
    with pytest.raises(ValueError, match="extractor must be"):
        afdm.extract_features(3, images)
    with pytest.raises(ValueError, match="batch must be"):
        afdm.extract_features("pixels", images, batch=0)


def test_a_torchscript_extractor(tmp_path):
    import afdm

    class Net(torch.nn.Module):
        def forward(self, x):
            flat = x.float().flatten(1)
            return flat[:, :6] / 255.0, flat[:, 6:16] / 32.0

    path = str(tmp_path / "extractor.pt")
    torch.jit.script(Net()).save(path)
    images = _u8((30, 1, 4, 4), 12)
    f, logits = afdm.extract_features(path, images, batch=16)
    assert torch.equal(f, images.float().flatten(1)[:, :6] / 255.0) and tuple(logits.shape) == (30, 10)
    res = afdm.fidelity(images, _u8((40, 1, 4, 4), 13), path, kid_subsets=3, kid_subset_size=10)
    assert set(res) == {"frechet_inception_distance", "kernel_inception_distance_mean", "kernel_inception_distance_std",
                        "inception_score_mean", "inception_score_std"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    assert (res["inception_score_mean"], res["inception_score_std"]) == afdm.inception_score(logits)


def test_fidelity_on_cpu_tensors_and_the_dataset_method():
    import afdm
    gen, ref = _u8((60, 3, 4, 4), 14), _u8((70, 3, 4, 4), 15)
    res = afdm.fidelity(gen, ref, "pixels", kid_subsets=5, kid_subset_size=20)
    assert set(res) == {"frechet_inception_distance", "kernel_inception_distance_mean", "kernel_inception_distance_std"}
    fg, fr = afdm.extract_features("pixels", gen)[0], afdm.extract_features("pixels", ref)[0]
    assert res["frechet_inception_distance"] == afdm.frechet_distance(afdm.feature_stats(fg), afdm.feature_stats(fr))
    kid = afdm.kernel_distance(fg, fr, subsets=5, subset_size=20)
    assert (res["kernel_inception_distance_mean"], res["kernel_inception_distance_std"]) == (kid["mean"], kid["std"])
    assert afdm.fidelity(gen, gen, "pixels", kid_subsets=2, kid_subset_size=60)["frechet_inception_distance"] == pytest.approx(0, abs=1e-7)
    with pytest.raises(ValueError, match="unknown arguments \\['subsets'\\]"):
        afdm.fidelity(gen, ref, "pixels", subsets=5)
    with pytest.raises(ValueError, match="subset_size 1000 exceeds"):
        afdm.fidelity(gen, ref, "pixels")
    store = afdm.DeviceDataset(ref, device="cpu")
    st = store.feature_stats("pixels", n=50, batch=16)
    want = afdm.feature_stats(fr[:50])
    assert st.n == 50 and torch.allclose(st.sum, want.sum, rtol=1e-13, atol=0) and torch.allclose(st.outer, want.outer, rtol=1e-13, atol=1e-12)
    assert torch.equal(store.pixels(3), ref[:3])
    floats = afdm.DeviceDataset(afdm.data.normalisation_table(3)[torch.arange(3).view(1, 3, 1, 1), ref.long()], device="cpu")
    assert torch.equal(floats.pixels(), ref)                # a float store maps back to the pixels it came from
    for bad in (0, 71, True):
        with pytest.raises(ValueError, match="n must be None or an int in"):
            store.feature_stats("pixels", n=bad)


def test_public_names():
    import afdm
    for name in ("FeatureStats", "feature_stats", "frechet_distance", "kernel_distance", "inception_score", "extract_features", "fidelity",
                 "fidelity_results", "mmd_indices", "mmd_sums"):
        assert callable(getattr(afdm, name)), name
    assert callable(afdm.ops.feature_moments) and callable(afdm.ops.poly_mmd_sums) and callable(afdm.DeviceDataset.feature_stats)
    assert "torch_fidelity" in afdm.fidelity.__globals__["__doc__"] and "no parity is claimed" in afdm.fidelity.__globals__["__doc__"]


# ---- ddpm_run ------------------------------------------------------------------------------------------------------------------------
def test_eval_fidelity_key_check():
    from afdm.tasks import _fidelity_cfg
    base = {"gen_total": 16}
    assert _fidelity_cfg(dict(base, eval_fidelity={"n": 16, "extractor": "pixels"})) == \
        {"n": 16, "extractor": "pixels", "kid_subsets": 100, "kid_subset_size": 16}
    fn = lambda x: x.float().flatten(1)      # noqa: E731
    got = _fidelity_cfg(dict(base, eval_fidelity={"n": np.int64(8), "extractor": fn, "kid_subsets": 3, "kid_subset_size": 8}))
    assert got == {"n": 8, "extractor": fn, "kid_subsets": 3, "kid_subset_size": 8} and type(got["n"]) is int
    for cfg, match in ((16, "needs n and extractor"), ({"n": 16}, "needs n and extractor"), ({"extractor": "pixels"}, "needs n and extractor"),
                       ({"n": 16, "extractor": "pixels", "window": None}, "needs n and extractor"),
                       ({"n": 17, "extractor": "pixels"}, "n must be an int in"), ({"n": 1, "extractor": "pixels"}, "n must be an int in"),
                       ({"n": True, "extractor": "pixels"}, "n must be an int in"), ({"n": 4.0, "extractor": "pixels"}, "n must be an int in"),
                       ({"n": 16, "extractor": 3}, "extractor must be"), ({"n": 16, "extractor": "no/such/file.pt"}, "neither 'pixels' nor"),
                       ({"n": 16, "extractor": "pixels", "kid_subsets": 0}, "kid_subsets must be"),
                       ({"n": 16, "extractor": "pixels", "kid_subset_size": 17}, "kid_subset_size must be"),
                       ({"n": 16, "extractor": "pixels", "kid_subset_size": 1}, "kid_subset_size must be")):
        with pytest.raises(ValueError, match=match):
            _fidelity_cfg(dict(base, eval_fidelity=cfg))
