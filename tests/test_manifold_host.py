"""Precision / recall / density / coverage, host side: the C ABI's entry points and their argument checks (no GPU is touched), the
cpu path of neighbour_radii and ball_membership against a double loop in numpy, manifold_scores on closed cases, every ValueError
and the eval_manifold key of ddpm_run."""
import ctypes

import numpy as np
import pytest
import torch

ENTRY_POINTS = ("afd_kth_neighbour_workspace_bytes", "afd_kth_neighbour_f32", "afd_ball_membership_workspace_bytes", "afd_ball_membership_f32")
INF = float("inf")


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _ints(shape, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg, sz, it = ctypes.c_void_p, ctypes.c_long, ctypes.c_size_t, ctypes.c_int
    want = {"afd_kth_neighbour_workspace_bytes": (sz, [lg, lg, lg]),
            "afd_kth_neighbour_f32": (it, [vp, lg, lg, lg, vp, vp, sz, vp]),
            "afd_ball_membership_workspace_bytes": (sz, [lg, lg, lg]),
            "afd_ball_membership_f32": (it, [vp, lg, vp, lg, lg, vp, vp, vp, vp, vp, vp, sz, vp])}
    for name in ENTRY_POINTS:
        assert name in sigs, name
        assert sigs[name] == want[name], name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))


def test_kth_neighbour_rejects_bad_arguments_before_any_launch():
    from afdm import AfdError, lib
    L = lib()
    n, D, k = 100, 48, 3
    need = L.afd_kth_neighbour_workspace_bytes(n, D, k)
    assert need > 0 and need % 8 == 0
    good = {"X": 1 << 24, "n": n, "D": D, "k": k, "radius2": 2 << 24, "workspace": 3 << 24, "bytes": need}

    def bad(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(AfdError, match="afd_kth_neighbour_f32: .*" + match):
            L.afd_kth_neighbour_f32(a["X"], a["n"], a["D"], a["k"], a["radius2"], a["workspace"], a["bytes"], None)

    for name in ("X", "radius2"):
        bad("X and radius2 must not be NULL", **{name: None})
    bad("workspace must not be NULL", workspace=None)
    for name in ("n", "D"):
        for v in (0, -3):
            bad("n and D must be positive", **{name: v})
    for v in (0, 17, -1):
        bad(r"k must lie in \[1, 16\]", k=v)
    bad(r"n must be below 2\^31", n=1 << 31, bytes=1 << 40)
    bad(r"D at most 2\^15", D=(1 << 15) + 1, bytes=1 << 40)
    bad(r"n D at most 2\^40", n=(1 << 30), D=1 << 11, bytes=1 << 40)
    bad("X must be 4-byte aligned", X=good["X"] + 2)
    for name in ("radius2", "workspace"):
        bad("must be 8-byte aligned", **{name: good[name] + 4})
    bad("workspace too small", bytes=need - 1)
    bad("workspace too small", bytes=0)
    for out in ("radius2", "workspace"):
        bad("must not overlap X", **{out: good["X"] + n * D * 4 - 8})
        bad("must not overlap X", **{out: good["X"]})
    bad("must not overlap each other", workspace=good["radius2"] + 8)
    bad("must not overlap each other", workspace=good["radius2"] - need + 8)


def test_ball_membership_rejects_bad_arguments_before_any_launch():
    from afdm import AfdError, lib
    L = lib()
    nq, nr, D = 70, 90, 17
    need = L.afd_ball_membership_workspace_bytes(nq, nr, D)
    assert need > 0 and need % 8 == 0
    good = {"Q": 1 << 24, "nq": nq, "R": 2 << 24, "nr": nr, "D": D, "radius2": 3 << 24, "exclude": 4 << 24, "count": 5 << 24,
            "nearest": 6 << 24, "nearest_d2": 7 << 24, "workspace": 8 << 24, "bytes": need}

    def bad(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(AfdError, match="afd_ball_membership_f32: .*" + match):
            L.afd_ball_membership_f32(a["Q"], a["nq"], a["R"], a["nr"], a["D"], a["radius2"], a["exclude"], a["count"], a["nearest"],
                                      a["nearest_d2"], a["workspace"], a["bytes"], None)

    for name in ("Q", "R", "radius2"):
        bad("Q, R and radius2 must not be NULL", **{name: None})
    bad("nearest and nearest_d2 go together", nearest=None)
    bad("nearest and nearest_d2 go together", nearest_d2=None)
    bad("nothing to compute", count=None, nearest=None, nearest_d2=None)
    bad("workspace must not be NULL", workspace=None)
    for name in ("nq", "nr", "D"):
        for v in (0, -3):
            bad("nq, nr and D must be positive", **{name: v})
    bad(r"nq and nr must be below 2\^31", nq=1 << 31, bytes=1 << 40)
    bad(r"nq and nr must be below 2\^31", nr=1 << 31, bytes=1 << 40)
    bad(r"D at most 2\^15", D=(1 << 15) + 1, bytes=1 << 40)
    for name in ("Q", "R"):
        bad("Q and R must be 4-byte aligned", **{name: good[name] + 2})
    bad("count must be 4-byte aligned", count=good["count"] + 2)
    for name in ("radius2", "exclude", "nearest", "nearest_d2", "workspace"):
        bad("must be 8-byte aligned", **{name: good[name] + 4})
    bad("workspace too small", bytes=need - 1)
    bad("workspace too small", bytes=0)
    ends = {"Q": nq * D * 4, "R": nr * D * 4, "radius2": nr * 8, "exclude": nq * 8}
    for out in ("count", "nearest", "nearest_d2", "workspace"):
        for name, size in ends.items():
            bad(f"must not overlap {name}", **{out: good[name] + (size - 8) // 8 * 8})
            bad(f"must not overlap {name}", **{out: good[name]})
    bad("must not overlap each other", nearest=good["count"])
    bad("must not overlap each other", nearest_d2=good["nearest"] + nq * 8 - 8)
    bad("must not overlap each other", workspace=good["nearest_d2"] + 8)
    bad("must not overlap each other", workspace=good["count"] - need + 8)


def test_workspace_sizes():
    from afdm import lib
    L = lib()
    kth, ball = L.afd_kth_neighbour_workspace_bytes, L.afd_ball_membership_workspace_bytes
    # the norms, and per segment and row k distances / a distance, an index and a count; the second launch aims at 4096 workgroups:
    # 782 stripes x 6 segments at 50000 rows, never more than 64 segments nor more segments than the store has tiles of 64 rows
    assert kth(1, 1, 1) == 8 + 8 and kth(50000, 2048, 3) == 8 * 50000 + 6 * 50000 * 3 * 8 and kth(100, 7, 16) == 8 * 100 + 2 * 100 * 16 * 8
    assert kth(5000, 4, 3) == 8 * 5000 + 40 * 5000 * 3 * 8
    assert ball(1, 1, 1) == 16 + 16 + 8 and ball(50000, 10000, 2048) == 8 * 60000 + 6 * 50000 * 20 and ball(64, 10 ** 6, 8) == 8 * (64 + 10 ** 6) + 64 * 64 * 20
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 17), (1 << 31, 1, 1), (1, (1 << 15) + 1, 1), (1 << 30, 1 << 11, 1)):
        assert kth(*bad) == 0, bad
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 31, 1, 1), (1, 1 << 31, 1), (1, 1, (1 << 15) + 1), (1, 1 << 30, 1 << 11)):
        assert ball(*bad) == 0, bad


# ---- the cpu path against a double loop --------------------------------------------------------------------------------------------
def _d2_loop(a, b):
    a, b = a.numpy().astype(np.float64), b.numpy().astype(np.float64)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        for j in range(len(b)):
            out[i, j] = sum((a[i, d] - b[j, d]) ** 2 for d in range(a.shape[1]))
    return out


def _radii_loop(x, k):
    d = _d2_loop(x, x)
    out = []
    for i in range(len(d)):
        c = sorted(v for j, v in enumerate(d[i]) if j != i and not np.isnan(v))
        out.append(c[k - 1] if len(c) >= k else INF)
    return np.array(out)


def _membership_loop(q, r, radius2, exclude):
    d = _d2_loop(q, r)
    count, nearest, nearest_d2 = [], [], []
    for i in range(len(d)):
        c, best, bj = 0, INF, -1
        for j in range(d.shape[1]):
            if (exclude is not None and j == exclude[i]) or np.isnan(d[i, j]):
                continue
            c += bool(d[i, j] <= radius2[j])
            if bj < 0 or d[i, j] < best:
                best, bj = d[i, j], j
        count.append(c)
        nearest.append(bj)
        nearest_d2.append(best)
    return np.array(count), np.array(nearest), np.array(nearest_d2)


@pytest.mark.parametrize("n,m,D,k,kind", ((5, 7, 3, 1, "int"), (17, 12, 5, 3, "int"), (40, 33, 6, 5, "randn"), (9, 40, 1, 16, "int"),
                                         (23, 19, 4, 3, "nan")))
def test_the_cpu_path_against_a_double_loop(n, m, D, k, kind):
    import afdm
    make = _randn if kind == "randn" else _ints
    x, q = make((n, D), 1), make((m, D), 2)
    if kind != "randn":
        x[n // 2], q[m // 2] = x[1], x[0]                       # duplicated rows: ties at 0, the lower index wins
    if kind == "nan":
        x[3, 1], q[5, 0] = float("nan"), float("nan")
    radius2 = afdm.neighbour_radii(x, k)
    want = _radii_loop(x, k)
    assert radius2.dtype == torch.float64 and tuple(radius2.shape) == (n,)
    np.testing.assert_allclose(radius2.numpy(), want, rtol=1e-14, atol=0)
    assert (k <= n - 1) or bool(torch.isinf(radius2).all())
    for exclude in (None, torch.arange(m) % n - 1):
        count, nearest, nearest_d2 = afdm.ball_membership(q, x, radius2, exclude)
        wc, wn, wd = _membership_loop(q, x, want, None if exclude is None else exclude.numpy())
        assert count.dtype == torch.int32 and nearest.dtype == torch.long and nearest_d2.dtype == torch.float64
        assert np.array_equal(count.numpy(), wc) and np.array_equal(nearest.numpy(), wn)
        np.testing.assert_allclose(nearest_d2.numpy(), wd, rtol=1e-14, atol=0)
    only = afdm.ball_membership(q, x, radius2, want_nearest=False)
    assert only[1] is None and only[2] is None and torch.equal(only[0], afdm.ball_membership(q, x, radius2)[0])
    assert afdm.ball_membership(q, x, radius2, want_count=False)[0] is None
    # the store against itself, leave-one-out: every row has exactly k neighbours inside ... unless ties extend the ball
    own = afdm.ball_membership(x, x, radius2, torch.arange(n))
    assert not bool((own[1] == torch.arange(n)).any())
    # a NaN radius is in no ball, an infinite one holds every non-NaN distance, and nothing is a candidate when all is excluded
    rad = radius2.clone()
    rad[0], rad[1] = float("nan"), INF
    count = afdm.ball_membership(q, x[:2], rad[:2])[0]
    assert torch.equal(count, (~torch.isnan(q).any(1) & ~torch.isnan(x[1]).any()).to(torch.int32))
    none = afdm.ball_membership(q[:3], x[:1], radius2[:1], torch.zeros(3, dtype=torch.long))
    assert none[0].tolist() == [0, 0, 0] and none[1].tolist() == [-1, -1, -1] and none[2].tolist() == [INF, INF, INF]


def test_the_cpu_path_is_chunked(monkeypatch):
    import sys
    import afdm
    M = sys.modules["afdm.manifold"]
    x, q = _ints((37, 6), 3), _ints((29, 6), 4)
    want_r = afdm.neighbour_radii(x, 3)
    want = afdm.ball_membership(q, x, want_r, torch.arange(29))
    monkeypatch.setattr(M, "_CHUNK", 37 * 6 * 5)                # five rows per block
    assert torch.equal(afdm.neighbour_radii(x, 3), want_r)
    got = afdm.ball_membership(q, x, want_r, torch.arange(29))
    assert all(torch.equal(a, b) for a, b in zip(got, want))


# ---- manifold_scores ---------------------------------------------------------------------------------------------------------------
def test_closed_cases():
    import afdm
    x = _randn((30, 8), 5)
    same = afdm.manifold_scores(x, x.clone(), k=3)
    assert same["precision"] == same["recall"] == same["coverage"] == same["f_score"] == 1.0 and same["density"] >= 1.0
    assert set(same) == {"precision", "recall", "f_score", "density", "coverage"} and all(type(v) is float for v in same.values())
    far = afdm.manifold_scores(x, _randn((25, 8), 6) + 1000.0, k=3)
    assert far == {"precision": 0.0, "recall": 0.0, "f_score": 0.0, "density": 0.0, "coverage": 0.0}
    # every generated row equal to one real row, which 3 of the 20 real rows equal
    real = _randn((20, 8), 7)
    real[4], real[11] = real[0], real[0]
    gen = real[0].repeat(9, 1)
    got = afdm.manifold_scores(gen, real, k=3)
    assert got["precision"] == 1.0 and got["recall"] == 3 / 20 and got["f_score"] == pytest.approx(2 * 0.15 / 1.15, rel=1e-15)
    # ... the three copies' balls have radius 0 at k = 2 and hold every generated row; so does the ball of any row that has a copy
    # among its 2 nearest
    real_r = afdm.neighbour_radii(real, 2)
    assert real_r[0] == real_r[4] == real_r[11] == 0.0
    inside = int((((real.double() - real[0].double()) ** 2).sum(1) <= real_r).sum())
    assert afdm.manifold_scores(gen, real, k=2)["density"] == inside / 2 and inside >= 3
    # coverage counts the real rows whose nearest generated row is inside their own ball: here those whose ball reaches real[0]
    assert afdm.manifold_scores(gen, real, k=2)["coverage"] == inside / 20


def test_scores_against_the_definitions():
    import afdm
    fg, fr, k = _randn((33, 5), 8) * 0.7 + 0.8, _randn((40, 5), 9), 4
    got = afdm.manifold_scores(fg, fr, k=k)
    rg, rr = _radii_loop(fg, k), _radii_loop(fr, k)
    d = _d2_loop(fg, fr)                                      # [generated, real]
    p, r = float((d <= rr[None, :]).any(1).mean()), float((d.T <= rg[None, :]).any(1).mean())
    want = {"precision": p, "recall": r, "f_score": 2 * p * r / (p + r), "density": float((d <= rr[None, :]).sum() / (k * 33)),
            "coverage": float((d.min(0) <= rr).mean())}
    assert got == pytest.approx(want, rel=1e-15) and 0 < p < 1 and 0 < r < 1
    images = torch.randint(0, 256, (12, 1, 3, 3), generator=torch.Generator().manual_seed(10), dtype=torch.uint8)
    ref = torch.randint(0, 256, (15, 1, 3, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    feats = [afdm.extract_features("pixels", t)[0] for t in (images, ref)]
    assert afdm.manifold(images, ref, "pixels", k=2, batch=5) == afdm.manifold_scores(feats[0], feats[1], k=2)


def test_value_errors():
    import afdm
    x, y = _randn((10, 4), 12), _randn((8, 4), 13)
    r = afdm.neighbour_radii(x, 2)
    for bad in (x.double(), x[0], x[:, :0], "features"):
        with pytest.raises(ValueError, match="neighbour_radii: features must be"):
            afdm.neighbour_radii(bad, 2)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match=r"neighbour_radii: k must be an int in \[1, 16\]"):
            afdm.neighbour_radii(x, bad)
        with pytest.raises(ValueError, match=r"manifold_scores: k must be an int in \[1, 16\]"):
            afdm.manifold_scores(x, y, bad)
    with pytest.raises(ValueError, match="ball_membership: queries must be"):
        afdm.ball_membership(y.double(), x, r)
    with pytest.raises(ValueError, match=r"ball_membership: store must be a non-empty \(n, 4\) float32"):
        afdm.ball_membership(y, _randn((10, 5), 1), r)
    for bad in (r.float(), r[:-1], r.view(1, -1)):
        with pytest.raises(ValueError, match="ball_membership: radius2 must be"):
            afdm.ball_membership(y, x, bad)
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(7, dtype=torch.long)):
        with pytest.raises(ValueError, match="ball_membership: exclude must be"):
            afdm.ball_membership(y, x, r, bad)
    with pytest.raises(ValueError, match="ball_membership: nothing to compute"):
        afdm.ball_membership(y, x, r, want_count=False, want_nearest=False)
    with pytest.raises(ValueError, match="manifold_scores: fr must be"):
        afdm.manifold_scores(x, _randn((8, 5), 1))
    for k in (8, 9, 16):
        with pytest.raises(ValueError, match=f"manifold_scores: k = {k} must be below the size of the smaller feature set"):
            afdm.manifold_scores(x, y, k)
    assert afdm.manifold_scores(x, y, 7)["f_score"] >= 0.0


def test_public_names():
    import afdm
    for name in ("neighbour_radii", "ball_membership", "manifold_scores", "manifold", "manifold_results"):
        assert callable(getattr(afdm, name)), name
    assert callable(afdm.ops.kth_neighbour) and callable(afdm.ops.ball_membership)
    doc = afdm.manifold_scores.__globals__["__doc__"]
    assert "torch_fidelity" in doc and "no parity is claimed" in doc


# ---- ddpm_run ------------------------------------------------------------------------------------------------------------------------
def test_eval_manifold_key_check():
    from afdm.tasks import _manifold_cfg
    base = {"gen_total": 16}
    assert _manifold_cfg(dict(base, eval_manifold={"n": 16, "extractor": "pixels"})) == {"n": 16, "extractor": "pixels", "k": 3}
    fn = lambda x: x.float().flatten(1)      # noqa: E731
    got = _manifold_cfg(dict(base, eval_manifold={"n": np.int64(6), "extractor": fn, "k": np.int64(5)}))
    assert got == {"n": 6, "extractor": fn, "k": 5} and type(got["n"]) is int and type(got["k"]) is int
    for cfg, match in ((16, "needs n and extractor"), ({"n": 16}, "needs n and extractor"), ({"extractor": "pixels"}, "needs n and extractor"),
                       ({"n": 16, "extractor": "pixels", "kid_subsets": 3}, "needs n and extractor"),
                       ({"n": 17, "extractor": "pixels"}, "n must be an int in"), ({"n": 3, "extractor": "pixels"}, "n must be an int in"),
                       ({"n": 5, "extractor": "pixels", "k": 5}, "n must be an int in"),
                       ({"n": True, "extractor": "pixels"}, "n must be an int in"), ({"n": 8.0, "extractor": "pixels"}, "n must be an int in"),
                       ({"n": 16, "extractor": "pixels", "k": 0}, "k must be an int in"),
                       ({"n": 16, "extractor": "pixels", "k": 17}, "k must be an int in"),
                       ({"n": 16, "extractor": "pixels", "k": 2.0}, "k must be an int in"),
                       ({"n": 16, "extractor": 3}, "extractor must be"), ({"n": 16, "extractor": "no/such/file.pt"}, "neither 'pixels' nor")):
        with pytest.raises(ValueError, match="eval_manifold.*" + match):
            _manifold_cfg(dict(base, eval_manifold=cfg))
    assert _manifold_cfg(dict(base, eval_manifold={"n": 4, "extractor": "pixels"}))["n"] == 4        # k + 1 is the smallest n
