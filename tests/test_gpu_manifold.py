"""Precision / recall / density / coverage on the GPU: afd_kth_neighbour_f32 and afd_ball_membership_f32 through the C ABI and
through ops, against the cpu path of manifold.py (plain torch fp64 in the difference form), manifold_scores on device tensors, and
ddpm_run with params["eval_manifold"].

Integer-valued features (|x| <= 8) make every distance an exact integer in either arithmetic form, with ties in plenty, so those
results are compared BIT FOR BIT.  Random features are held to the distance contract's bound, which is twice the forward bound of
three length-D fp64 chains of exact products,
    |d2 - exact| <= 2 (D + 4) 2^-52 (|a|^2 + |b|^2),
computed here from the data; a k-th smallest or a smallest distance moves by at most the largest bound among its candidates.
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
CANARY = -7777.0
INF = float("inf")


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _oracle():
    import afdm  # noqa: F401
    return sys.modules["afdm.manifold"]


def _ints(shape, seed, lo=-8, hi=8):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    """Equal bit for bit (so that +inf equals +inf and nothing else does)."""
    a, b = a.cpu(), b.cpu()
    return a.dtype == b.dtype and a.shape == b.shape and (torch.equal(_bits(a), _bits(b)) if a.dtype == torch.float64 else torch.equal(a, b))


def _kth_abi(afdm, X, k, fill=0xFF):
    """The C ABI with raw pointers: radius2 sits inside a longer buffer whose other elements must come back untouched, and the
    workspace is pre-filled with the byte `fill`."""
    L = afdm.lib()
    n, D = X.shape
    need = L.afd_kth_neighbour_workspace_bytes(n, D, k)
    assert 0 < need <= 64 << 20 and need % 8 == 0
    ws = torch.full((need + 64,), fill, device=X.device, dtype=torch.uint8)
    r = torch.full((n + 16,), CANARY, device=X.device, dtype=torch.float64)
    L.afd_kth_neighbour_f32(X.data_ptr(), n, D, k, r.data_ptr(), ws.data_ptr(), need, afdm.ops._stream())
    assert bool((ws[need:] == fill).all()) and bool((r[n:] == CANARY).all())
    return r[:n].clone()


def _ball_abi(afdm, Q, R, radius2, exclude=None, count=True, near=True, fill=0xFF):
    L = afdm.lib()
    (nq, D), nr = Q.shape, R.shape[0]
    need = L.afd_ball_membership_workspace_bytes(nq, nr, D)
    assert 0 < need <= 64 << 20 and need % 8 == 0
    dev = Q.device
    ws = torch.full((need + 64,), fill, device=dev, dtype=torch.uint8)
    c = torch.full((nq + 16,), -77, device=dev, dtype=torch.int32)
    j = torch.full((nq + 16,), -77, device=dev, dtype=torch.int64)
    d = torch.full((nq + 16,), CANARY, device=dev, dtype=torch.float64)
    L.afd_ball_membership_f32(Q.data_ptr(), nq, R.data_ptr(), nr, D, radius2.data_ptr(), None if exclude is None else exclude.data_ptr(),
                              c.data_ptr() if count else None, j.data_ptr() if near else None, d.data_ptr() if near else None, ws.data_ptr(), need,
                              afdm.ops._stream())
    assert bool((ws[need:] == fill).all())
    assert bool((c[nq if count else 0:] == -77).all()) and bool((j[nq if near else 0:] == -77).all()) and bool((d[nq if near else 0:] == CANARY).all())
    return c[:nq].clone(), j[:nq].clone(), d[:nq].clone()


# ---- 1. integer-valued features: bit for bit ---------------------------------------------------------------------------------------
INT_CASES = ((2, 1, 1, "plain"), (2, 3, 3, "plain"), (17, 5, 16, "dup"), (17, 257, 1, "plain"), (63, 64, 3, "dup"), (64, 67, 1, "nan"),
             (64, 3, 16, "view"), (65, 257, 3, "dup"), (65, 1, 16, "plain"), (130, 3, 16, "nan"), (130, 64, 3, "view"), (130, 5, 1, "dup"))


@pytest.mark.parametrize("n,D,k,kind", INT_CASES)
def test_integer_features_bit_for_bit(A, n, D, k, kind):
    afdm, dev = A
    m = n + 7
    x, q = _ints((n, D), 100 + n + D), _ints((m, D), 200 + n + D)
    if kind == "dup":                                           # duplicated rows: distance 0 at another index, ties everywhere
        x[n - 1], x[n // 2], q[3], q[m - 1] = x[0], x[1], x[n // 2], x[n - 1]
    if kind == "nan":
        x[5, D // 2], q[2, 0] = float("nan"), float("nan")
    want_r = afdm.neighbour_radii(x, k)
    ex = (torch.arange(m) * 5) % (n + 1) - 1                    # every store row and -1 (nothing)
    want = {None: afdm.ball_membership(q, x, want_r), "ex": afdm.ball_membership(q, x, want_r, ex)}
    if kind == "view":                                          # one float past an allocation: 4-byte aligned and no more
        xd = torch.cat([torch.zeros(1), x.flatten()]).to(dev)[1:].view(n, D)
        qd = torch.cat([torch.zeros(1), q.flatten()]).to(dev)[1:].view(m, D)
        assert xd.data_ptr() % 8 == 4 and qd.data_ptr() % 8 == 4 and xd.is_contiguous()
    else:
        xd, qd = x.to(dev), q.to(dev)
    got_r = _kth_abi(afdm, xd, k)
    assert _same(got_r, want_r), (got_r.cpu(), want_r)
    assert _same(afdm.ops.kth_neighbour(xd, k), want_r) and _same(afdm.neighbour_radii(xd, k), want_r)
    if k > n - 1:
        assert bool(torch.isinf(got_r).all())
    for key, e in ((None, None), ("ex", ex.to(dev))):
        got = _ball_abi(afdm, qd, xd, got_r, e)
        for name, g, w in zip(("count", "nearest", "nearest_d2"), got, want[key]):
            assert _same(g, w), (name, key, g.cpu(), w)
        assert all(_same(g, w) for g, w in zip(afdm.ops.ball_membership(qd, xd, got_r, e), want[key]))
    only_c = _ball_abi(afdm, qd, xd, got_r, None, near=False)
    only_n = _ball_abi(afdm, qd, xd, got_r, None, count=False)
    assert _same(only_c[0], want[None][0]) and _same(only_n[1], want[None][1]) and _same(only_n[2], want[None][2])
    # a NaN radius is in no ball, an infinite one holds every non-NaN distance; with everything excluded there is no candidate
    rad = got_r.clone()
    rad[0], rad[1] = float("nan"), INF
    assert all(_same(g, w) for g, w in zip(afdm.ops.ball_membership(qd, xd, rad), afdm.ball_membership(q, x, rad.cpu())))
    none = afdm.ops.ball_membership(qd[:3], xd[:1], got_r[:1], torch.zeros(3, dtype=torch.long, device=dev))
    assert none[0].tolist() == [0, 0, 0] and none[1].tolist() == [-1, -1, -1] and none[2].tolist() == [INF, INF, INF]


def test_a_store_that_spans_many_workgroups(A):
    afdm, dev = A
    x, q = _ints((5000, 4), 31), _ints((333, 4), 32)
    want_r = afdm.neighbour_radii(x, 3)
    got_r = afdm.ops.kth_neighbour(x.to(dev), 3)
    assert _same(got_r, want_r)
    ex = torch.arange(333) * 15
    want = afdm.ball_membership(q, x, want_r, ex)
    got = afdm.ops.ball_membership(q.to(dev), x.to(dev), got_r, ex.to(dev))
    assert all(_same(g, w) for g, w in zip(got, want))
    # ... and the long side as the queries
    rq = afdm.neighbour_radii(q, 5)
    assert all(_same(g, w) for g, w in zip(afdm.ops.ball_membership(x.to(dev), q.to(dev), rq.to(dev)), afdm.ball_membership(x, q, rq)))


# ---- 2. random features: the bound ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,seed", ((64, 41), (300, 42)))
def test_random_features_within_the_bound(A, D, seed):
    """radius2 and nearest_d2 within the bound; count and nearest equal wherever no pair lies within the bound of its threshold
    (such rows are counted, and may not be more than 1 % of the rows; for these seeds the cpu path shows none)."""
    afdm, dev = A
    M = _oracle()
    n, m, k = 200, 150, 3
    x, q = _randn((n, D), seed) * 1.5 + 0.25, _randn((m, D), seed + 100) * 1.4 + 0.25
    unit = 2 * (D + 4) * 2.0 ** -52
    sx, sq = (x.double() ** 2).sum(1), (q.double() ** 2).sum(1)
    want_r = afdm.neighbour_radii(x, k)
    got_r = afdm.ops.kth_neighbour(x.to(dev), k)
    bound_r = unit * (sx + sx.max())
    err = ((got_r.cpu() - want_r).abs() / bound_r).max().item()
    print(f"D={D}: radius2 worst error {err:.3f} of the bound")
    note("manifold radius2 / bound (gate 1)", err, f"n={n} D={D}")
    assert err <= 1.0
    want = afdm.ball_membership(q, x, want_r)
    got = [t.cpu() for t in afdm.ops.ball_membership(q.to(dev), x.to(dev), want_r.to(dev))]
    d = torch.cat([blk for _, blk in M._d2_blocks(q, x)])       # the oracle's distances [query, store row]
    pair = unit * (sq.unsqueeze(1) + sx.unsqueeze(0))
    close_count = ((d - want_r.unsqueeze(0)).abs() <= pair).any(1)           # a distance within its bound of the radius it is held against
    two = d.topk(2, dim=1, largest=False).values
    close_near = (two[:, 1] - two[:, 0]) <= 2 * unit * (sq + sx.max())
    touched = int((close_count | close_near).sum())
    print(f"D={D}: {int(close_count.sum())} rows with a distance on a threshold, {int(close_near.sum())} with two nearest rows within the bound")
    assert touched <= 0.01 * m
    assert torch.equal(got[0][~close_count], want[0][~close_count]) and torch.equal(got[1][~close_near], want[1][~close_near])
    err = ((got[2] - want[2]).abs() / (unit * (sq + sx.max()))).max().item()
    print(f"D={D}: nearest_d2 worst error {err:.3f} of the bound")
    note("manifold nearest_d2 / bound (gate 1)", err, f"nq={m} nr={n} D={D}")
    assert err <= 1.0


# ---- 3. the distance contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,D,k", ((150, 64, 3), (131, 37, 5), (70, 300, 16)))
def test_the_distance_contract(A, n, D, k):
    afdm, dev = A
    x = (_randn((n, D), 50 + D) * 2).to(dev)
    own = torch.arange(n, device=dev)
    radius2 = afdm.ops.kth_neighbour(x, k)
    assert bool(torch.isfinite(radius2).all()) and bool((radius2 > 0).all())
    # every row's k-th neighbour sits ON its ball's boundary: the counts sum to k n only if the k-th smallest of row j's distances
    # and the distance from the other side have the same bits (tie-free: the k-th and the (k + 1)-th distances differ)
    assert not bool((afdm.ops.kth_neighbour(x, k + 1) == radius2).any()) if k < 16 else True
    count, nearest, nearest_d2 = afdm.ops.ball_membership(x, x, radius2, own)
    assert int(count.sum()) == k * n, (int(count.sum()), k * n)
    assert _same(nearest_d2, afdm.ops.kth_neighbour(x, 1))      # the nearest other row, from either entry point
    # d2 of a row with itself is 0, and nothing is below it
    zero = torch.zeros(n, dtype=torch.float64, device=dev)
    c0, j0, d0 = afdm.ops.ball_membership(x, x, zero)
    assert bool((d0 == 0).all()) and torch.equal(j0, own) and bool((c0 == 1).all())
    # symmetric bit for bit, whichever side is the query and wherever the rows sit: d2(q, r) for single rows, both ways round
    for a, b in ((0, n - 1), (5, 64 % n), (n // 2, 1)):
        ab = afdm.ops.ball_membership(x[a:a + 1], x[b:b + 1], zero[:1])[2]
        ba = afdm.ops.ball_membership(x[b:b + 1], x[a:a + 1], zero[:1])[2]
        inside = afdm.ops.ball_membership(x[a:a + 1], x, zero, torch.full((1,), -1, device=dev), want_count=False)
        assert _same(ab, ba) and bool(ab > 0)
        full = afdm.ops.ball_membership(x, x[b:b + 1], zero[:1], want_count=False)[2]
        assert _same(full[a:a + 1], ab) and int(inside[1]) == a
    # permuting the store permutes radius2 bit for bit and leaves the counts unchanged
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(dev)
    assert _same(afdm.ops.kth_neighbour(x[perm].contiguous(), k), radius2[perm])
    q = _randn((90, D), 60 + D).to(dev) * 2
    base = afdm.ops.ball_membership(q, x, radius2)
    moved = afdm.ops.ball_membership(q, x[perm].contiguous(), radius2[perm].contiguous())
    assert _same(moved[0], base[0]) and _same(moved[2], base[2]) and torch.equal(perm[moved[1]], base[1])


def test_integer_rows_with_large_sums_are_exact(A):
    """Rows of integers up to 2^11 at D = 257: sums near 2^31, far below 2^53."""
    afdm, dev = A
    x, q = _ints((70, 257), 71, -2048, 2048), _ints((66, 257), 72, -2048, 2048)
    want_r = afdm.neighbour_radii(x, 2)
    got_r = afdm.ops.kth_neighbour(x.to(dev), 2)
    assert _same(got_r, want_r) and float(want_r.max()) > 2.0 ** 29
    assert all(_same(g, w) for g, w in zip(afdm.ops.ball_membership(q.to(dev), x.to(dev), got_r), afdm.ball_membership(q, x, want_r)))


# ---- 4. repeatability and graph capture --------------------------------------------------------------------------------------------
def test_two_calls_and_a_captured_graph_give_the_same_bits(A):
    afdm, dev = A
    L = afdm.lib()
    n, m, D, k = 300, 170, 70, 3
    x, q = _randn((n, D), 81).to(dev), _randn((m, D), 82).to(dev)
    first = _kth_abi(afdm, x, k, fill=0x00)
    assert _same(first, _kth_abi(afdm, x, k, fill=0xFF))        # (whatever the workspace held)
    b1, b2 = _ball_abi(afdm, q, x, first, fill=0x00), _ball_abi(afdm, q, x, first, fill=0xFF)
    assert all(_same(a, b) for a, b in zip(b1, b2))
    need_k, need_b = L.afd_kth_neighbour_workspace_bytes(n, D, k), L.afd_ball_membership_workspace_bytes(m, n, D)
    ws = torch.empty(max(need_k, need_b) // 8, device=dev, dtype=torch.float64)
    r = torch.zeros(n, device=dev, dtype=torch.float64)
    c = torch.zeros(m, device=dev, dtype=torch.int32)
    j = torch.zeros(m, device=dev, dtype=torch.int64)
    d = torch.zeros(m, device=dev, dtype=torch.float64)

    def both():
        L.afd_kth_neighbour_f32(x.data_ptr(), n, D, k, r.data_ptr(), ws.data_ptr(), need_k, afdm.ops._stream())
        L.afd_ball_membership_f32(q.data_ptr(), m, x.data_ptr(), n, D, r.data_ptr(), None, c.data_ptr(), j.data_ptr(), d.data_ptr(), ws.data_ptr(),
                                  need_b, afdm.ops._stream())

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for buf in (r, d):
        buf.fill_(CANARY)
    c.fill_(-1)
    j.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert _same(r, first) and _same(c, b1[0]) and _same(j, b1[1]) and _same(d, b1[2])
    x.copy_(_randn((n, D), 83))                                 # new contents, the same graph
    g.replay()
    torch.cuda.synchronize()
    again = _kth_abi(afdm, x, k)
    assert _same(r, again) and not _same(r, first) and all(_same(a, b) for a, b in zip((c, j, d), _ball_abi(afdm, q, x, again)))


def test_ops_argument_checks(A):
    afdm, dev = A
    x, q = _randn((20, 6), 91).to(dev), _randn((9, 6), 92).to(dev)
    r = afdm.ops.kth_neighbour(x, 2)
    for bad in (x.cpu(), x.double(), x[0], x[:, :0]):
        with pytest.raises(afdm.AfdError, match="kth_neighbour: features must be"):
            afdm.ops.kth_neighbour(bad, 2)
    for bad in (0, 17, True, 2.0):
        with pytest.raises(afdm.AfdError, match=r"kth_neighbour: k must be an int in \[1, 16\]"):
            afdm.ops.kth_neighbour(x, bad)
    with pytest.raises(afdm.AfdError, match="ball_membership: store must have the row size 6"):
        afdm.ops.ball_membership(q, x[:, :5], r)
    for bad in (r.float(), r[:-1], r.cpu()):
        with pytest.raises(afdm.AfdError, match="ball_membership: radius2 must be"):
            afdm.ops.ball_membership(q, x, bad)
    with pytest.raises(afdm.AfdError, match="ball_membership: exclude must be"):
        afdm.ops.ball_membership(q, x, r, torch.zeros(9, dtype=torch.int32, device=dev))
    with pytest.raises(afdm.AfdError, match="ball_membership: nothing to compute"):
        afdm.ops.ball_membership(q, x, r, want_count=False, want_nearest=False)
    # a view that is not contiguous is made so
    wide = _randn((20, 12), 93).to(dev)
    assert _same(afdm.ops.kth_neighbour(wide[:, ::2], 2), afdm.ops.kth_neighbour(wide[:, ::2].contiguous(), 2))


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
def test_manifold_scores_on_the_device_equal_the_cpu_path(A):
    afdm, dev = A
    fg, fr = _ints((150, 20), 95, -3, 3), _ints((170, 20), 96, -3, 3) + (torch.arange(20) % 3 == 0).float()
    for k in (3, 5):
        want = afdm.manifold_scores(fg, fr, k=k)
        got = afdm.manifold_scores(fg.to(dev), fr.to(dev), k=k)
        assert got == want, (got, want)
        assert 0 < want["precision"] < 1 and 0 < want["recall"] < 1 and 0 < want["coverage"] < 1 and want["density"] > 0
        assert afdm.manifold_scores(fg.to(dev), fr, k=k) == want            # both sets go to fg's device
    gen = torch.randint(0, 256, (40, 3, 4, 4), generator=torch.Generator().manual_seed(97), dtype=torch.uint8)
    ref = torch.randint(0, 256, (50, 3, 4, 4), generator=torch.Generator().manual_seed(98), dtype=torch.uint8)
    got, want = afdm.manifold(gen.to(dev), ref.to(dev), "pixels", k=3), afdm.manifold(gen, ref, "pixels", k=3)
    # pixels / 127.5 - 1 are not integers: the two arithmetic forms may differ in the last bits, so a row may change sides only where a
    # distance sits on a threshold; these sets have none (the scores are multiples of 1 / 40 and 1 / 50)
    assert got == pytest.approx(want, abs=1e-12)


def test_ddpm_run_with_eval_manifold(A, tmp_path, monkeypatch):
    from PIL import Image
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    cfg = {"n": 16, "extractor": "pixels", "k": 2}
    runs = {}
    for key in ("plain", "manifold"):
        wd = tmp_path / key
        wd.mkdir()
        np.savetxt(wd / "mnist.csv", arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 8, "gen_total": 16, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "manifold":
            params["eval_manifold"] = dict(cfg)
        out = afdm.ddpm_run(params)
        run_dir = os.path.join("runs", "DDPM_Uncondtional_MNIST_3")
        runs[key] = (out, open(os.path.join(run_dir, "settings_MNIST_3.txt")).read().replace(str(wd), ""), str(wd / run_dir))
    (po, pt, pdir), (fo, ft, fdir) = runs["plain"], runs["manifold"]
    assert "manifold" not in po and pt == ft and po["loss_all"] == fo["loss_all"]
    assert not [f for f in os.listdir(pdir) if f.startswith("manifold")]
    assert sorted(os.listdir(fdir)) == sorted(os.listdir(pdir) + ["manifold_MNIST_3.json"])

    def saved(out):
        return torch.stack([torch.from_numpy(np.array(Image.open(os.path.join(out["gen_dir"], f"image_{i}.png")))) for i in range(16)])
    images = saved(fo)
    assert torch.equal(images, saved(po))                   # the same generated images with and without the key
    res = fo["manifold"]
    keys = {"precision", "recall", "f_score", "density", "coverage"}
    assert set(res) == keys and all(isinstance(v, float) and math.isfinite(v) for v in res.values())
    with open(os.path.join(fdir, "manifold_MNIST_3.json")) as fh:
        written = json.load(fh)
    assert {k: written[k] for k in keys} == res and written["n"] == 16 and written["k"] == 2 and set(written) == keys | {"n", "k"}
    # the saved samples against the training tensors, on the cpu: the scores are multiples of 1 / 16 and 1 / 32
    monkeypatch.chdir(tmp_path / "manifold")
    train = afdm.get_data_MNIST(afdm.argument(dataset_path="mnist.csv", batch_size=8))[1].tensors[0]
    pixels = afdm.DeviceDataset(train[:16], device="cpu").pixels()
    want = afdm.manifold(images.view(16, 1, 32, 32), pixels, "pixels", k=2)
    assert res == pytest.approx(want, abs=1e-12), (res, want)
    with pytest.raises(ValueError, match="eval_manifold n must be an int in"):
        afdm.ddpm_run(dict(params, eval_manifold=dict(cfg, n=17)))      # more than gen_total: fails before any training
    data = {"args": afdm.argument(image_size=32, image_channels=1, device="cuda", noise_steps=6), "unet_v": 3, "seed": 42,
            "f_settings": {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2},
            "modelpath": fo["modelpath"]}
    r = afdm.manifold_results(data, train, 16, "pixels", k=2)
    assert set(r) == keys and all(math.isfinite(v) for v in r.values())
    with pytest.raises(ValueError, match="manifold_results: n must be an int in"):
        afdm.manifold_results(data, train, 17, "pixels")
