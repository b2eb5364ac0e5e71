"""Nearest-training-image search on the GPU: afd_nn_search_u8 / afd_nn_search_f32 through the C ABI and through
DeviceDataset.nearest / self_nearest, against the pure-torch brute force (DeviceDataset on device="cpu", pinned to a numpy brute
force by tests/test_nearest_host.py), and ddpm_run with params["eval_nearest"].  The u8 search and the f32 search on exactly
representable data are compared with torch.equal, no tolerance; f32 on randn data within one fp32 ulp (the two fp64 sums differ
by at most (D + 2) 2^-53 relative, so their roundings to fp32 differ by at most one ulp)."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1, 1), (1, 5, 7), (1, 8, 8), (3, 8, 8), (1, 8, 125), (3, 32, 32))      # D = 1, 35, 64, 192, 1000, 3072
STORES = (1, 63, 257, 1000)
QUERIES = (1, 17, 70)
KS = (1, 5, 16)
CANARY = -7777
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _u8(shape, seed, values=None):
    g = torch.Generator().manual_seed(seed)
    if values is None:
        return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    return torch.tensor(values, dtype=torch.uint8)[torch.randint(0, len(values), shape, generator=g)]


def _grid(shape, seed):
    """fp32 values j / 128, j an integer in [-128, 128]: every difference, square and fp64 sum is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-128, 129, shape, generator=g).float() / 128


def _oracle(afdm, data, queries, k, exclude=None):
    return afdm.DeviceDataset(data, device="cpu").nearest(queries, k, exclude)


def _same(got, want):
    """(dist, idx) pairs are equal: idx as integers, dist as integers or as fp32 bits."""
    (gd, gi), (wd, wi) = got, want
    if wd.dtype == torch.float32:
        gd, wd = gd.cpu().view(torch.int32), wd.view(torch.int32)
    return torch.equal(gi.cpu(), wi) and torch.equal(gd.cpu(), wd) and gd.dtype == wd.dtype


def _abi(afdm, data, queries, k, exclude=None, fill=0xFF):
    """The C ABI with raw pointers: data (N, ...) and queries (n, ...) device tensors (views allowed).  Outputs sit inside longer
    buffers whose other elements must come back untouched; the workspace is pre-filled with `fill`."""
    L = afdm.lib()
    N, n = data.shape[0], queries.shape[0]
    D = data[0].numel()
    f32 = data.dtype == torch.float32
    need = L.afd_nn_search_workspace_bytes(N, D, n, k, int(f32))
    assert 0 < need <= 64 << 20
    ws = torch.full((need,), fill, device=data.device, dtype=torch.uint8)
    idx = torch.full((n * k + 64,), CANARY, device=data.device, dtype=torch.long)
    dist = torch.full((n * k + 64,), CANARY, device=data.device, dtype=torch.float32 if f32 else torch.long)
    fn = L.afd_nn_search_f32 if f32 else L.afd_nn_search_u8
    fn(data.data_ptr(), N, D, queries.data_ptr(), n, None if exclude is None else exclude.data_ptr(), k, idx.data_ptr(), dist.data_ptr(),
       ws.data_ptr(), need, afdm.ops._stream())
    assert bool((idx[n * k:] == CANARY).all()) and bool((dist[n * k:] == CANARY).all())
    return dist[:n * k].view(n, k), idx[:n * k].view(n, k)


def _offset_view(t, dev, skip_bytes=1):
    """A contiguous copy of t on the device that starts skip_bytes into its allocation."""
    flat = t.contiguous().view(-1).view(torch.uint8)
    buf = torch.empty(flat.numel() + 64, device=dev, dtype=torch.uint8)
    view = buf[skip_bytes:skip_bytes + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == skip_bytes
    return view.view(t.shape) if t.dtype == torch.uint8 else view


# ---- 1. u8: exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", SHAPES)
def test_u8_random_bytes_against_the_oracle(A, chw):
    """Every N, n and k of the grid (k > N included) through the C ABI, with the workspace pre-filled with 0xFF and with 0x00, and
    through DeviceDataset.nearest.  The oracle runs once per (N, n) at k = 16: the order is total, so the answer at a smaller k is
    its first k columns."""
    afdm, dev = A
    for N in STORES:
        data = _u8((N,) + chw, 1000 + N)
        ds = afdm.DeviceDataset(data, device=dev)
        for n in QUERIES:
            queries = _u8((n,) + chw, 2000 + n)
            want_d, want_i = _oracle(afdm, data, queries, 16)
            qd = queries.to(dev)
            for k in KS:
                want = (want_d[:, :k], want_i[:, :k])
                for fill in (0xFF, 0x00):
                    assert _same(_abi(afdm, ds.images, qd, k, fill=fill), want), (N, n, k, fill)
                got = ds.nearest(queries, k)
                assert got[0].is_cuda and tuple(got[0].shape) == (n, k) and _same(got, want), (N, n, k)
                if N < k:
                    assert bool((got[1][:, N:] == -1).all()) and bool((got[0][:, N:] == -1).all())


@pytest.mark.parametrize("chw,N,n", (((3, 32, 32), 257, 17), ((2, 128, 128), 3, 3)))
def test_u8_sign_boundary_and_the_largest_distance(A, chw, N, n):
    """Bytes 0, 127, 128, 255 only: both sides of the XOR's sign boundary, and D 255^2 between an all-0 and an all-255 row, at
    D = 3072 and at the cap D = 32768."""
    afdm, dev = A
    D = chw[0] * chw[1] * chw[2]
    data, queries = _u8((N,) + chw, 5, (0, 127, 128, 255)), _u8((n,) + chw, 6, (0, 127, 128, 255))
    data[0], data[N - 1], queries[0], queries[n - 1] = 0, 255, 255, 0
    ds = afdm.DeviceDataset(data, device=dev)
    for k in (1, 5):
        want = _oracle(afdm, data, queries, k)
        assert _same(ds.nearest(queries, k), want) and _same(_abi(afdm, ds.images, queries.to(dev), k), want)
    far = _oracle(afdm, data[:1], queries[:1], 1)
    assert far[0].item() == D * 255 ** 2 and _same(_abi(afdm, ds.images[:1], queries[:1].to(dev), 1), far)


def test_u8_duplicates_exclude_and_misaligned_views(A):
    afdm, dev = A
    chw, N, n = (3, 8, 8), 257, 17
    data, queries = _u8((N,) + chw, 7), _u8((n,) + chw, 8)
    data[100] = data[40]
    data[200] = data[40]
    data[256] = data[3]
    queries[0], queries[5], queries[16] = data[40], data[3], data[255]
    ds = afdm.DeviceDataset(data, device=dev)
    for k in (1, 5, 16):
        want = _oracle(afdm, data, queries, k)
        assert want[0][0, 0] == 0 and want[1][0, 0] == 40 and want[1][5, 0] == 3 and (k == 1 or want[1][0, :3].tolist() == [40, 100, 200])
        assert _same(ds.nearest(queries, k), want)
        ex = torch.full((n,), -1, dtype=torch.long)
        ex[0], ex[5], ex[16], ex[7] = 40, 256, 255, 0
        want_ex = _oracle(afdm, data, queries, k, ex)
        assert want_ex[1][0, 0] == 100 and not (want_ex[1] == ex.view(-1, 1)).any()
        assert _same(ds.nearest(queries, k, ex), want_ex) and _same(_abi(afdm, ds.images, queries.to(dev), k, ex.to(dev)), want_ex)
        neg = torch.tensor([-1, -2, -2 ** 63] * 6)[:n]
        assert _same(ds.nearest(queries, k, neg), want) and _same(_abi(afdm, ds.images, queries.to(dev), k, neg.to(dev)), want)
        # data and queries one byte into their buffers: byte loads, the same result
        dv, qv = _offset_view(data, dev), _offset_view(queries, dev)
        assert _same(_abi(afdm, dv, qv, k), want) and _same(_abi(afdm, dv, queries.to(dev), k), want)
        assert _same(_abi(afdm, ds.images, qv, k, ex.to(dev)), want_ex)
    # k exceeds what exclude leaves
    got = ds.nearest(data[:2], 2, torch.tensor([0, 1]))
    one = afdm.DeviceDataset(data[:1], device=dev)
    assert _same(one.nearest(data[:2], 2, torch.tensor([0, 1])), _oracle(afdm, data[:1], data[:2], 2, torch.tensor([0, 1])))
    assert one.nearest(data[:2], 2, torch.tensor([0, 1]))[1].tolist() == [[-1, -1], [0, -1]] and bool((got[1] >= 0).all())


@pytest.mark.parametrize("kind", ("u8", "f32"))
@pytest.mark.parametrize("chw,N,n", (((3, 8, 8), 257, 300), ((1, 4, 4), 16640, 389)))
def test_more_queries_than_one_tile(A, kind, chw, N, n):
    """A store of few chunks splits its query tiles over the grid's second axis: one tile per workgroup at N = 257, several
    at N = 16640 (130 chunks of 128 rows for u8, 65 of 256 for f32).  The oracle runs at k = 5; k = 1 is its first column."""
    afdm, dev = A
    data, queries = (_u8((N,) + chw, 51), _u8((n,) + chw, 52)) if kind == "u8" else (_grid((N,) + chw, 51), _grid((n,) + chw, 52))
    queries[n - 1] = data[N - 1]
    ex = torch.full((n,), -1, dtype=torch.long)
    ex[n - 1] = N - 1
    ds = afdm.DeviceDataset(data, device=dev)
    want, want_ex = _oracle(afdm, data, queries, 5), _oracle(afdm, data, queries, 5, ex)
    assert want[1][n - 1, 0] == N - 1 and want_ex[1][n - 1, 0] != N - 1
    for k in (1, 5):
        assert _same(ds.nearest(queries, k), (want[0][:, :k], want[1][:, :k]))
        assert _same(_abi(afdm, ds.images, queries.to(dev), k, ex.to(dev)), (want_ex[0][:, :k], want_ex[1][:, :k]))


# ---- 2. partition independence ------------------------------------------------------------------------------------------------------
def test_the_result_depends_on_no_partition(A):
    afdm, dev = A
    chw, N, n, k = (3, 32, 32), 1000, 70, 8
    data, queries = _u8((N,) + chw, 11), _u8((n,) + chw, 12)
    ds = afdm.DeviceDataset(data, device=dev)
    whole = ds.nearest(queries, k)
    parts = [ds.nearest(queries[:1], k), ds.nearest(queries[1:], k)]
    assert torch.equal(torch.cat([p[0] for p in parts]), whole[0]) and torch.equal(torch.cat([p[1] for p in parts]), whole[1])
    want = _oracle(afdm, data, queries, k + 1)
    assert bool((want[0][:, 1:] > want[0][:, :-1]).all())        # no tie among the k + 1 nearest: the k nearest are one set, one order
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(13))
    moved = afdm.DeviceDataset(data[perm], device=dev).nearest(queries, k)
    assert torch.equal(moved[0], whole[0]) and torch.equal(perm.to(dev)[moved[1]], whole[1])
    assert _same(whole, (want[0][:, :k], want[1][:, :k]))


# ---- 3. f32 on exactly representable data --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", ((1, 1, 1), (1, 5, 7), (3, 8, 8), (3, 32, 32)))
def test_f32_exact_data_against_the_oracle(A, chw):
    afdm, dev = A
    for N in (1, 257):
        data = _grid((N,) + chw, 3000 + N)
        if N > 200:
            data[100] = data[40]
            data[200] = data[40]
        ds = afdm.DeviceDataset(data, device=dev)
        for n in QUERIES:
            queries = _grid((n,) + chw, 4000 + n)
            queries[0] = data[min(40, N - 1)]
            want_d, want_i = _oracle(afdm, data, queries, 16)
            assert want_d[0, 0] == 0
            ex = torch.full((n,), -1, dtype=torch.long)
            ex[0] = min(40, N - 1)
            ex_d, ex_i = _oracle(afdm, data, queries, 16, ex)
            qd = queries.to(dev)
            for k in KS:
                want = (want_d[:, :k], want_i[:, :k])
                for fill in (0xFF, 0x00):
                    assert _same(_abi(afdm, ds.images, qd, k, fill=fill), want), (N, n, k, fill)
                got = ds.nearest(queries, k)
                assert got[0].dtype == torch.float32 and _same(got, want), (N, n, k)
                assert _same(ds.nearest(queries, k, ex), (ex_d[:, :k], ex_i[:, :k])), (N, n, k)
                if N < k:
                    assert bool((got[1][:, N:] == -1).all()) and bool(torch.isposinf(got[0][:, N:]).all())


def test_f32_nan_and_infinite_rows_rank_last(A):
    afdm, dev = A
    chw, N, n = (3, 8, 8), 257, 17
    data, queries = _grid((N,) + chw, 21), _grid((n,) + chw, 22)
    data[5, 0, 0, 0] = float("nan")
    data[250, 2, 7, 7] = torch.tensor([-0x3edcba], dtype=torch.int32).view(torch.float32)[0]      # a negative NaN with a payload
    data[9, 1, 2, 3] = float("inf")
    data[130, 0, 5, 5] = float("-inf")
    queries[3, 1, 2, 3] = float("inf")                           # inf - inf against row 9: NaN there, +inf everywhere else
    ds = afdm.DeviceDataset(data, device=dev)
    want = _oracle(afdm, data, queries, 16)
    full = afdm.DeviceDataset(data, device="cpu")._nearest_torch(queries, N, None)       # every rank
    bits = full[0].view(torch.int32)
    assert full[1][0, -4:].tolist() == [9, 130, 5, 250] and bits[0, -4:].tolist() == [0x7f800000] * 2 + [0x7fc00000] * 2
    assert full[1][3, -3:].tolist() == [5, 9, 250] and bits[3].tolist() == [0x7f800000] * (N - 3) + [0x7fc00000] * 3
    assert want[1][3].tolist() == [i for i in range(19) if i not in (5, 9)][:16]
    for k in KS:
        assert _same(ds.nearest(queries, k), (want[0][:, :k], want[1][:, :k]))
        assert _same(_abi(afdm, ds.images, queries.to(dev), k), (want[0][:, :k], want[1][:, :k]))
    # the special rows themselves, reached through exclude: a store of the four of them
    rows = [9, 130, 5, 250]
    small = afdm.DeviceDataset(data[rows], device=dev)
    got = small.nearest(queries, 5)
    assert _same(got, _oracle(afdm, data[rows], queries, 5))
    assert got[1][0].tolist() == [0, 1, 2, 3, -1] and got[0][0].cpu().view(torch.int32).tolist() == [0x7f800000] * 2 + [0x7fc00000] * 2 + [0x7f800000]


# ---- 4. f32 on randn data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chw", ((3, 8, 8), (3, 32, 32)))
def test_f32_randn_within_one_ulp(A, chw):
    afdm, dev = A
    N, n, k = 257, 17, 8
    g = torch.Generator().manual_seed(31)
    data, queries = torch.randn((N,) + chw, generator=g), torch.randn((n,) + chw, generator=g)
    want_d, _ = _oracle(afdm, data, queries, k)
    for got_d, got_i in (afdm.DeviceDataset(data, device=dev).nearest(queries, k), _abi(afdm, data.to(dev), queries.to(dev), k)):
        got_d, got_i = got_d.cpu().double(), got_i.cpu()
        assert bool((got_i >= 0).all()) and bool((got_i < N).all())
        assert bool(((got_d - want_d.double()).abs() <= ULP * want_d.double()).all())
        d64 = ((data.double().view(N, -1)[got_i] - queries.double().view(n, 1, -1)) ** 2).sum(-1)
        assert bool(((got_d - d64).abs() <= ULP * d64).all())


# ---- 5. self_nearest ----------------------------------------------------------------------------------------------------------------
def test_self_nearest_is_leave_one_out(A):
    afdm, dev = A
    N = 300
    data = _u8((N, 3, 8, 8), 41)
    data[299] = data[0]
    ds = afdm.DeviceDataset(data, device=dev)
    got = ds.self_nearest(k=5, batch=128)                        # 128, 128, 44
    own = torch.arange(N)
    assert _same(got, _oracle(afdm, data, data, 5, own)) and _same(ds.nearest(data, 5, exclude=own), (got[0].cpu(), got[1].cpu()))
    assert got[1][0, 0] == 299 and got[0][0, 0] == 0 and not bool((got[1].cpu() == own.view(-1, 1)).any())


# ---- 6. ddpm_run --------------------------------------------------------------------------------------------------------------------
def test_ddpm_run_with_eval_nearest(A, tmp_path, monkeypatch):
    from PIL import Image
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    runs = {}
    for key in ("plain", "nearest"):
        wd = tmp_path / key
        wd.mkdir()
        np.savetxt(wd / "mnist.csv", arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42}
        if key == "nearest":
            params["eval_nearest"] = {"n": 3, "k": 2}
        out = afdm.ddpm_run(params)
        run_dir = os.path.join("runs", "DDPM_Uncondtional_MNIST_3")
        runs[key] = (out, open(os.path.join(run_dir, "settings_MNIST_3.txt")).read().replace(str(wd), ""), str(wd / run_dir))
    (po, pt, pdir), (no, nt, ndir) = runs["plain"], runs["nearest"]
    assert "nearest" not in po and pt == nt and po["loss_all"] == no["loss_all"]
    assert not [f for f in os.listdir(pdir) if f.startswith("nearest")]
    res = no["nearest"]
    with np.load(os.path.join(ndir, "nearest_MNIST_3.npz")) as z:
        assert set(z.files) == {"dist", "idx", "baseline_dist", "baseline_idx"}
        for name in z.files:
            assert z[name].shape == (3, 2) and np.array_equal(z[name], res[name], equal_nan=True)
    assert res["dist"].dtype == np.float32 and res["idx"].dtype == np.int64
    with Image.open(os.path.join(ndir, "nearest_MNIST_3.jpg")) as im:
        assert im.size == (3 * 34 + 2, 3 * 34 + 2)              # 3 rows of 1 + 2 images, 32 pixels and 2 of padding each
    # the saved samples against the training tensors, on the cpu
    monkeypatch.chdir(tmp_path / "nearest")
    args = afdm.argument(dataset_path="mnist.csv", batch_size=8)
    train = afdm.get_data_MNIST(args)[1].tensors[0]
    saved = torch.stack([torch.from_numpy(np.array(Image.open(os.path.join(no["gen_dir"], f"image_{i}.png")))) for i in range(3)])
    samples = afdm.data.normalisation_table(1)[0][saved.long()].view(3, 1, 32, 32)
    cpu = afdm.DeviceDataset(train, device="cpu")
    want = cpu.nearest(samples, 2)
    assert np.array_equal(res["dist"].view(np.int32), want[0].numpy().view(np.int32)) and np.array_equal(res["idx"], want[1].numpy())
    base = cpu.nearest(train[:3], 2, exclude=torch.arange(3))
    assert np.array_equal(res["baseline_dist"].view(np.int32), base[0].numpy().view(np.int32)) and np.array_equal(res["baseline_idx"], base[1].numpy())
    with pytest.raises(ValueError, match="eval_nearest n must be"):
        afdm.ddpm_run(dict(params, eval_nearest={"n": 5}))      # more than gen_total: fails before any training
