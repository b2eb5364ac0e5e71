"""Nearest-training-image search, host side: the C ABI's three entry points and their argument checks, the workspace bound, the
pure-torch brute force of DeviceDataset.nearest on device="cpu" (the oracle of tests/test_gpu_nearest.py) against a numpy brute
force written here, argument validation, the public names and the eval_nearest key of ddpm_run."""
import ctypes

import numpy as np
import pytest
import torch

ENTRY_POINTS = ("afd_nn_search_workspace_bytes", "afd_nn_search_u8", "afd_nn_search_f32")
NAN_BITS, INF_BITS = 0x7fc00000, 0x7f800000


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg, sz = ctypes.c_void_p, ctypes.c_long, ctypes.c_size_t
    search = [vp, lg, lg, vp, lg, vp, lg, vp, vp, vp, sz, vp]
    want = {"afd_nn_search_workspace_bytes": (sz, [lg, lg, lg, lg, ctypes.c_int]), "afd_nn_search_u8": (ctypes.c_int, search),
            "afd_nn_search_f32": (ctypes.c_int, search)}
    for name in ENTRY_POINTS:
        assert name in sigs, name
        assert sigs[name] == want[name], name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))          # exported by the library, wrapped by the binding


@pytest.mark.parametrize("fn", ("afd_nn_search_u8", "afd_nn_search_f32"))
def test_entry_points_reject_bad_arguments_before_any_launch(fn):
    from afdm import AfdError, lib
    L = lib()
    call = getattr(L, fn)
    f32 = fn.endswith("f32")
    N, D, n, k = 100, 64, 8, 4
    need = L.afd_nn_search_workspace_bytes(N, D, n, k, int(f32))
    assert need > 0
    # non-NULL, aligned, far apart: nothing is dereferenced before the checks pass
    good = {"data": 1 << 20, "N": N, "D": D, "queries": 2 << 20, "n": n, "exclude": 3 << 20, "k": k, "idx": 4 << 20, "dist": 5 << 20,
            "workspace": 6 << 20, "bytes": need}

    def bad(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(AfdError, match=match):
            call(a["data"], a["N"], a["D"], a["queries"], a["n"], a["exclude"], a["k"], a["idx"], a["dist"], a["workspace"], a["bytes"], None)

    for name in ("data", "queries", "idx", "dist", "workspace"):
        bad(f"{name} must not be NULL", **{name: None})
    for name in ("N", "D", "n"):
        for v in (0, -3):
            bad("N, D and n must be positive", **{name: v})
    for v in (0, 17, -1):
        bad(r"k must lie in \[1, 16\]", k=v)
    if not f32:
        bad("D must be at most 32768", D=32769, bytes=1 << 30)
    bad("N and n must be below 2\\^31", N=1 << 31, bytes=1 << 40)
    bad("idx must be 8-byte aligned", idx=good["idx"] + 4)
    bad("dist must be . 8-byte aligned".replace(". 8", "4" if f32 else "8"), dist=good["dist"] + 2)
    bad("exclude must be 8-byte aligned", exclude=good["exclude"] + 4)
    bad("workspace must be 8-byte aligned", workspace=good["workspace"] + 4)
    if f32:
        bad("data and queries must be 4-byte aligned", data=good["data"] + 2)
        bad("data and queries must be 4-byte aligned", queries=good["queries"] + 1)
    bad("workspace too small", bytes=need - 1)
    bad("workspace too small", bytes=0)
    esz = 4 if f32 else 1
    for out in ("idx", "dist", "workspace"):
        bad("must not overlap data", **{out: good["data"] + N * D * esz - 8})
        bad("must not overlap queries", **{out: good["queries"] + 8})
        bad("must not overlap exclude", **{out: good["exclude"] + 8 * (n - 1)})
    bad("must not overlap each other", dist=good["idx"] + 8)
    bad("must not overlap each other", workspace=good["idx"] + n * k * 8 - 8)
    bad("must not overlap each other", workspace=good["dist"] - need + 8)


def test_workspace_is_positive_monotone_and_bounded():
    from afdm import lib, ops
    ws = lib().afd_nn_search_workspace_bytes
    for f32 in (0, 1):
        assert ws(1, 1, 1, 1, f32) > 0
        for N in (1, 257, 60000):
            sizes = [[ws(N, 1024, n, k, f32) for k in range(1, 17)] for n in (1, 2, 17, 1000, 100000)]
            assert all(s > 0 for row in sizes for s in row)
            assert all(a < b for row in sizes for a, b in zip(row, row[1:]))                     # in k
            assert all(a < b for lo, hi in zip(sizes, sizes[1:]) for a, b in zip(lo, hi))         # in n
        assert ws(0, 8, 1, 1, f32) == 0 and ws(8, 8, 1, 17, f32) == 0
        # what ops.nn_search passes: the queries in groups, one workspace
        for k in (1, 5, 16):
            for D in (1024, 3072):
                group = ops.nn_group(60000, D, 100000, k, bool(f32))
                assert 1 <= group <= 100000
                assert 0 < ws(60000, D, group, k, f32) <= ops.NN_WORKSPACE_LIMIT == 64 << 20
        assert ops.nn_group(60000, 1024, 100000, 16, bool(f32)) >= 256                           # (and not one query at a time)


# ---- the cpu oracle against numpy ------------------------------------------------------------------------------------------------
def _numpy_nearest(data, queries, k, exclude=None):
    """int64 (uint8) or fp64 rounded once to fp32, then np.lexsort on (index, distance); NaN ranks last, as the canonical NaN."""
    N, n = data.shape[0], queries.shape[0]
    a, q = data.reshape(N, -1), queries.reshape(n, -1)
    u8 = a.dtype == np.uint8
    idx = np.full((n, k), -1, np.int64)
    dist = np.full((n, k), -1, np.int64) if u8 else np.full((n, k), np.inf, np.float32)
    for i in range(n):
        with np.errstate(invalid="ignore", over="ignore"):
            if u8:
                d = ((a.astype(np.int64) - q[i].astype(np.int64)) ** 2).sum(1)
                rank = d
            else:
                d = ((a.astype(np.float64) - q[i].astype(np.float64)) ** 2).sum(1).astype(np.float32)
                d[np.isnan(d)] = np.array([NAN_BITS], np.uint32).view(np.float32)[0]
                rank = d.view(np.uint32).astype(np.int64)          # non-negative floats and the canonical NaN: monotone bits
        order = np.lexsort((np.arange(N), rank))
        if exclude is not None:
            order = order[order != exclude[i]]
        m = min(k, order.size)
        idx[i, :m], dist[i, :m] = order[:m], d[order[:m]]
    return dist, idx


def _check(images, queries, k, exclude=None):
    from afdm.data import DeviceDataset
    ds = DeviceDataset(torch.from_numpy(images), device="cpu")
    ex = None if exclude is None else torch.from_numpy(np.asarray(exclude, np.int64))
    dist, idx = ds.nearest(torch.from_numpy(queries), k, ex)
    want_d, want_i = _numpy_nearest(images, queries, k, exclude)
    assert idx.dtype == torch.long and tuple(idx.shape) == (queries.shape[0], k) == tuple(dist.shape)
    assert np.array_equal(idx.numpy(), want_i)
    if images.dtype == np.uint8:
        assert dist.dtype == torch.long and np.array_equal(dist.numpy(), want_d)
    else:
        assert dist.dtype == torch.float32 and np.array_equal(dist.numpy().view(np.uint32), want_d.view(np.uint32))
    return dist, idx


def test_cpu_oracle_u8_duplicates_exclude_and_sentinels():
    rng = np.random.default_rng(0)
    images = rng.integers(0, 256, (23, 3, 4, 5), dtype=np.uint8)
    images[7] = images[3]
    images[19] = images[3]                                   # three equal rows: ties go to the lower index
    images[11] = images[2]
    queries = np.concatenate([images[[3, 2, 22]], rng.integers(0, 256, (4, 3, 4, 5), dtype=np.uint8)])
    for k in (1, 5, 16):
        dist, idx = _check(images, queries, k)
        assert dist[:3, 0].tolist() == [0, 0, 0] and idx[:3, 0].tolist() == [3, 2, 22]
        if k >= 5:
            assert idx[0, :3].tolist() == [3, 7, 19] and idx[1, :2].tolist() == [2, 11]
    ex = np.array([3, 11, 22, -1, -7, 0, 22], np.int64)
    dist, idx = _check(images, queries, 5, ex)
    assert idx[0, :2].tolist() == [7, 19] and idx[1, 0] == 2 and not (idx == torch.from_numpy(ex).view(-1, 1)).any()
    none = _check(images, queries, 5, np.full(7, -1, np.int64))
    plain = _check(images, queries, 5)
    assert torch.equal(none[0], plain[0]) and torch.equal(none[1], plain[1])
    # k exceeds the rows available
    small = images[:3]
    dist, idx = _check(small, queries, 5)
    assert (idx[:, 3:] == -1).all() and (dist[:, 3:] == -1).all() and (idx[:, :3] >= 0).all()
    dist, idx = _check(small, queries[:3], 3, np.array([0, 1, -1], np.int64))
    assert idx[0].tolist()[2] == -1 and idx[1].tolist()[2] == -1 and idx[2].tolist()[2] >= 0
    dist, idx = _check(images[:1], queries[:2], 2, np.array([0, 5], np.int64))
    assert idx.tolist() == [[-1, -1], [0, -1]] and dist[0].tolist() == [-1, -1]
    # the extremes: 0 against 255 everywhere
    lo, hi = np.zeros((2, 1, 8, 8), np.uint8), np.full((1, 1, 8, 8), 255, np.uint8)
    dist, _ = _check(lo, hi, 1)
    assert dist.item() == 64 * 255 ** 2


def test_cpu_oracle_f32_rounds_once_and_orders_ties_by_index():
    # distances that differ in fp64 and round to the same fp32: the order among them is the index order
    images = np.zeros((6, 1, 1, 2), np.float32)
    images[:, 0, 0, 0] = 1.0
    images[:, 0, 0, 1] = np.array([3e-5, 1e-5, 2e-5, 0.5, 1e-5, 0.0], np.float32)
    queries = np.zeros((1, 1, 1, 2), np.float32)
    d64 = ((images.reshape(6, 2).astype(np.float64)) ** 2).sum(1)
    assert len(set(d64[[0, 1, 2, 5]].tolist())) == 4 and len(set(d64.astype(np.float32)[[0, 1, 2, 4, 5]].tolist())) == 1
    dist, idx = _check(images, queries, 6)
    assert idx[0].tolist() == [0, 1, 2, 4, 5, 3]
    rng = np.random.default_rng(1)
    images = rng.standard_normal((40, 2, 3, 5)).astype(np.float32)
    images[9] = images[4]
    queries = np.concatenate([images[[4]], rng.standard_normal((5, 2, 3, 5)).astype(np.float32)])
    for k in (1, 7, 16):
        _check(images, queries, k)
    dist, idx = _check(images, queries, 4, np.array([4, -1, 0, 1, 2, 39], np.int64))
    assert idx[0, 0] == 9 and dist[0, 0] == 0
    dist, idx = _check(images[:2], queries, 4)
    assert (idx[:, 2:] == -1).all() and torch.isinf(dist[:, 2:]).all() and (dist[:, 2:] > 0).all()


def test_cpu_oracle_f32_nan_and_infinite_rows():
    rng = np.random.default_rng(2)
    images = rng.standard_normal((9, 1, 2, 4)).astype(np.float32)
    images[2, 0, 0, 1] = np.nan
    images[6, 0, 1, 0] = np.array([0xffc12345], np.uint32).view(np.float32)[0]      # another NaN, negative with a payload
    images[4, 0, 0, 0] = np.inf
    images[7, 0, 1, 3] = -np.inf
    images[1] *= 1e20                                                               # a finite fp64 sum that rounds to +inf
    queries = rng.standard_normal((3, 1, 2, 4)).astype(np.float32)
    queries[2, 0, 0, 0] = np.inf                                                    # inf - inf against row 4: NaN
    dist, idx = _check(images, queries, 9)
    bits = dist.view(torch.int32)
    for q in range(2):
        assert idx[q, 4:].tolist() == [1, 4, 7, 2, 6]
        assert bits[q, 4:].tolist() == [INF_BITS] * 3 + [NAN_BITS] * 2
    assert idx[2, -3:].tolist() == [2, 4, 6] and bits[2].tolist() == [INF_BITS] * 6 + [NAN_BITS] * 3
    _check(images, queries, 16)


def test_self_nearest_on_the_cpu_is_leave_one_out():
    from afdm.data import DeviceDataset
    g = torch.Generator().manual_seed(4)
    images = torch.randint(0, 256, (50, 1, 3, 3), generator=g, dtype=torch.uint8)
    images[30] = images[10]
    ds = DeviceDataset(images, device="cpu")
    dist, idx = ds.self_nearest(k=3, batch=16)
    want = ds.nearest(images, 3, exclude=torch.arange(50))
    assert torch.equal(dist, want[0]) and torch.equal(idx, want[1])
    assert not (idx == torch.arange(50).view(-1, 1)).any() and idx[10, 0] == 30 and idx[30, 0] == 10 and dist[10, 0] == 0
    with pytest.raises(ValueError, match="batch must be"):
        ds.self_nearest(batch=0)


# ---- validation --------------------------------------------------------------------------------------------------------------------
def test_every_argument_error_names_its_argument():
    from afdm.data import DeviceDataset
    u8 = torch.zeros(4, 3, 2, 2, dtype=torch.uint8)
    ds, fs = DeviceDataset(u8, device="cpu"), DeviceDataset(u8.float(), device="cpu")
    for d, bad in ((ds, u8.float()), (fs, u8), (ds, u8.long()), (ds, [[[[0]]]])):
        with pytest.raises(ValueError, match="nearest: queries must be a tensor of the store's dtype"):
            d.nearest(bad)
    for bad in (u8[0], u8[:, :2], u8[:, :, :1], u8.reshape(4, 12), u8.permute(0, 2, 3, 1)):
        with pytest.raises(ValueError, match=r"nearest: queries must have the shape \(n, 3, 2, 2\)"):
            ds.nearest(bad)
    with pytest.raises(ValueError, match="n >= 1"):
        ds.nearest(u8[:0])
    for bad in (0, 17, -1, 2.0, None, True, "3"):
        with pytest.raises(ValueError, match=r"nearest: k must be an int in \[1, 16\]"):
            ds.nearest(u8, k=bad)
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.long), [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="nearest: exclude must be None or an int64 tensor of shape"):
            ds.nearest(u8, exclude=bad)
    big = DeviceDataset(torch.zeros(1, 3, 128, 128, dtype=torch.uint8), device="cpu")
    with pytest.raises(ValueError, match="at most 32768 elements"):
        big.nearest(big.images)


def test_public_names():
    import afdm
    import modules.utils as U
    from afdm import data, ops
    assert afdm.nn_search is ops.nn_search is U.nn_search
    assert afdm.DeviceDataset is data.DeviceDataset is U.DeviceDataset
    for name in ("nearest", "self_nearest"):
        assert callable(getattr(U.DeviceDataset, name))


def test_eval_nearest_key_check():
    from afdm.tasks import _nearest_cfg
    p = {"gen_total": 8}
    assert _nearest_cfg(dict(p, eval_nearest={"n": 4})) == {"n": 4, "k": 5}
    assert _nearest_cfg(dict(p, eval_nearest={"n": 8, "k": 16})) == {"n": 8, "k": 16}
    for bad in ({}, {"k": 3}, {"n": 4, "K": 3}, {"n": 4, "k": 3, "batch": 2}, 4, [4, 5]):
        with pytest.raises(ValueError, match="eval_nearest needs n"):
            _nearest_cfg(dict(p, eval_nearest=bad))
    for bad in (0, 9, -1, 2.0, True, None, "4"):
        with pytest.raises(ValueError, match="eval_nearest n must be"):
            _nearest_cfg(dict(p, eval_nearest={"n": bad}))
    for bad in (0, 17, 2.5, True, None):
        with pytest.raises(ValueError, match="eval_nearest k must be"):
            _nearest_cfg(dict(p, eval_nearest={"n": 4, "k": bad}))
