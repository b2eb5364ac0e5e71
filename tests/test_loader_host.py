"""The device-resident data set, host side: the C ABI's two entry points, the normalisation table, DeviceDataset on device="cpu"
(the pure-torch form that tests/test_gpu_loader.py uses as the kernels' oracle) against the host loaders it stands in for, the
batch order and random stream of DeviceLoader against torch's DataLoader, flips, and argument validation."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

ENTRY_POINTS = ("afd_batch_gather_u8", "afd_batch_gather_f32")
INT64_MIN = -2 ** 63


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg = ctypes.c_void_p, ctypes.c_long
    want = {"afd_batch_gather_u8": [vp, lg, lg, lg, lg, vp, vp, vp, vp, vp, vp, lg, vp],
            "afd_batch_gather_f32": [vp, lg, lg, lg, lg, vp, vp, vp, vp, vp, lg, vp]}
    for name in ENTRY_POINTS:
        assert name in sigs, name
        restype, argtypes = sigs[name]
        assert restype is ctypes.c_int and argtypes == want[name], name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))          # exported by the library, wrapped by the binding


def test_entry_points_reject_bad_arguments_before_any_launch():
    from afdm import AfdError, lib
    L = lib()
    p, q = 4096, 1 << 20                                 # non-NULL, aligned, apart: nothing is dereferenced before the checks pass
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_batch_gather_u8(p, 4, 3, 8, 8, p, None, None, q, None, None, 2, None)
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_batch_gather_f32(None, 4, 3, 8, 8, p, None, q, None, None, 2, None)
    with pytest.raises(AfdError, match="must be positive"):
        L.afd_batch_gather_f32(p, 4, 3, 8, 8, p, None, q, None, None, 0, None)
    with pytest.raises(AfdError, match="must be positive"):
        L.afd_batch_gather_u8(p, 0, 3, 8, 8, p, None, p, q, None, None, 2, None)
    with pytest.raises(AfdError, match="labels and y go together"):
        L.afd_batch_gather_f32(p, 4, 3, 8, 8, p, None, q, p, None, 2, None)
    with pytest.raises(AfdError, match="labels and y go together"):
        L.afd_batch_gather_u8(p, 4, 3, 8, 8, p, None, p, q, None, p, 2, None)
    with pytest.raises(AfdError, match="aligned"):
        L.afd_batch_gather_f32(p, 4, 3, 8, 8, p, None, q + 2, None, None, 2, None)
    with pytest.raises(AfdError, match="aligned"):
        L.afd_batch_gather_f32(p, 4, 3, 8, 8, p + 4, None, q, None, None, 2, None)
    with pytest.raises(AfdError, match="must not overlap"):
        L.afd_batch_gather_f32(p, 4, 3, 8, 8, q, None, p + 64, None, None, 2, None)


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def test_table_is_the_host_expression_bitwise():
    from afdm.data import DeviceDataset, normalisation_table
    u = torch.arange(256).float() / 255
    t = normalisation_table(3)
    assert t.dtype == torch.float32 and tuple(t.shape) == (3, 256)
    assert torch.equal(t, ((u - 0.5) / 0.5).expand(3, 256))
    m, s = [0.4914, 0.4822, 0.4465], [0.2470, 0.2435, 0.2616]
    want = torch.stack([(u - mc) / sc for mc, sc in zip(m, s)])
    for mean, std in ((m, s), (torch.tensor(m, dtype=torch.float64), np.array(s))):
        assert torch.equal(normalisation_table(3, mean, std), want)
    ds = DeviceDataset(torch.zeros(2, 3, 4, 4, dtype=torch.uint8), mean=m, std=s, device="cpu")
    assert torch.equal(ds.table, want) and ds.table.device.type == "cpu"
    assert DeviceDataset(torch.zeros(2, 3, 4, 4), device="cpu").table is None
    # every pixel value of every channel comes out as the table says
    px = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).repeat(1, 3, 1, 1)
    x, y = DeviceDataset(px, mean=m, std=s, device="cpu").batch(torch.zeros(1, dtype=torch.long))
    assert y is None and torch.equal(x[0].reshape(3, 256), want)


# ---- from_folder -------------------------------------------------------------------------------------------------------------------
def _write_folder(root, sizes=((40, 40),) * 9):
    from PIL import Image
    rng = np.random.default_rng(5)
    names = []
    for k, (w, h) in enumerate(sizes):
        cls = "zebra" if k % 2 else "ant"                 # 2 classes; sorted order: ant, zebra
        d = root / cls
        d.mkdir(parents=True, exist_ok=True)
        path = d / f"img_{k:02d}.png"
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)
        names.append(str(path))
    return names


def test_from_folder_is_the_host_loader_bitwise(tmp_path):
    from afdm.data import DeviceDataset, ImageFolder
    _write_folder(tmp_path / "data")
    host = ImageFolder(str(tmp_path / "data"), 32)
    ds = DeviceDataset.from_folder(str(tmp_path / "data"), 32, device="cpu")
    N = len(host)
    assert N == 9 and len(ds) == 9 and ds.images.dtype == torch.uint8 and tuple(ds.images.shape) == (9, 3, 32, 32)
    x, y = ds.batch(torch.arange(N))
    want = torch.stack([host[i][0] for i in range(N)])
    assert x.dtype == torch.float32 and torch.equal(x, want)
    assert y.tolist() == [host[i][1] for i in range(N)] == [0] * 5 + [1] * 4
    assert ds.classes == ["ant", "zebra"] == sorted(host.class_to_idx, key=host.class_to_idx.get)


def test_from_folder_rejects_shapes_that_do_not_collate(tmp_path):
    from afdm.data import DeviceDataset
    names = _write_folder(tmp_path / "data", ((40, 40), (40, 40), (40, 60), (40, 40)))
    with pytest.raises(ValueError) as e:
        DeviceDataset.from_folder(str(tmp_path / "data"), 32, device="cpu")
    assert names[2] in str(e.value)


def test_from_folder_cache_round_trip(tmp_path):
    from afdm.data import DeviceDataset
    root, cache = tmp_path / "data", tmp_path / "cache" / "set.npz"
    names = _write_folder(root)
    a = DeviceDataset.from_folder(str(root), 32, cache=str(cache), device="cpu")
    assert cache.exists()
    with np.load(cache, allow_pickle=False) as z:
        assert set(z.files) >= {"images", "labels", "classes"} and z["images"].dtype == np.uint8
    keep = {n: open(n, "rb").read() for n in names}
    for n in names:
        os.remove(n)
    b = DeviceDataset.from_folder(str(root), 32, cache=str(cache), device="cpu")           # the image files are gone
    assert torch.equal(a.images, b.images) and torch.equal(a.labels, b.labels) and a.classes == b.classes
    with pytest.raises(FileNotFoundError):
        DeviceDataset.from_folder(str(root), 16, cache=str(cache), device="cpu")           # another size: a rebuild, with nothing to read
    for n, data in keep.items():
        open(n, "wb").write(data)
    c = DeviceDataset.from_folder(str(root), 16, cache=str(cache), device="cpu")            # rebuilt at the new size
    assert tuple(c.images.shape) == (9, 3, 16, 16)
    with np.load(cache, allow_pickle=False) as z:
        assert tuple(z["images"].shape) == (9, 3, 16, 16)
    os.remove(names[0])                                                                      # another file list: a rebuild
    d = DeviceDataset.from_folder(str(root), 16, cache=str(cache), device="cpu")
    assert len(d) == 8 and torch.equal(d.images, c.images[1:])


def test_from_tensor_dataset_keeps_the_host_values():
    from afdm.data import DeviceDataset
    x = torch.randn(7, 1, 8, 8, generator=torch.Generator().manual_seed(0))
    lab = torch.arange(7) % 3
    ds = DeviceDataset.from_tensor_dataset(TensorDataset(x, lab), device="cpu")
    assert ds.images.dtype == torch.float32 and ds.table is None
    got, y = ds.batch(torch.tensor([6, 0, 6]))
    assert torch.equal(got, x[[6, 0, 6]]) and y.tolist() == [0, 0, 0]
    with pytest.raises(ValueError, match="TensorDataset"):
        DeviceDataset.from_tensor_dataset([x, lab], device="cpu")


# ---- batch: the pure-torch form ----------------------------------------------------------------------------------------------------
def test_batch_flips_bad_indices_and_labels_on_the_cpu():
    from afdm import NULL_LABEL
    from afdm.data import DeviceDataset
    g = torch.Generator().manual_seed(1)
    px = torch.randint(0, 256, (5, 3, 4, 6), generator=g, dtype=torch.uint8)
    ds = DeviceDataset(px, torch.arange(5) * 10, mean=[0.1, 0.2, 0.3], std=[0.5, 0.25, 2.0], device="cpu")
    idx = torch.tensor([4, -1, 0, 5, 4, 2 ** 40])
    flip = torch.tensor([1, 1, 0, 0, 0, 1], dtype=torch.uint8)
    x, y = ds.batch(idx, flip)
    chan = torch.arange(3).view(3, 1, 1)
    assert torch.equal(x[0], ds.table[chan, px[4].long()].flip(-1))
    assert torch.equal(x[2], ds.table[chan, px[0].long()]) and torch.equal(x[4], ds.table[chan, px[4].long()])
    assert torch.isnan(x[[1, 3, 5]]).all() and not torch.isnan(x[[0, 2, 4]]).any()
    assert y.tolist() == [40, INT64_MIN, 0, INT64_MIN, 40, INT64_MIN] and INT64_MIN != NULL_LABEL
    assert torch.equal(ds.batch(idx, flip.bool())[0].view(torch.int32), x.view(torch.int32))
    # the f32 form moves bits
    f = torch.tensor([0x7fc01234, 0x7f800000, -0x00800000, -0x80000000, 0x3f800000, 0x00000001], dtype=torch.int32)
    f = f.view(torch.float32).view(1, 1, 1, 6).repeat(2, 1, 1, 1)
    xf, yf = DeviceDataset(f, device="cpu").batch(torch.tensor([1, 0]), torch.tensor([True, False]))
    assert yf is None and torch.equal(xf[0].view(torch.int32), f[1].flip(-1).view(torch.int32))
    assert torch.equal(xf[1].view(torch.int32), f[0].view(torch.int32))


# ---- order and random stream -------------------------------------------------------------------------------------------------------
def test_order_and_random_stream_are_the_host_loaders():
    from afdm.data import DeviceDataset, DeviceLoader
    N, B = 1003, 64
    images, labels = torch.zeros(N, 1, 2, 2), torch.arange(N)

    def drive(loader):
        torch.manual_seed(3)
        seen, draws = [], []
        for _ in range(2):
            for x, y in loader:
                seen.append(y.clone())
                draws.append(torch.randint(low=1, high=1000, size=(x.shape[0],)))      # what sample_timesteps draws per batch
        return seen, draws, torch.rand(1)

    ds = DeviceDataset(images, labels, device="cpu")
    loader = DeviceLoader(ds, B)
    assert loader.dataset is ds and len(loader) == 16
    host = DataLoader(TensorDataset(images, labels), B, shuffle=True)
    (a, da, ra), (b, db, rb) = drive(loader), drive(host)
    assert len(a) == len(b) == 32 and all(torch.equal(p, q) for p, q in zip(a, b))
    assert all(torch.equal(p, q) for p, q in zip(da, db)) and torch.equal(ra, rb)
    assert a[15].numel() == 43 and a[31].numel() == 43 and sorted(torch.cat(a[:16]).tolist()) == list(range(N))
    assert not torch.equal(torch.cat(a[:16]), torch.arange(N)) and not torch.equal(torch.cat(a[:16]), torch.cat(a[16:]))
    short = DeviceLoader(ds, B, drop_last=True)
    assert len(short) == 15 and [y.numel() for _, y in short] == [64] * 15
    plain = DeviceLoader(ds, B, shuffle=False)
    assert torch.equal(torch.cat([y for _, y in plain]), torch.arange(N))
    # every batch is a tensor of its own
    xs = [x for x, _ in DeviceLoader(ds, 500, shuffle=False)]
    assert len({x.data_ptr() for x in xs}) == 3 and [x.shape[0] for x in xs] == [500, 500, 3]


# ---- flips -------------------------------------------------------------------------------------------------------------------------
def test_flip_bits_come_from_the_loaders_own_generator():
    from afdm.data import DeviceDataset, DeviceLoader
    N = 200
    ramp = torch.arange(8, dtype=torch.float32).view(1, 1, 1, 8).repeat(N, 1, 1, 1)      # row b is flipped iff x[b, 0, 0, 0] == 7
    ds = DeviceDataset(ramp, torch.arange(N), device="cpu")

    def bits(loader):
        got = torch.zeros(N, dtype=torch.bool)
        for x, y in loader:
            assert ((x[:, 0, 0, 0] == 7) | (x[:, 0, 0, 0] == 0)).all()
            got[y] = x[:, 0, 0, 0] == 7
        return got

    a, b, c = (bits(DeviceLoader(ds, 32, shuffle=False, flip_prob=0.5, seed=s)) for s in (11, 11, 12))
    assert torch.equal(a, b) and not torch.equal(a, c) and 60 < int(a.sum()) < 140
    loader = DeviceLoader(ds, 32, shuffle=False, flip_prob=0.5, seed=11)
    first, second = bits(loader), bits(loader)
    assert torch.equal(first, a) and not torch.equal(second, first)                        # a new draw every epoch
    # flips never touch the global generator: the draw itself leaves it as it was, and an epoch with flips leaves it where an epoch
    # without them does (torch's DataLoader takes its base seed from it at the start of every epoch, as on the host)
    torch.manual_seed(9)
    before = torch.get_rng_state()
    flips = DeviceLoader(ds, 32, shuffle=True, flip_prob=0.5, seed=1)
    assert flips._gen is not torch.default_generator
    assert int((torch.rand(N, generator=flips._gen) < 0.5).sum()) > 0 and torch.equal(torch.get_rng_state(), before)
    bits(flips)
    after = torch.get_rng_state()
    torch.manual_seed(9)
    bits(DeviceLoader(ds, 32, shuffle=True, flip_prob=0.0))
    assert torch.equal(torch.get_rng_state(), after) and not torch.equal(after, before)
    assert bits(DeviceLoader(ds, 32, flip_prob=1.0, seed=0)).all()
    assert not bits(DeviceLoader(ds, 32, flip_prob=0.0, seed=0)).any()
    idx, flip = DeviceLoader(ds, 32, flip_prob=0.0).epoch_plan()
    assert flip is None and idx.numel() == N


# ---- validation --------------------------------------------------------------------------------------------------------------------
def test_every_argument_error_names_its_argument():
    from afdm.data import DeviceDataset, DeviceLoader
    u8 = torch.zeros(4, 3, 2, 2, dtype=torch.uint8)
    for bad in (u8.to(torch.float64), u8.to(torch.int32), u8.to(torch.float16), [[[[0]]]]):
        with pytest.raises(ValueError, match="images must be a uint8 or float32"):
            DeviceDataset(bad, device="cpu")
    for bad in (u8[0], u8[None], u8[:0]):
        with pytest.raises(ValueError, match="4-D"):
            DeviceDataset(bad, device="cpu")
    for std in (0, 0.0, [0.5, 0.0, 0.5]):
        with pytest.raises(ValueError, match="std must not contain 0"):
            DeviceDataset(u8, std=std, device="cpu")
    for name, kw in (("mean", {"mean": [0.5, 0.5]}), ("std", {"std": [0.5] * 4}), ("mean", {"mean": "x"}), ("std", {"std": float("nan")})):
        with pytest.raises(ValueError, match=f"DeviceDataset: {name} must be"):
            DeviceDataset(u8, device="cpu", **kw)
    for bad in (torch.zeros(3, dtype=torch.long), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 1, dtype=torch.long), [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="labels must be"):
            DeviceDataset(u8, bad, device="cpu")
    ds = DeviceDataset(u8, device="cpu")
    for bad in (torch.zeros(2, dtype=torch.int32), torch.zeros(2), [0, 1], torch.zeros(2, 1, dtype=torch.long), torch.zeros(0, dtype=torch.long)):
        with pytest.raises(ValueError, match="idx must be"):
            ds.batch(bad)
    for bad in (torch.zeros(3, dtype=torch.uint8), torch.zeros(2), [0, 1]):
        with pytest.raises(ValueError, match="flip must be"):
            ds.batch(torch.zeros(2, dtype=torch.long), bad)
    for bad in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="flip_prob must lie in"):
            DeviceLoader(ds, 2, flip_prob=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="batch_size must be"):
            DeviceLoader(ds, bad)
    with pytest.raises(ValueError, match="dataset must be a DeviceDataset"):
        DeviceLoader(TensorDataset(u8), 2)
    with pytest.raises(ValueError, match="seed must be"):
        DeviceLoader(ds, 2, seed=1.5)


def test_public_names():
    import afdm
    import modules.utils as U
    from afdm import data
    for name in ("DeviceDataset", "DeviceLoader", "get_data_device", "get_data_MNIST_device"):
        assert getattr(afdm, name) is getattr(data, name) is getattr(U, name)
