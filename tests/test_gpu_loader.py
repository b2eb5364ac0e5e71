"""Batch assembly from a device-resident data set on the GPU: afd_batch_gather_u8 / afd_batch_gather_f32 through the C ABI and
through DeviceDataset.batch, against the pure-torch form (DeviceDataset on device="cpu", pinned to the host loaders by
tests/test_loader_host.py), and train() fed by DeviceLoader against train() fed by torch's DataLoader.  Every comparison is of
bits: torch.equal on int32 views, no tolerance anywhere."""
import math

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
N = 37
SHAPES = ((32, 32), (8, 8), (5, 7), (4, 48))      # 16-byte path (u8: 2 chunks per row), f32-only 16-byte path, scalar, 3 chunks per row
BATCHES = (1, 5, 70)                              # 70 > N: repeated indices
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2470, 0.2435, 0.2616)
INT64_MIN = -2 ** 63
CANARY = 12345.0


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _store(kind, C, H, W, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * C + 10 * H + W)
    if kind == "u8":
        return torch.randint(0, 256, (N, C, H, W), generator=g, dtype=torch.uint8)
    x = torch.randn(N, C, H, W, generator=g)
    flat = x.view(torch.int32).view(-1)
    special = torch.tensor([0x7fc01234, 0x7f800000, -0x00800000, -0x80000000, 0x7f812345], dtype=torch.int32)
    pos = torch.randperm(flat.numel(), generator=g)[:5 * 8].view(8, 5)      # quiet and signalling NaN payloads, +-inf, -0.0
    for row in pos:
        flat[row] = special
    return x


def _pair(afdm, dev, kind, C, H, W, labels=True):
    """The same store on the CPU (the oracle) and on the device."""
    data = _store(kind, C, H, W)
    lab = (torch.arange(N) * 7919) % 1000 - 3 if labels else None
    kw = {"mean": MEAN[:C], "std": STD[:C]}
    return afdm.DeviceDataset(data, lab, device="cpu", **kw), afdm.DeviceDataset(data, lab, device=dev, **kw)


def _indices(B, seed=0):
    return torch.randint(0, N, (B,), generator=torch.Generator().manual_seed(100 + B + seed))


def _flips(B):
    return (None, torch.ones(B, dtype=torch.uint8), (torch.arange(B) % 2).to(torch.uint8))


def _gather(afdm, ds, idx, flip, x, y):
    """The C ABI, with raw pointers: x and y are written in place."""
    L, n, (Nn, C, H, W) = afdm.lib(), idx.numel(), ds.images.shape
    p = lambda t: None if t is None else t.data_ptr()
    if ds.images.dtype == torch.uint8:
        L.afd_batch_gather_u8(p(ds.images), Nn, C, H, W, p(idx), p(flip), p(ds.table), p(x), p(ds.labels), p(y), n, afdm.ops._stream())
    else:
        L.afd_batch_gather_f32(p(ds.images), Nn, C, H, W, p(idx), p(flip), p(x), p(ds.labels), p(y), n, afdm.ops._stream())


def _view_at(dev, n, dtype, skip, tail=64, fill=None):
    """(the whole buffer, a contiguous n-element view that starts `skip` elements into it)."""
    buf = torch.empty(skip + n + tail, device=dev, dtype=dtype)
    if fill is not None:
        buf.fill_(fill)
    return buf, buf[skip:skip + n]


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_gather_through_the_c_abi(A, kind, C, hw):
    """Every batch size and flip pattern, x 16-byte aligned (the 16-byte path where the shape allows it) and x 4 bytes into its
    allocation (the scalar path), idx a view at offset 1 of a longer buffer; a canary around x stays as it was."""
    afdm, dev = A
    H, W = hw
    cpu, ds = _pair(afdm, dev, kind, C, H, W)
    chw = C * H * W
    for B in BATCHES:
        idx = _indices(B)
        _, idx_d = _view_at(dev, B, torch.long, 1)
        idx_d.copy_(idx)
        assert idx_d.data_ptr() % 16 == 8
        for flip in _flips(B):
            want_x, want_y = cpu.batch(idx, flip)
            flip_d = None if flip is None else flip.to(dev)
            for skip in (4, 1):
                buf, x = _view_at(dev, B * chw, torch.float32, skip, fill=CANARY)
                assert x.data_ptr() % 16 == (0 if skip == 4 else 4)
                y = torch.full((B,), -77, device=dev, dtype=torch.long)
                _gather(afdm, ds, idx_d, flip_d, x, y)
                assert torch.equal(_bits(x.view(B, C, H, W)), _bits(want_x)), (B, skip, flip is not None)
                assert torch.equal(y.cpu(), want_y)
                assert bool((buf[:skip] == CANARY).all()) and bool((buf[skip + B * chw:] == CANARY).all())


@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_a_store_view_that_is_only_4_or_8_byte_aligned(A, kind):
    afdm, dev = A
    C, H, W, B = 3, 32, 32, 5
    cpu, ds = _pair(afdm, dev, kind, C, H, W)
    idx = _indices(B)
    flip = (torch.arange(B) % 2).to(torch.uint8)
    want_x, want_y = cpu.batch(idx, flip)
    for skip_bytes in (4, 8):
        skip = skip_bytes // ds.images.element_size()
        _, flat = _view_at(dev, ds.images.numel(), ds.images.dtype, skip)
        flat.copy_(ds.images.view(-1))
        moved = afdm.DeviceDataset.__new__(afdm.DeviceDataset)
        moved.images, moved.labels, moved.table, moved.device = flat.view(N, C, H, W), ds.labels, ds.table, ds.device
        assert moved.images.data_ptr() % 16 == skip_bytes
        x, y = moved.batch(idx, flip)
        assert torch.equal(_bits(x), _bits(want_x)) and torch.equal(y.cpu(), want_y)


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_dataset_batch_on_the_device(A, kind, hw):
    afdm, dev = A
    H, W = hw
    for C in (1, 3):
        cpu, ds = _pair(afdm, dev, kind, C, H, W)
        assert ds.images.is_cuda and ds.labels.is_cuda and (ds.table is None or ds.table.is_cuda) and len(ds) == N
        for B in BATCHES:
            idx = _indices(B, seed=1)
            for flip in _flips(B):
                want_x, want_y = cpu.batch(idx, flip)
                for f in (flip, None if flip is None else flip.bool().to(dev)):
                    x, y = ds.batch(idx.to(dev), f)
                    assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, C, H, W) and y.dtype == torch.long
                    assert torch.equal(_bits(x), _bits(want_x)) and torch.equal(y.cpu(), want_y)
        a, b = ds.batch(torch.arange(4)), ds.batch(torch.arange(4))                  # a CPU index is moved; every batch is its own tensor
        assert a[0].data_ptr() != b[0].data_ptr() and torch.equal(_bits(a[0]), _bits(b[0]))


@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_without_labels_nothing_is_gathered(A, kind):
    afdm, dev = A
    cpu, ds = _pair(afdm, dev, kind, 3, 8, 8, labels=False)
    idx = _indices(5)
    x, y = ds.batch(idx)
    assert y is None and cpu.batch(idx)[1] is None and torch.equal(_bits(x), _bits(cpu.batch(idx)[0]))
    with pytest.raises(afdm.AfdError, match="labels and y go together"):
        _gather(afdm, ds, idx.to(dev), None, torch.empty(5 * 3 * 64, device=dev), torch.empty(5, device=dev, dtype=torch.long))


@pytest.mark.parametrize("hw", ((32, 32), (5, 7)))
@pytest.mark.parametrize("kind", ("u8", "f32"))
def test_an_index_outside_the_store_gives_a_nan_row_and_reads_nothing(A, kind, hw):
    """Defined behaviour of the kernel: the row is quiet NaN, its label INT64_MIN, every other row exact, nothing written past x."""
    afdm, dev = A
    H, W = hw
    C = 3
    cpu, ds = _pair(afdm, dev, kind, C, H, W)
    idx = torch.tensor([3, -1, 0, N, N - 1, 2 ** 40, 5, -2 ** 63, 2 ** 63 - 1])
    bad = torch.tensor([False, True, False, True, False, True, False, True, True])
    B, chw = idx.numel(), C * H * W
    for flip in _flips(B):
        want_x, want_y = cpu.batch(idx, flip)
        assert torch.isnan(want_x[bad]).all() and not torch.isnan(want_x[~bad]).all(dim=(1, 2, 3)).any()
        assert (want_y[bad] == INT64_MIN).all() and (want_y[~bad] != INT64_MIN).all()
        buf, x = _view_at(dev, B * chw, torch.float32, 4, tail=4096, fill=CANARY)
        y = torch.full((B,), -77, device=dev, dtype=torch.long)
        _gather(afdm, ds, idx.to(dev), None if flip is None else flip.to(dev), x, y)
        got = x.view(B, C, H, W)
        assert torch.equal(_bits(got), _bits(want_x)) and bool((_bits(got[bad]) == 0x7fc00000).all())
        assert torch.equal(y.cpu(), want_y)
        assert bool((buf[:4] == CANARY).all()) and bool((buf[4 + B * chw:] == CANARY).all())
        x2, y2 = ds.batch(idx, flip)
        assert torch.equal(_bits(x2), _bits(want_x)) and torch.equal(y2.cpu(), want_y)


def test_device_loader_on_the_device_follows_the_cpu_loader(A):
    afdm, dev = A
    cpu, ds = _pair(afdm, dev, "u8", 3, 32, 32)
    runs = []
    for d in (cpu, ds):
        torch.manual_seed(5)
        runs.append([(x.cpu(), y.cpu()) for _ in range(2) for x, y in afdm.DeviceLoader(d, 16, flip_prob=0.5, seed=7)])
    assert [x.shape[0] for x, _ in runs[1]] == [16, 16, 5] * 2
    assert all(torch.equal(_bits(a), _bits(c)) and torch.equal(b, e) for (a, b), (c, e) in zip(*runs))


def _train(afdm, dev, loader, tmp):
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=10, img_size=32, device=dev)
    args = afdm.argument(run_name="loader", epochs=1, batch_size=16, image_size=32, image_channels=3, device=dev, lr=3e-4,
                         noise_steps=10, image_gen_n=1)
    afdm.set_seed(11)
    ckpt = tmp / "ckpt.pt"
    losses = afdm.train(args, model_path=str(ckpt), dataloader=loader, model=model, diffusion=diff)
    return losses, torch.load(str(ckpt), weights_only=True)


def test_train_fed_by_the_device_loader_is_train_fed_by_the_host_loader(A, tmp_path, monkeypatch):
    """40 random uint8 images, one epoch of batches 16, 16, 8: the same losses and the same weights, bit for bit -- the order, the
    random stream, the normalisation, and a step that never notices where its batch came from."""
    afdm, dev = A
    g = torch.Generator().manual_seed(3)
    px = torch.randint(0, 256, (40, 3, 32, 32), generator=g, dtype=torch.uint8)
    labels = torch.arange(40) % 10
    ds = afdm.DeviceDataset(px, labels, device=dev)
    host_images = ds.table.cpu()[torch.arange(3).view(1, 3, 1, 1), px.long()]
    assert torch.equal(host_images, (px.float() / 255.0 - 0.5) / 0.5)
    out = []
    for key, loader in (("device", afdm.DeviceLoader(ds, 16)), ("host", DataLoader(TensorDataset(host_images, labels), 16, shuffle=True))):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        assert len(loader) == 3
        out.append(_train(afdm, dev, loader, wd))
    (la, sa), (lb, sb) = out
    assert len(la) == 1 and math.isfinite(la[0]) and la == lb
    assert set(sa) == set(sb) and all(torch.equal(_bits(sa[k]), _bits(sb[k])) for k in sa)


def test_ddpm_run_with_the_device_loader_is_the_host_run(A, tmp_path, monkeypatch):
    """ddpm_run on an MNIST-shaped csv with and without params["device_loader"]: the same losses, checkpoint and bits per dim (scored
    on dataset.batch(arange(N)) in the device run); the settings file gains the key and nothing else."""
    import os
    import numpy as np
    afdm, dev = A
    rng = np.random.default_rng(0)
    arr = np.concatenate([rng.integers(0, 10, (16, 1)), rng.integers(0, 256, (16, 784))], axis=1)
    runs = {}
    for key in ("host", "device"):
        wd = tmp_path / key
        wd.mkdir()
        np.savetxt(wd / "mnist.csv", arr, fmt="%d", delimiter=",", header=",".join(["label"] + [f"p{i}" for i in range(784)]), comments="")
        monkeypatch.chdir(wd)
        params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1,
                  "device": "cuda", "lr": 3e-4, "noise_steps": 6, "image_gen_per_epoch": 1, "dataset_dir": "mnist.csv",
                  "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
                  "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42, "eval_bpd": 4}
        if key == "device":
            params["device_loader"] = True
        out = afdm.ddpm_run(params)
        settings = open(os.path.join("runs", "DDPM_Uncondtional_MNIST_3", "settings_MNIST_3.txt")).read().replace(str(wd), "")
        runs[key] = (out, torch.load(out["modelpath"], weights_only=True), settings)
    (ho, hs, ht), (do, dsd, dt) = runs["host"], runs["device"]
    assert ho["loss_all"] == do["loss_all"] and math.isfinite(do["loss_all"][0]) and ho["bpd"] == do["bpd"]
    assert all(torch.equal(_bits(hs[k]), _bits(dsd[k])) for k in hs)
    assert torch.equal(ho["sample"].cpu(), do["sample"].cpu())
    assert dt == ht + "\ndevice_loader: True"
    monkeypatch.chdir(tmp_path / "host")
    with pytest.raises(ValueError, match="flip_prob needs device_loader"):
        afdm.tasks._loader("MNIST", afdm.argument(), {"flip_prob": 0.5})
