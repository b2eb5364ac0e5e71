"""Host-side data / image I/O of the reference's `modules/utils.py`, without torchvision
(SURVEY.md section 8f-1).  Not on the timed path.
DeviceDataset / DeviceLoader keep a training set in device memory and assemble its batches there."""
import math
import os
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Dataset, TensorDataset

IMG_EXT = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def get_data_MNIST(args):
    """CSV loader (utils.py:55-82): column 0 = label, 784 pixel columns; resize 28 -> 32 (bilinear,
    antialiased like torchvision's tensor Resize), normalise to [-1, 1]."""
    import pandas as pd
    data = pd.read_csv(args.dataset_path)
    labels = torch.tensor(data.iloc[:, 0].values, dtype=torch.long)
    feats = torch.tensor(data.iloc[:, 1:].values / 255.0, dtype=torch.float32).view(-1, 1, 28, 28)
    feats = F.interpolate(feats, size=(32, 32), mode="bilinear", antialias=True, align_corners=False)
    feats = (feats - 0.5) / 0.5
    dataset = TensorDataset(feats, labels)
    return DataLoader(dataset, batch_size=args.batch_size, shuffle=True), dataset


class ImageFolder(Dataset):
    """root/<class>/<image> like torchvision.datasets.ImageFolder (utils.py:43-52): RGB, shorter side
    resized to `size` (bilinear), scaled to [0,1], normalised with mean = std = 0.5."""

    def __init__(self, root, size):
        self.size = size
        classes = sorted(d.name for d in os.scandir(root) if d.is_dir())
        if not classes:
            raise FileNotFoundError(f"Couldn't find any class folder in {root}.")
        self.class_to_idx = {c: i for i, c in enumerate(classes)}
        self.samples = []
        for c in classes:
            for dirpath, _, files in sorted(os.walk(os.path.join(root, c))):
                for f in sorted(files):
                    if f.lower().endswith(IMG_EXT):
                        self.samples.append((os.path.join(dirpath, f), self.class_to_idx[c]))

    def __len__(self):
        return len(self.samples)

    def load_uint8(self, i):
        """Image i, opened and resized: (3, h, w) uint8."""
        from PIL import Image
        path = self.samples[i][0]
        img = Image.open(path).convert("RGB")
        w, h = img.size
        s = self.size
        if w <= h:
            nw, nh = s, max(1, int(s * h / w))
        else:
            nw, nh = max(1, int(s * w / h)), s
        img = img.resize((nw, nh), Image.BILINEAR)
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1)

    def __getitem__(self, i):
        x = self.load_uint8(i).float() / 255.0
        return (x - 0.5) / 0.5, self.samples[i][1]


def get_data(args):
    dataset = ImageFolder(args.dataset_path, args.image_size)
    return DataLoader(dataset, batch_size=args.batch_size, shuffle=True), dataset


INT64_MIN = -2 ** 63      # the label of a row whose index lies outside the store (never ops.NULL_LABEL)


def _per_channel(v, C, name):
    """A scalar or a length-C sequence / tensor -> C Python floats."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().reshape(-1).tolist()
    elif isinstance(v, np.ndarray):
        v = v.reshape(-1).tolist()
    vals = [v] * C if isinstance(v, (int, float)) and not isinstance(v, bool) else v
    try:
        vals = [float(a) for a in vals]
    except (TypeError, ValueError):
        vals = None
    if vals is None or len(vals) != C or not all(math.isfinite(a) for a in vals):
        raise ValueError(f"DeviceDataset: {name} must be a finite number or {C} of them, one per channel (got {v!r})")
    return vals


def normalisation_table(C, mean=0.5, std=0.5):
    """(C, 256) fp32, table[c][u] = the float the host loader makes of pixel value u in channel c, by its own expression on the
    CPU (ImageFolder.__getitem__: `x.float() / 255.0`, then `(x - mean) / std`), so a lookup returns the loader's bits."""
    mean, std = _per_channel(mean, C, "mean"), _per_channel(std, C, "std")
    if any(s == 0.0 for s in std):
        raise ValueError(f"DeviceDataset: std must not contain 0 (got {std!r})")
    u = torch.arange(256, dtype=torch.uint8).float() / 255.0
    return torch.stack([(u - m) / s for m, s in zip(mean, std)])


class DeviceDataset:
    """A whole image data set in device memory, batches assembled there by one launch (ops.batch_gather: afd_batch_gather_u8 /
    afd_batch_gather_f32).

    images: (N, C, H, W) uint8 pixels, normalised on the way out through `table` = normalisation_table(C, mean, std) -- bit for
    bit what ImageFolder.__getitem__ returns for those pixels -- or float32 values that are handed out as they are (mean and std
    are then unused).  labels: None or (N,) int64.  `.images`, `.labels`, `.table` live on `device`.
    device="cpu" runs `batch` as plain torch indexing: the same values, and the oracle of the kernels' tests.
    `nearest` / `self_nearest` search the store for the nearest images of a set of queries; on
    device="cpu" they are a plain torch brute force, the oracle of that kernel's tests.
    `power_spectrum` is the mean power spectrum of the store's images.
    `feature_stats` is the mean and covariance of an extractor's features of the store's images, for FID."""

    def __init__(self, images, labels=None, mean=0.5, std=0.5, device="cuda", classes=None):
        if isinstance(images, np.ndarray):
            images = torch.from_numpy(images)
        if not isinstance(images, torch.Tensor) or images.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"DeviceDataset: images must be a uint8 or float32 tensor (got {getattr(images, 'dtype', type(images).__name__)})")
        if images.dim() != 4 or images.numel() == 0:
            raise ValueError(f"DeviceDataset: images must be a non-empty 4-D (N, C, H, W) store (got shape {tuple(images.shape)})")
        N, C = images.shape[:2]
        if labels is not None:
            if isinstance(labels, np.ndarray):
                labels = torch.from_numpy(labels)
            if not isinstance(labels, torch.Tensor) or labels.dtype != torch.long or tuple(labels.shape) != (N,):
                raise ValueError(f"DeviceDataset: labels must be None or an int64 tensor of shape ({N},) (got "
                                 f"{getattr(labels, 'dtype', type(labels).__name__)}, shape {tuple(getattr(labels, 'shape', ()))})")
        self.device = torch.device(device)
        self.table = normalisation_table(C, mean, std).to(self.device) if images.dtype == torch.uint8 else None
        self.images = images.detach().to(self.device).contiguous()
        self.labels = None if labels is None else labels.detach().to(self.device).contiguous()
        self.classes = None if classes is None else list(classes)

    def __len__(self):
        return self.images.shape[0]

    def batch(self, idx, flip=None):
        """idx: (B,) int64 indices (repeats allowed); flip: None or (B,) bool / uint8, rows to mirror left-right.
        -> (x (B, C, H, W) float32, y (B,) int64 or None without labels), fresh tensors on the store's device.  A row whose
        index lies outside [0, N) is all NaN and its label INT64_MIN."""
        if not isinstance(idx, torch.Tensor) or idx.dtype != torch.long or idx.dim() != 1 or idx.numel() == 0:
            raise ValueError(f"DeviceDataset.batch: idx must be a non-empty 1-D int64 tensor (got "
                             f"{getattr(idx, 'dtype', type(idx).__name__)}, shape {tuple(getattr(idx, 'shape', ()))})")
        if flip is not None:
            if not isinstance(flip, torch.Tensor) or flip.dtype not in (torch.bool, torch.uint8) or tuple(flip.shape) != tuple(idx.shape):
                raise ValueError(f"DeviceDataset.batch: flip must be None or a bool / uint8 tensor of shape {tuple(idx.shape)}")
            flip = flip.to(self.device)
            flip = flip.view(torch.uint8) if flip.dtype == torch.bool else flip
        idx = idx.to(self.device)
        if self.device.type == "cpu":
            return self._batch_torch(idx, flip)
        from . import ops
        with torch.cuda.device(self.device):
            return ops.batch_gather(self.images, idx.contiguous(), None if flip is None else flip.contiguous(), self.table, self.labels)

    def _batch_torch(self, idx, flip):
        N, C = self.images.shape[:2]
        bad = (idx < 0) | (idx >= N)
        safe = idx.clamp(0, N - 1)
        x = self.images[safe]
        if self.table is not None:
            x = self.table[torch.arange(C, device=x.device).view(1, C, 1, 1), x.long()]
        if flip is not None:
            rows = flip != 0
            x[rows] = x[rows].flip(-1)
        x[bad] = float("nan")
        if self.labels is None:
            return x, None
        y = self.labels[safe]
        y[bad] = INT64_MIN
        return x, y

    def nearest(self, queries, k=1, exclude=None):
        """For each query image the k images of the store of smallest squared L2 distance, ascending, ties to the lower index
        (ops.nn_search: afd_nn_search_u8 / afd_nn_search_f32).  queries: (n, C, H, W) of the store's
        dtype -- raw pixels for a uint8 store, values on the store's scale for a float32 one; exclude: None or (n,) int64, query q
        skips image exclude[q] (negative: nothing).  -> (dist (n, k), idx (n, k) int64) on the store's device: dist is the exact
        sum of squared pixel differences as int64 (uint8), or the fp64 sum rounded once to float32, a NaN distance reported as
        the canonical NaN and ranked last (float32).  A slot with no image left has idx -1 and dist -1 / +inf."""
        what = "DeviceDataset.nearest"
        if isinstance(queries, np.ndarray):
            queries = torch.from_numpy(queries)
        if not isinstance(queries, torch.Tensor) or queries.dtype != self.images.dtype:
            raise ValueError(f"{what}: queries must be a tensor of the store's dtype {self.images.dtype} (got "
                             f"{getattr(queries, 'dtype', type(queries).__name__)})")
        if queries.dim() != 4 or tuple(queries.shape[1:]) != tuple(self.images.shape[1:]):
            raise ValueError(f"{what}: queries must have the shape (n, {', '.join(str(s) for s in self.images.shape[1:])}) "
                             f"(got {tuple(queries.shape)})")
        n = queries.shape[0]
        if n < 1:
            raise ValueError(f"{what}: queries must hold at least one image (n >= 1)")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= 16:
            raise ValueError(f"{what}: k must be an int in [1, 16] (got {k!r})")
        if exclude is not None and (not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.long or tuple(exclude.shape) != (n,)):
            raise ValueError(f"{what}: exclude must be None or an int64 tensor of shape ({n},)")
        if self.images.dtype == torch.uint8 and self.images[0].numel() > 32768:
            raise ValueError(f"{what}: a uint8 image holds at most 32768 elements (C H W = {self.images[0].numel()})")
        queries = queries.detach().to(self.device).contiguous()
        exclude = None if exclude is None else exclude.to(self.device).contiguous()
        if self.device.type == "cpu":
            return self._nearest_torch(queries, int(k), exclude)
        from . import ops
        with torch.cuda.device(self.device):
            return ops.nn_search(self.images, queries, int(k), exclude)

    def self_nearest(self, k=1, batch=1024):
        """Leave-one-out: nearest(images, k, exclude = own index) over the whole store, `batch` queries at a time.  The
        distribution that the distances of generated samples are read against."""
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"DeviceDataset.self_nearest: batch must be an integer >= 1 (got {batch!r})")
        own = torch.arange(len(self), device=self.device)
        parts = [self.nearest(self.images[a:a + batch], k, own[a:a + batch]) for a in range(0, len(self), int(batch))]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def power_spectrum(self, window="hann", remove_mean=True, n=None):
        """The mean power spectrum of the first n images of the store (None: all of them), read through the store's own table:
        spectrum.power_spectrum's dict (afd_power_spectrum_u8 / _f32 on the device, plain torch on device="cpu"; DESIGN.md
        section 6p)."""
        from .spectrum import power_spectrum
        if n is not None and (isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= len(self)):
            raise ValueError(f"DeviceDataset.power_spectrum: n must be None or an int in [1, {len(self)}] (got {n!r})")
        return power_spectrum(self.images if n is None else self.images[:int(n)], self.table, window, remove_mean)

    def pixels(self, n=None):
        """The first n images of the store (None: all) as uint8 pixels: a uint8 store's own bytes; a float32 store's values mapped
        back from [-1, 1], (x clamped + 1) * 127.5 rounded to the nearest pixel value."""
        if n is not None and (isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= len(self)):
            raise ValueError(f"DeviceDataset.pixels: n must be None or an int in [1, {len(self)}] (got {n!r})")
        x = self.images if n is None else self.images[:int(n)]
        return x if x.dtype == torch.uint8 else ((x.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8)

    def feature_stats(self, extractor, n=None, batch=256):
        """fidelity.FeatureStats of the features `extractor` makes of the first n images of the store (None: all), read as
        pixels(n), `batch` images at a time (fidelity.extract_features; afd_feature_moments_f32 on the device, plain torch on
        device="cpu").  Its state() can be saved and reused as a training set's reference statistics."""
        from .fidelity import FeatureStats, extract_features, load_extractor
        images, extractor = self.pixels(n), load_extractor(extractor, self.device)
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"DeviceDataset.feature_stats: batch must be an integer >= 1 (got {batch!r})")
        stats = None
        for a in range(0, images.shape[0], int(batch)):
            f = extract_features(extractor, images[a:a + int(batch)], int(batch))[0]
            stats = FeatureStats(f.shape[1], self.device) if stats is None else stats
            stats.update(f)
        return stats

    def _nearest_torch(self, queries, k, exclude):
        """Brute force in plain torch: int64 sums of squared differences (uint8) or fp64 sums rounded once to float32, then a stable
        sort by distance (NaN last), so equal distances keep their index order."""
        N, n = len(self), queries.shape[0]
        u8 = self.images.dtype == torch.uint8
        data = self.images.reshape(N, -1)
        data = data.to(torch.int16) if u8 else data.double()
        q = queries.reshape(n, -1)
        q = q.to(torch.int16) if u8 else q.double()
        d = torch.empty(n, N, dtype=torch.long if u8 else torch.float32, device=data.device)
        step = max(1, (1 << 24) // max(1, data.numel()))
        for a in range(0, n, step):
            diff = data[None] - q[a:a + step, None]
            if u8:
                diff = diff.to(torch.int32)
                d[a:a + step] = (diff * diff).sum(-1, dtype=torch.long)
            else:
                d[a:a + step] = (diff * diff).sum(-1).float()
        if not u8:
            d[torch.isnan(d)] = float("nan")                       # the canonical quiet NaN
        order = torch.sort(d, dim=1, stable=True)[1]
        if exclude is not None:                                    # the excluded row goes behind every candidate, order kept
            out = order == exclude.view(n, 1)
            order = order.gather(1, torch.sort(out.to(torch.uint8), dim=1, stable=True)[1])
            avail = N - out.sum(1)
        else:
            avail = torch.full((n,), N, device=d.device)
        idx = torch.full((n, k), -1, dtype=torch.long, device=d.device)
        dist = torch.full((n, k), -1 if u8 else float("inf"), dtype=d.dtype, device=d.device)
        m = min(k, N)
        keep = torch.arange(m, device=d.device).view(1, m) < avail.view(n, 1)
        idx[:, :m] = torch.where(keep, order[:, :m], idx[:, :m])
        dist[:, :m] = torch.where(keep, d.gather(1, order[:, :m]), dist[:, :m])
        return dist, idx

    @classmethod
    def from_folder(cls, root, size, cache=None, device="cuda", mean=0.5, std=0.5):
        """root/<class>/<image>, walked and resized by ImageFolder itself, stored as uint8.  Raises ValueError with the
        offending path if the resized shapes differ (the host loader could not collate those either).
        cache: the path of one .npz (images, labels, the class list) written here and read by later calls; it is rebuilt when
        `size` or the list of files differs (a walk that finds no image at all takes the cache as it is)."""
        try:
            folder = ImageFolder(root, size)
        except (FileNotFoundError, NotADirectoryError):
            folder = None                      # (the images may be gone once the cache holds them)
        files = [] if folder is None else [os.path.relpath(p, root) for p, _ in folder.samples]
        if cache is not None and os.path.exists(cache):
            with np.load(cache, allow_pickle=False) as z:
                if int(z["size"]) == int(size) and (not files or z["files"].tolist() == files):
                    return cls(torch.from_numpy(z["images"]), torch.from_numpy(z["labels"]), mean, std, device, z["classes"].tolist())
        if not files:
            raise FileNotFoundError(f"DeviceDataset.from_folder: no image found under {root}" +
                                    ("" if cache is None else f", and {cache} holds no cache for size {size}"))
        images = None
        for k in range(len(folder)):
            u8 = folder.load_uint8(k)
            if images is None:
                images = torch.empty((len(folder),) + tuple(u8.shape), dtype=torch.uint8)
            if tuple(u8.shape) != tuple(images.shape[1:]):
                raise ValueError(f"DeviceDataset.from_folder: {folder.samples[k][0]} resizes to {tuple(u8.shape)}, the images before "
                                 f"it to {tuple(images.shape[1:])}: one store (and one collated batch) needs one shape")
            images[k] = u8
        labels = torch.tensor([lab for _, lab in folder.samples], dtype=torch.long)
        classes = sorted(folder.class_to_idx, key=folder.class_to_idx.get)
        if cache is not None:
            os.makedirs(os.path.dirname(os.path.abspath(cache)), exist_ok=True)
            tmp = f"{cache}.tmp.npz"
            np.savez(tmp, images=images.numpy(), labels=labels.numpy(), classes=np.array(classes, dtype=np.str_),
                     files=np.array(files, dtype=np.str_), size=np.int64(size))
            os.replace(tmp, cache)
        return cls(images, labels, mean, std, device, classes)

    @classmethod
    def from_tensor_dataset(cls, ds, device="cuda"):
        """A TensorDataset of (float32 images, int64 labels), which is what get_data_MNIST builds: stored as fp32, so a batch
        holds the host path's values by construction."""
        if not isinstance(ds, TensorDataset) or len(ds.tensors) != 2:
            raise ValueError("DeviceDataset.from_tensor_dataset: ds must be a TensorDataset of (images, labels)")
        return cls(ds.tensors[0], ds.tensors[1], device=device)


class _EpochIndices(Dataset):
    """What the index-only DataLoader iterates: item i is i."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


class DeviceLoader:
    """Iterates a DeviceDataset in batches assembled on the device: `for images, labels in loader`, one gather launch per batch,
    every batch a fresh tensor.  The order is torch's own: at the start of an epoch an index-only
    DataLoader(range(N), batch_size, shuffle, drop_last) runs to its end, so the batches -- and the use of torch's global CPU
    generator -- are those of DataLoader(dataset, batch_size, shuffle) on the host; the epoch's indices go to the device in one
    copy and each batch's index is a view of that buffer.
    flip_prob > 0: each row is mirrored left-right with that probability; the epoch's bits come from a generator of the
    loader's own (seed), never from the global one, and travel with the indices.  flip_prob = 0 draws nothing."""

    def __init__(self, dataset, batch_size, shuffle=True, drop_last=False, flip_prob=0.0, seed=None):
        if not isinstance(dataset, DeviceDataset):
            raise ValueError(f"DeviceLoader: dataset must be a DeviceDataset (got {type(dataset).__name__})")
        if isinstance(batch_size, bool) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError(f"DeviceLoader: batch_size must be an integer >= 1 (got {batch_size!r})")
        if isinstance(flip_prob, bool) or not isinstance(flip_prob, (int, float)) or not 0.0 <= flip_prob <= 1.0:
            raise ValueError(f"DeviceLoader: flip_prob must lie in [0, 1] (got {flip_prob!r})")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer))):
            raise ValueError(f"DeviceLoader: seed must be an integer or None (got {seed!r})")
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.shuffle, self.drop_last, self.flip_prob = bool(shuffle), bool(drop_last), float(flip_prob)
        self._order = DataLoader(_EpochIndices(len(dataset)), batch_size=self.batch_size, shuffle=self.shuffle, drop_last=self.drop_last)
        self._gen = torch.Generator()
        if seed is None:
            self._gen.seed()
        else:
            self._gen.manual_seed(int(seed))

    def __len__(self):
        return len(self._order)

    def epoch_plan(self):
        """-> (the epoch's index batches as one (n,) int64 CPU tensor in batch order, its (n,) uint8 flip bits or None).
        Advances the global generator as one epoch of the host DataLoader does, and the loader's own by the flip draw."""
        batches = list(self._order)
        idx = torch.cat(batches) if batches else torch.empty(0, dtype=torch.long)
        flip = None
        if self.flip_prob > 0.0:
            flip = (torch.rand(idx.numel(), generator=self._gen) < self.flip_prob).view(torch.uint8)
        return idx, flip

    def __iter__(self):
        idx, flip = self.epoch_plan()
        dev = self.dataset.device
        idx = idx.to(dev)
        flip = None if flip is None else flip.to(dev)
        for a in range(0, idx.numel(), self.batch_size):
            b = min(a + self.batch_size, idx.numel())
            yield self.dataset.batch(idx[a:b], None if flip is None else flip[a:b])


def get_data_device(args, cache=None, flip_prob=0.0, seed=None):
    """get_data with the data set in device memory: (DeviceLoader, DeviceDataset)."""
    dataset = DeviceDataset.from_folder(args.dataset_path, args.image_size, cache=cache, device=args.device)
    return DeviceLoader(dataset, args.batch_size, shuffle=True, flip_prob=flip_prob, seed=seed), dataset


def get_data_MNIST_device(args, flip_prob=0.0, seed=None):
    """get_data_MNIST with the data set in device memory: (DeviceLoader, DeviceDataset)."""
    dataset = DeviceDataset.from_tensor_dataset(get_data_MNIST(args)[1], device=args.device)
    return DeviceLoader(dataset, args.batch_size, shuffle=True, flip_prob=flip_prob, seed=seed), dataset


def _to_pil(img):
    """uint8 / float (C,H,W) or (H,W) tensor -> PIL image (torchvision ToPILImage semantics)."""
    from PIL import Image
    t = img.detach().cpu()
    if t.dtype != torch.uint8:
        t = (t * 255).to(torch.uint8)          # ToPILImage: float in [0,1] -> mul(255).byte()
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() == 2:
        return Image.fromarray(t.numpy(), mode="L")
    return Image.fromarray(t.permute(1, 2, 0).numpy())


def save_gen_images(path_str, data, fileno):
    """`<path>/image_<n>.png`, one file per generated image (utils.py:175-198)."""
    save_dir = Path(path_str)
    save_dir.mkdir(parents=True, exist_ok=True)
    for i in range(data.shape[0]):
        _to_pil(data[i]).save(save_dir / f"image_{fileno[i]}.png", format="PNG")


def save_dataset_MNIST(path_str, dataset):
    save_dir = Path(path_str)
    save_dir.mkdir(parents=True, exist_ok=True)
    for i, (image, _) in enumerate(dataset):
        _to_pil(image).save(save_dir / f"image_{i}.png", format="PNG")


def make_collage(filedir, savedir, images_per_collage, total_image, image_size):
    """sqrt(n) x sqrt(n) RGB collages `<savedir>_collage_<start>.png` (utils.py:208-234)."""
    from PIL import Image
    per = int(math.sqrt(images_per_collage))
    side = int(image_size * math.sqrt(images_per_collage))
    for start in np.arange(0, total_image, images_per_collage):
        files = [f"{filedir}/image_{i}.png" for i in np.arange(start, start + images_per_collage, 1)]
        images = [Image.open(f).resize((image_size, image_size)) for f in files]
        collage = Image.new("RGB", (side, side))
        for i in range(per):
            for j in range(per):
                collage.paste(images[i * per + j], (i * image_size, j * image_size))
        collage.save(savedir + f"_collage_{start}.png")
