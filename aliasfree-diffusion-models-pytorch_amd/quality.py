"""PSNR and SSIM of image pairs: what inpainting and super-resolution report, an image against its ground
truth, over the whole image or over a region of it.  On device tensors the work is one launch of csrc/quality.hip
(ops.pair_quality); on cpu tensors it is plain torch fp64 with the same formula in the same operation order (its multiply-adds
unfused), the oracle of the kernel's tests.

The convention, stated rather than borrowed: a separable Gaussian window of 11 taps with sigma 1.5, normalised to sum 1; weighted
POPULATION variances and covariance (no n / (n - 1) factor); "valid" windows only, so (K - 1) / 2 pixels of border carry no window;
Wang et al. 2004's constants c1 = (0.01 L)^2 and c2 = (0.03 L)^2 with L the data range; SSIM of an image = the mean over its
windows and channels.  A region selects the pixels PSNR counts and, by their centre pixel, the windows SSIM counts.  skimage,
torchmetrics and pytorch_msssim are not available to this project's tests, so NOTHING here is tested for agreement with them, and
no parity is claimed."""
import math

import numpy as np
import torch

MAX_SIDE = 64
MAX_WINDOW = 15
_CHUNK = 1 << 21            # elements of one block of planes on the cpu path (five fp64 maps of it are alive at once)


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def gaussian_window(size=11, sigma=1.5):
    """(size,) fp64: exp(-(i - c)^2 / (2 sigma^2)) with c = (size - 1) / 2, divided by its sum (the sum rounded once, so the
    weights add up to 1 within an ulp), symmetric bit for bit.  size: an odd int in [1, 15]; sigma > 0, or None for the uniform
    window 1 / size."""
    if not _is_int(size) or not 1 <= size <= MAX_WINDOW or size % 2 == 0:
        raise ValueError(f"gaussian_window: size must be an odd int in [1, {MAX_WINDOW}] (got {size!r})")
    size = int(size)
    if sigma is None:
        return torch.full((size,), 1.0 / size, dtype=torch.float64)
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"gaussian_window: sigma must be a positive number or None (got {sigma!r})")
    c = (size - 1) / 2
    g = [math.exp(-((i - c) ** 2) / (2.0 * float(sigma) ** 2)) for i in range(size)]
    total = math.fsum(g)
    return torch.tensor([x / total for x in g], dtype=torch.float64)


def _window(what, window, sigma):
    if isinstance(window, torch.Tensor):
        if window.dtype != torch.float64 or window.dim() != 1 or not 1 <= window.shape[0] <= MAX_WINDOW or window.shape[0] % 2 == 0:
            raise ValueError(f"{what}: a window of weights must be a 1-D float64 tensor of an odd length in [1, {MAX_WINDOW}] (got "
                             f"{window.dtype}, shape {tuple(window.shape)})")
        return window.detach().cpu().contiguous()
    try:
        return gaussian_window(window, sigma)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None


def _images(what, a, b):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    if isinstance(b, np.ndarray):
        b = torch.from_numpy(b)
    for name, v in (("a", a), ("b", b)):
        if not isinstance(v, torch.Tensor) or v.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"{what}: {name} must be a uint8 or float32 tensor (got {getattr(v, 'dtype', type(v).__name__)})")
        if v.dim() != 4 or v.numel() == 0:
            raise ValueError(f"{what}: {name} must be a non-empty 4-D (n, C, H, W) set (got shape {tuple(v.shape)})")
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        raise ValueError(f"{what}: a and b must have the same shape, dtype and device (got {tuple(a.shape)} {a.dtype} {a.device} and "
                         f"{tuple(b.shape)} {b.dtype} {b.device})")
    H, W = a.shape[2:]
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: H and W must lie in [1, {MAX_SIDE}] (got {H}, {W})")
    return a.detach().contiguous(), b.detach().contiguous()


def _region(what, region, shape, device):
    """-> None, or the masks as a contiguous (1 | n, H, W) uint8 tensor on `device`."""
    if region is None:
        return None
    n, _, H, W = shape
    r = torch.as_tensor(region)
    try:
        full = torch.broadcast_shapes(tuple(r.shape), (n, 1, H, W))
    except RuntimeError:
        full = None
    if r.dtype.is_complex or full != (n, 1, H, W):
        raise ValueError(f"{what}: region of shape {tuple(r.shape)} does not broadcast to ({n}, 1, {H}, {W})")
    if not bool(((r == 0) | (r == 1)).all()):
        raise ValueError(f"{what}: region must hold 0 or 1")
    r = r.reshape((1,) * (4 - r.dim()) + tuple(r.shape))
    rows = r.shape[0]
    return r.expand(rows, 1, H, W).reshape(rows, H, W).to(torch.uint8).to(device).contiguous()


def _weighted(p, win, K):
    """The windows' weighted sums of the planes p (..., H, W): along the row first, then down the rows, taps in ascending order
    from the first product, as the kernel adds them."""
    Ho, Wo = p.shape[-2] - K + 1, p.shape[-1] - K + 1
    h = win[0] * p[..., :, 0:Wo]
    for s in range(1, K):
        h = h + win[s] * p[..., :, s:s + Wo]
    m = win[0] * h[..., 0:Ho, :]
    for r in range(1, K):
        m = m + win[r] * h[..., r:r + Ho, :]
    return m


def _pair_sums_torch(a, b, win, c1, c2, region, want_map):
    n, C, H, W = a.shape
    K = win.shape[0]
    Ho, Wo, half = H - K + 1, W - K + 1, (K - 1) // 2
    win = win.to(a.device)
    out = torch.empty(n, C, 5, dtype=torch.float64, device=a.device)
    ssim_map = torch.empty(n, C, Ho, Wo, dtype=torch.float64, device=a.device) if want_map else None
    step = max(1, _CHUNK // (C * H * W))
    for lo in range(0, n, step):
        x, y = a[lo:lo + step].double(), b[lo:lo + step].double()
        rows = x.shape[0]
        if region is None:
            inside = torch.ones(1, 1, H, W, dtype=torch.bool, device=a.device)
        else:
            inside = (region if region.shape[0] == 1 else region[lo:lo + step]).unsqueeze(1) != 0
        centre = inside[..., half:half + Ho, half:half + Wo]
        d = x - y
        zero = torch.zeros((), dtype=torch.float64, device=a.device)
        out[lo:lo + step, :, 0] = torch.where(inside, d * d, zero).sum((-2, -1))
        out[lo:lo + step, :, 1] = torch.where(inside, d.abs(), zero).sum((-2, -1))
        out[lo:lo + step, :, 2] = inside.sum((-2, -1)).to(torch.float64).expand(rows, C)
        ma, mb, maa, mbb, mab = _weighted(torch.stack([x, y, x * x, y * y, x * y]), win, K)
        vaa, vbb, vab = maa - ma * ma, mbb - mb * mb, mab - ma * mb
        ssim = ((2.0 * ma * mb + c1) * (2.0 * vab + c2)) / ((ma * ma + mb * mb + c1) * (vaa + vbb + c2))
        out[lo:lo + step, :, 3] = torch.where(centre, ssim, zero).sum((-2, -1))
        out[lo:lo + step, :, 4] = centre.sum((-2, -1)).to(torch.float64).expand(rows, C)
        if want_map:
            ssim_map[lo:lo + step] = ssim
    return out, ssim_map


def pair_sums(a, b, win, c1, c2, region=None, want_map=False):
    """The five sums per plane behind image_quality -> (out (n, C, 5) fp64, ssim_map (n, C, H - K + 1, W - K + 1) fp64 or None):
    out[i][c] = [the sum of (a - b)^2 and of |a - b| over the region's pixels, their number, the sum of SSIM over the windows
    whose centre pixel lies in the region, their number].  a, b: (n, C, H, W) uint8 or float32, alike; win: the (K,) fp64 window;
    region: None or what image_quality takes.  One launch of afd_pair_quality_u8 / _f32 on a device, plain torch on the cpu."""
    what = "pair_sums"
    a, b = _images(what, a, b)
    win = _window(what, win, None)
    if win.shape[0] > min(a.shape[2:]):
        raise ValueError(f"{what}: the window of {win.shape[0]} taps is larger than min(H, W) = {min(a.shape[2:])}")
    region = _region(what, region, a.shape, a.device)
    if a.device.type == "cpu":
        return _pair_sums_torch(a, b, win, float(c1), float(c2), region, bool(want_map))
    from . import ops
    with torch.cuda.device(a.device):
        return ops.pair_quality(a, b, win, float(c1), float(c2), region, bool(want_map))


def image_quality(a, b, data_range=None, window=11, sigma=1.5, k1=0.01, k2=0.03, region=None, return_map=False):
    """PSNR and SSIM of the images a against the images b, both (n, C, H, W) of one shape, dtype (uint8 or float32) and device,
    H and W at most 64, everything in fp64.
    data_range L: 255 for uint8 and 2.0 for float32 (the project's [-1, 1] scale) unless given; c1 = (k1 L)^2, c2 = (k2 L)^2.
    window: the size of the Gaussian window (gaussian_window(window, sigma); sigma None: uniform), or a 1-D float64 tensor of an
    odd number (at most 15) of weights; at most min(H, W) taps.  region: None, or an array of 0 / 1 that broadcasts to
    (n, 1, H, W): PSNR counts the pixels where it is 1, SSIM the windows whose centre pixel is one of them.
    -> a dict of fp64 tensors on the inputs' device:
        mse, mae (n,)        the squared and the absolute error summed over the channels / the pixels counted
        psnr (n,)            10 log10(L^2 / mse): +inf where mse == 0, NaN where the image's region is empty
        ssim (n,)            the windows' SSIM summed over the channels / the windows counted (NaN where there are none)
        ssim_channels (n, C) the same per channel
        pixels, windows (n,) the pixels and the windows counted, over all channels
        ssim_map (n, C, H - K + 1, W - K + 1)    with return_map: every window's SSIM, whatever the region is
    A NaN or an infinity in a plane propagates to its image's results; nothing is clamped.  The convention is the module's
    docstring's; no parity with any library is claimed."""
    what = "image_quality"
    a, b = _images(what, a, b)
    win = _window(what, window, sigma)
    if win.shape[0] > min(a.shape[2:]):
        raise ValueError(f"{what}: the window of {win.shape[0]} taps is larger than min(H, W) = {min(a.shape[2:])}")
    L = (255.0 if a.dtype == torch.uint8 else 2.0) if data_range is None else data_range
    if isinstance(L, bool) or not isinstance(L, (int, float, np.integer, np.floating)) or not (L > 0 and math.isfinite(L)):
        raise ValueError(f"{what}: data_range must be a positive number (got {data_range!r})")
    L = float(L)
    for name, k in (("k1", k1), ("k2", k2)):
        if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not (k >= 0 and math.isfinite(k)):
            raise ValueError(f"{what}: {name} must be a non-negative number (got {k!r})")
    out, ssim_map = pair_sums(a, b, win, (float(k1) * L) ** 2, (float(k2) * L) ** 2, region, return_map)
    sse, sae, pix, ssum, wins = out.unbind(-1)
    pixels, windows = pix.sum(1), wins.sum(1)
    mse = sse.sum(1) / pixels
    res = {"mse": mse, "mae": sae.sum(1) / pixels, "psnr": 10.0 * torch.log10(L * L / mse), "ssim": ssum.sum(1) / windows,
           "ssim_channels": ssum / wins, "pixels": pixels, "windows": windows}
    if return_map:
        res["ssim_map"] = ssim_map
    return res


def psnr(a, b, **kw):
    """image_quality(a, b, **kw)["psnr"]: (n,) fp64."""
    return image_quality(a, b, **kw)["psnr"]


def ssim(a, b, **kw):
    """image_quality(a, b, **kw)["ssim"]: (n,) fp64."""
    return image_quality(a, b, **kw)["ssim"]
