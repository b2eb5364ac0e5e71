"""Power spectra of image sets: the mean |DFT|^2 of a set of images per channel, in fp64, and its radial
average, for setting the spectrum of generated images against that of the training set.  On a device tensor the work is two
launches of csrc/spectrum.hip (ops.power_spectrum); on a cpu tensor it is plain torch (torch.fft.rfft2 in fp64), the oracle of
the kernels' tests."""
import functools
import math

import numpy as np
import torch

MAX_SIDE = 64
WINDOWS = ("hann", None)


def hann_window(N):
    """(N,) fp64, w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / N): the half-sample Hann window, symmetric about the middle of the axis and
    nowhere 0 (N = 1 gives 1)."""
    if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or N < 1:
        raise ValueError(f"hann_window: N must be an int >= 1 (got {N!r})")
    j = torch.arange(int(N), dtype=torch.float64)
    return 0.5 - 0.5 * torch.cos(2.0 * math.pi * (j + 0.5) / int(N))


def mirror_weights(W):
    """(W // 2 + 1,) fp64, m(v): 1 on the columns of an rfft2 layout that are their own mirror image (v = 0, and v = W / 2 for an
    even W), 2 on the others, which stand for two coefficients of the full spectrum."""
    m = torch.full((W // 2 + 1,), 2.0, dtype=torch.float64)
    m[0] = 1.0
    if W % 2 == 0:
        m[W // 2] = 1.0
    return m


def spectrum_bins(H, W):
    """-> (bins (H, W // 2 + 1) int32, counts (R,) fp64, R).  With M = min(H, W) and fu, fv the signed frequency indices of a
    coefficient, rho = sqrt((fu M / H)^2 + (fv M / W)^2) is its radius in cycles per M pixels and bins = floor(rho + 0.5);
    R = M // 2 + 1, and a coefficient beyond the shorter axis' Nyquist (bin >= R) gets -1 and is left out.  counts[r] = the sum
    of m(v) over the bin: the number of coefficients of the full spectrum in it."""
    for name, N in (("H", H), ("W", W)):
        if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or N < 1:
            raise ValueError(f"spectrum_bins: {name} must be an int >= 1 (got {N!r})")
    H, W = int(H), int(W)
    M = min(H, W)
    R = M // 2 + 1
    u = torch.arange(H, dtype=torch.float64)
    fu = torch.where(u <= H // 2, u, u - H)
    fv = torch.arange(W // 2 + 1, dtype=torch.float64)
    rho = torch.sqrt((fu * M / H).view(H, 1) ** 2 + (fv * M / W).view(1, -1) ** 2)
    r = torch.floor(rho + 0.5).to(torch.int32)
    bins = torch.where(r < R, r, torch.full_like(r, -1))
    counts = torch.zeros(R, dtype=torch.float64)
    keep = bins >= 0
    counts.index_add_(0, bins[keep].long(), mirror_weights(W).view(1, -1).expand(H, -1)[keep])
    return bins, counts, R


def _windows(window, H, W):
    if window not in WINDOWS:
        raise ValueError(f"power_spectrum: window must be 'hann' or None (got {window!r})")
    return (None, None) if window is None else (hann_window(H), hann_window(W))


@functools.lru_cache(maxsize=64)
def _constants(H, W, window, device):
    """(win_h, win_w, bins, counts, R) of a plane shape on `device`, built once: they are read, never written."""
    win_h, win_w = _windows(window, H, W)
    bins, counts, R = spectrum_bins(H, W)
    to = lambda t: None if t is None else t.to(device)      # noqa: E731
    return to(win_h), to(win_w), to(bins), to(counts), R


def _power_torch(images, table, win_h, win_w, remove_mean, chunk=4096):
    """The oracle: the sum over the images of |rfft2|^2 in fp64, a chunk of images at a time, divided by n once."""
    n, C = images.shape[:2]
    total = None
    for a in range(0, n, chunk):
        x = images[a:a + chunk]
        if table is not None:
            x = table[torch.arange(C, device=x.device).view(1, C, 1, 1), x.long()]
        x = x.double()
        if remove_mean:
            x = x - x.mean(dim=(-2, -1), keepdim=True)
        if win_h is not None:
            x = x * (win_h.view(-1, 1) * win_w.view(1, -1))
        f = torch.fft.rfft2(x)
        p = (f.real * f.real + f.imag * f.imag).sum(0)
        total = p if total is None else total + p
    return total / n


def power_spectrum(images, table=None, window="hann", remove_mean=True):
    """images: (n, C, H, W), H and W at most 64, uint8 pixels read through table (C, 256) fp32 (None: normalisation_table(C)) or
    float32 values taken as they are.  Each plane loses its own mean (remove_mean), is multiplied by the separable half-sample
    Hann window (window="hann"; None: no window) and transformed, all in fp64.
    -> {"power": (C, H, W // 2 + 1) the mean |F|^2 over the images in rfft2 layout, "radial": (C, R) its mean over the
    coefficients of each bin of spectrum_bins(H, W), the mirrored half counted, "counts": (R,), "n"}, fp64 tensors on the images'
    device."""
    what = "power_spectrum"
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(images)
    if not isinstance(images, torch.Tensor) or images.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: images must be a uint8 or float32 tensor (got {getattr(images, 'dtype', type(images).__name__)})")
    if images.dim() != 4 or images.numel() == 0:
        raise ValueError(f"{what}: images must be a non-empty 4-D (n, C, H, W) set (got shape {tuple(images.shape)})")
    n, C, H, W = images.shape
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: H and W must lie in [1, {MAX_SIDE}] (got {H}, {W})")
    _windows(window, H, W)
    dev = images.device
    win_h, win_w, bins, counts, R = _constants(H, W, window, dev)
    if images.dtype == torch.uint8:
        if table is None:
            from .data import normalisation_table
            table = normalisation_table(C)
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or tuple(table.shape) != (C, 256):
            raise ValueError(f"{what}: table must be a float32 tensor of shape ({C}, 256)")
        table = table.to(dev).contiguous()
    elif table is not None:
        raise ValueError(f"{what}: table goes with uint8 images only (float32 images are taken as they are)")
    images = images.detach().contiguous()
    if dev.type == "cpu":
        power = _power_torch(images, table, win_h, win_w, bool(remove_mean))
        keep = bins >= 0
        radial = torch.zeros(C, R, dtype=torch.float64)
        radial.index_add_(1, bins[keep].long(), (power * mirror_weights(W))[:, keep])
    else:
        from . import ops
        with torch.cuda.device(dev):
            power, radial = ops.power_spectrum(images, table, win_h, win_w, bool(remove_mean), bins, R)
    return {"power": power, "radial": radial / counts, "counts": counts.clone(), "n": int(n)}


def compare_spectra(ref, gen):
    """ref, gen: two results of power_spectrum over planes of one shape.  -> (db, lsd, hf_ratio):
    db (C, R) = 10 log10(gen.radial / ref.radial), nan where ref is 0;
    lsd = the root mean square of db over all channels and the bins r >= 1 (the log-spectral distance in dB; nan bins skipped);
    hf_ratio = gen's share of its radial energy (radial * counts, r = 0 left out) in the bins r > (R - 1) / 2, over ref's share:
    above 1 the generated set holds more of its energy in the upper half of the band than the reference does."""
    rr, gr = ref["radial"].double().cpu(), gen["radial"].double().cpu()
    counts = ref["counts"].double().cpu()
    if rr.shape != gr.shape or rr.dim() != 2 or tuple(counts.shape) != (rr.shape[1],) or not torch.equal(counts, gen["counts"].double().cpu()):
        raise ValueError(f"compare_spectra: ref and gen must come from planes of one shape (got radial {tuple(rr.shape)} and {tuple(gr.shape)})")
    R = rr.shape[1]
    db = 10.0 * torch.log10(gr / rr)
    db = torch.where(rr == 0, torch.full_like(db, float("nan")), db)
    tail = db[:, 1:]
    ok = ~torch.isnan(tail)
    lsd = float(torch.sqrt((tail[ok] ** 2).mean())) if bool(ok.any()) else float("nan")
    r = torch.arange(R)
    high, band = (r > (R - 1) / 2) & (r >= 1), r >= 1

    def share(radial):
        e = radial * counts
        return float(e[:, high].sum() / e[:, band].sum()) if bool(band.any()) else float("nan")

    ref_share = share(rr)
    hf_ratio = share(gr) / ref_share if ref_share != 0 else float("nan")
    return db, lsd, hf_ratio
