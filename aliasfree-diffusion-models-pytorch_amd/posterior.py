"""Linear measurement operators for diffusion posterior sampling: one parametrised family
A x = m . S_s(k * x) that covers inpainting (a mask alone), deblurring (any kernel), super-resolution (an anti-alias kernel and
a stride) and their combinations, with its exact adjoint and a noisy measurement y = A x + sigma n.  `Diffusion.posterior_sample`
restores images from such a measurement (DPS, Chung et al. 2023).  On device tensors A and A^T are csrc/posterior.hip
(ops.linop_apply, ops.linop_adjoint); on cpu tensors they are plain torch fp64, F.conv2d and its transpose, the oracle of the
kernels' tests (autograd passes through them)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

MAX_KERNEL = 15
MAX_SIDE = 64
STRIDES = (1, 2, 4)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def gaussian_kernel(size, sigma):
    """The normalised (size, size) float32 Gaussian kernel g g^T, g_i = exp(-(i - (size - 1) / 2)^2 / (2 sigma^2)), built in fp64
    and rounded once; size odd in [1, 15], sigma > 0."""
    if not _is_int(size) or size < 1 or size > MAX_KERNEL or size % 2 == 0:
        raise ValueError(f"LinearOperator: a kernel's size must be an odd int in [1, {MAX_KERNEL}] (got {size!r})")
    if not _is_number(sigma) or not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"LinearOperator: a Gaussian kernel's sigma must be a finite number > 0 (got {sigma!r})")
    i = torch.arange(int(size), dtype=torch.float64) - (int(size) - 1) / 2
    g = torch.exp(-(i * i) / (2.0 * float(sigma) ** 2))
    g = g / g.sum()
    return torch.outer(g, g).float()


class LinearOperator:
    """A x = m . S_s(k * x), per channel, the same kernel and mask for every row of an (n, C, H, W) batch with H, W <= 64.

    kernel: None (the 1 x 1 delta) or a (K, K) float tensor, K odd, 1 <= K <= 15, applied as a correlation with zero padding
    K // 2: exactly F.conv2d(x, k, padding=K // 2, stride=s, groups=C).
    stride: s in {1, 2, 4}; H and W must be multiples of it and the measurement plane is h x w = H / s x W / s.
    mask: None or a float tensor of shape (1 | C, h, w), usually 0 / 1, applied at measurement resolution.
    `adjoint` is the exact adjoint: the transposed strided correlation of m . r.
    cpu tensors (float32 or float64) are computed, and returned, in fp64 by plain torch; device tensors must be float32 and go
    through the HIP kernels.  Every argument error is a ValueError that starts with "LinearOperator: "."""

    def __init__(self, kernel=None, stride=1, mask=None):
        if kernel is None:
            k = torch.ones(1, 1, dtype=torch.float32)
        else:
            if not isinstance(kernel, (torch.Tensor, np.ndarray)):
                raise ValueError(f"LinearOperator: kernel must be None or a (K, K) float tensor (got {type(kernel).__name__})")
            k = torch.as_tensor(kernel).detach().cpu()
            if not k.dtype.is_floating_point or k.dim() != 2 or k.shape[0] != k.shape[1]:
                raise ValueError(f"LinearOperator: kernel must be a square (K, K) float tensor (got {k.dtype}, shape {tuple(k.shape)})")
            K = int(k.shape[0])
            if K < 1 or K > MAX_KERNEL or K % 2 == 0:
                raise ValueError(f"LinearOperator: the kernel's side K must be odd with 1 <= K <= {MAX_KERNEL} (got {K})")
            if not bool(torch.isfinite(k).all()):
                raise ValueError("LinearOperator: every kernel value must be finite")
            k = k.float().contiguous()
        if not _is_int(stride) or int(stride) not in STRIDES:
            raise ValueError(f"LinearOperator: stride must be 1, 2 or 4 (got {stride!r})")
        if mask is not None:
            if not isinstance(mask, (torch.Tensor, np.ndarray)):
                raise ValueError(f"LinearOperator: mask must be None or a (1 | C, h, w) float tensor (got {type(mask).__name__})")
            m = torch.as_tensor(mask).detach().cpu()
            if not m.dtype.is_floating_point or m.dim() != 3 or m.numel() == 0:
                raise ValueError(f"LinearOperator: mask must be a non-empty (1 | C, h, w) float tensor (got {m.dtype}, shape {tuple(m.shape)})")
            if not bool(torch.isfinite(m).all()):
                raise ValueError("LinearOperator: every mask value must be finite")
            mask = m.float().contiguous()
        self.kernel, self.stride, self.mask = k, int(stride), mask
        self.K = int(k.shape[0])
        self._taps = np.ascontiguousarray(k.numpy())              # the kernels take the taps as launch arguments: no H2D copy
        self._mask_dev = {}

    def __repr__(self):
        return (f"LinearOperator(K={self.K}, stride={self.stride}, "
                f"mask={None if self.mask is None else tuple(self.mask.shape)})")

    # ---- the named members of the family ------------------------------------------------------------------------------------------
    @classmethod
    def inpainting(cls, mask):
        """Keep the pixels where `mask` is 1: mask (H, W) or (1 | C, H, W), the delta kernel, stride 1."""
        if isinstance(mask, (torch.Tensor, np.ndarray)):
            mask = torch.as_tensor(mask)
            if mask.dim() == 2:
                mask = mask.unsqueeze(0)
            if not mask.dtype.is_floating_point and not mask.dtype.is_complex:
                mask = mask.float()
        if mask is None:
            raise ValueError("LinearOperator: inpainting needs a mask")
        return cls(None, 1, mask)

    @classmethod
    def gaussian_blur(cls, size, sigma):
        """Blur with `gaussian_kernel(size, sigma)`, stride 1."""
        return cls(gaussian_kernel(size, sigma), 1, None)

    @classmethod
    def super_resolution(cls, factor, size=None, sigma=None):
        """Decimate by `factor` (1, 2 or 4) behind a Gaussian anti-alias kernel.  Defaults: size = 2 factor + 1 taps and
        sigma = factor / 2 (at factor 4: 9 taps, sigma 2; about the width of one measurement pixel)."""
        if not _is_int(factor) or int(factor) not in STRIDES:
            raise ValueError(f"LinearOperator: factor must be 1, 2 or 4 (got {factor!r})")
        size = 2 * int(factor) + 1 if size is None else size
        sigma = int(factor) / 2.0 if sigma is None else sigma
        return cls(gaussian_kernel(size, sigma), int(factor), None)

    @classmethod
    def motion_blur(cls, kernel):
        """Blur with any normalised (K, K) kernel (its values must add up to 1 within 1e-4), stride 1."""
        op = cls(kernel, 1, None)
        if kernel is None or abs(float(op.kernel.double().sum()) - 1.0) > 1e-4:
            raise ValueError("LinearOperator: motion_blur needs a normalised kernel (its values must add up to 1)")
        return op

    # ---- shapes ---------------------------------------------------------------------------------------------------------------------
    def _mask_for(self, C, h, w):
        m = self.mask
        if m is not None and (m.shape[0] not in (1, C) or tuple(m.shape[1:]) != (h, w)):
            raise ValueError(f"LinearOperator: the mask of shape {tuple(m.shape)} does not fit the measurement plane: expected "
                             f"(1 | {C}, {h}, {w})")
        return m

    def _check(self, name, v):
        if not isinstance(v, torch.Tensor) or v.dim() != 4 or v.numel() == 0:
            raise ValueError(f"LinearOperator: {name} must be a non-empty (n, C, H, W) tensor")
        if v.dtype != torch.float32 and not (v.device.type == "cpu" and v.dtype == torch.float64):
            raise ValueError(f"LinearOperator: {name} must be float32 (on the cpu float64 as well; got {v.dtype})")

    def measurement_shape(self, shape):
        """(n, C, H, W) -> (n, C, H / s, W / s), after checking the sizes."""
        n, C, H, W = (int(v) for v in shape)
        s = self.stride
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f"LinearOperator: H and W must lie in [1, {MAX_SIDE}] (got {H}, {W})")
        if H % s or W % s:
            raise ValueError(f"LinearOperator: H and W must be multiples of the stride {s} (got {H}, {W})")
        return n, C, H // s, W // s

    def image_shape(self, shape):
        """(n, C, h, w) -> (n, C, h s, w s), after checking the sizes."""
        n, C, h, w = (int(v) for v in shape)
        s = self.stride
        if not (1 <= h * s <= MAX_SIDE and 1 <= w * s <= MAX_SIDE):
            raise ValueError(f"LinearOperator: H = h s and W = w s must lie in [1, {MAX_SIDE}] (got a measurement of {h} x {w} at stride {s})")
        return n, C, h * s, w * s

    def _device_mask(self, device):
        if self.mask is None:
            return None
        key = str(device)
        if key not in self._mask_dev:
            self._mask_dev[key] = self.mask.to(device).contiguous()
        return self._mask_dev[key]

    # ---- A, A^T and the measurement -------------------------------------------------------------------------------------------------
    def apply(self, x):
        """A x: (n, C, H, W) -> (n, C, H / s, W / s)."""
        self._check("x", x)
        _, C, h, w = self.measurement_shape(x.shape)
        m = self._mask_for(C, h, w)
        if x.device.type == "cpu":
            k = self.kernel.double().expand(C, 1, self.K, self.K)
            y = F.conv2d(x.double(), k, padding=self.K // 2, stride=self.stride, groups=C)
            return y if m is None else y * m.double()
        from . import ops
        with torch.cuda.device(x.device):
            return ops.linop_apply(x, self._taps, self.stride, self._device_mask(x.device))

    def adjoint(self, r):
        """A^T r: (n, C, h, w) -> (n, C, h s, w s)."""
        self._check("r", r)
        _, C, H, W = self.image_shape(r.shape)
        m = self._mask_for(C, r.shape[2], r.shape[3])
        if r.device.type == "cpu":
            k = self.kernel.double().expand(C, 1, self.K, self.K)
            r = r.double() if m is None else r.double() * m.double()
            return F.conv_transpose2d(r, k, padding=self.K // 2, stride=self.stride, output_padding=self.stride - 1, groups=C)
        from . import ops
        with torch.cuda.device(r.device):
            return ops.linop_adjoint(r, self._taps, self.stride, self._device_mask(r.device))

    def measure(self, x, sigma=0.0, generator=None):
        """y = A x + sigma n, n standard normal drawn from `generator` (default: the global generator of x's device) in y's dtype."""
        if not _is_number(sigma) or not (sigma >= 0 and math.isfinite(sigma)):
            raise ValueError(f"LinearOperator: sigma must be a finite number >= 0 (got {sigma!r})")
        y = self.apply(x)
        if sigma == 0:
            return y
        if generator is None:
            noise = torch.randn(y.shape, device=y.device, dtype=y.dtype)
        else:
            noise = torch.randn(y.shape, generator=generator, device=generator.device, dtype=y.dtype).to(y.device)
        return y + float(sigma) * noise
