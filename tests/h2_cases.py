"""Inputs that make the running power-of-two scales of the f16x2 kernels MOVE (csrc/h2_common.h; csrc/h2.hip, h2_wgrad.hip),
shared by tests/test_gpu_h2_scales.py (the kernels against fp64) and tests/test_h2_cases_host.py (torch's CPU fp32 against
fp64 on the same inputs under the same gates: the inputs are fair, a gate missed on the device is the kernel's).

With randn inputs every chunk of every operand has the same magnitude: a scale is set once and never changes, every wave
ends with the same one, and a slip in the carry-over, in the unscaling of per-wave partial sums or in the scale an epilogue
divides by cannot be seen.  The builders here follow the kernels' geometry instead:

  k_ramp       the 32-channel chunks of the reduction axis differ by nine decades (a workgroup's / wave's scale is lowered
               chunk after chunk, or is set by the first chunk and the later ones are small); under split-K wave kw takes
               chunks kw, kw + KSP, ..: every wave of a workgroup ends with another scale.
  pair_scale   whole scale scopes differ by powers of two: image PAIRS where a tile or slice holds two images (two 4 x 4
               images per 32-pixel slice of conv_h2_sk, two 8 x 8 images per 128-pixel tile), single images where a tile is an
               image or less (16 x 16, 32 x 32).
  stream_ramp  for the weight gradients, whose scales run over the batch: the stream units (images, or the 128-pixel row
               bands of a larger image) rise or fall by powers of two, or jump by 2^hi from one unit on ("step").
  zero_chunk, zero_images   all-zero blocks: the scale must stay at its cap until data arrives.

All functions are deterministic (seeded torch.Generator) and return new CPU fp32 tensors."""
import math

import torch
import torch.nn.functional as F

TOL = 1e-5                    # the project's contract (tests/test_gpu_ops.py)
TOL_BIAS = 5e-6               # bias gradients take unscaled values (test_linear_wgrad_full_batch_matches_double_precision)
RAMPS = ("ascending", "descending", "flat")
# (factor of x, factor of the gradient tensor): unit, and both ends of fp32's range, as test_conv_f16x2_online_scaling_dynamic_range
GLOBALS = ((1.0, 1e-9), (1e-25, 1e12), (1e18, 1e-30))
PAIR_X = (-30, 0, 30)
# the gradient tensor goes down to 1e-30: times 2^-30 it would be an fp32 subnormal and lose bits before any kernel sees it,
# so its scopes differ by 2^12 (NARROWED from 2^30: the span, not the structure)
PAIR_DY = (-12, 0, 12)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def k_ramp(x, kind):
    """The 32-channel chunks of x's channel axis times logspace(-6, 3) (ascending), logspace(3, -6) (descending) or 1 (flat).
    One chunk has nothing to ramp over and is left alone."""
    nch = x.shape[1] // 32
    assert x.shape[1] % 32 == 0 and kind in RAMPS
    if nch == 1 or kind == "flat":
        return x.clone()
    ramp = torch.logspace(-6, 3, nch) if kind == "ascending" else torch.logspace(3, -6, nch)
    return x * ramp.repeat_interleave(32)[None, :, None, None]


def pair_scale(t, exps, group=2):
    """Images group * j .. group * j + group - 1 times 2^exps[j mod len(exps)]."""
    e = torch.tensor([float(exps[(b // group) % len(exps)]) for b in range(t.shape[0])])
    return t * torch.exp2(e)[:, None, None, None]


def stream_ramp(t, kind, lo, hi, bands=1, at=None):
    """Stream unit u (image b = u // bands, row band u % bands of its H rows) times a power of two: rising from 2^lo to 2^hi
    over the units (ascending), falling from 2^hi to 2^lo (descending), or 1 before unit `at` and 2^hi from it on (step)."""
    B, C, H, W = t.shape
    n = B * bands
    assert H % bands == 0
    if kind == "ascending":
        e = torch.linspace(lo, hi, n).round()
    elif kind == "descending":
        e = torch.linspace(hi, lo, n).round()
    else:
        assert kind == "step" and at is not None and 0 < at < n
        e = torch.zeros(n)
        e[at:] = float(hi)
    f = torch.exp2(e).reshape(B, 1, bands, 1, 1)
    return (t.reshape(B, C, bands, H // bands, W) * f).reshape(B, C, H, W)


def zero_chunk(x, chunk=0):
    x = x.clone()
    x[:, 32 * chunk:32 * chunk + 32] = 0.0
    return x


def zero_images(t, images):
    t = t.clone()
    t[images] = 0.0
    return t


# ---- gates: rel-L2 per slice that owns a scale -----------------------------------------------------------------------------
def rel(a, ref):
    """rel-L2 in fp64 with no floor under the norm (slices here go down to 1e-34); an all-zero reference asks for zeros."""
    a, ref = a.double().flatten(), ref.double().flatten()
    n = float(ref.norm())
    if n == 0.0:
        return 0.0 if not bool(a.any()) else float("inf")
    return float((a - ref).norm()) / n


def per_image(a, ref):
    """worst image: (error, image)"""
    return max((rel(a[b], ref[b]), b) for b in range(ref.shape[0]))


def per_block(dw, ref, bn=32, bk=32):
    """worst bn x bk block (output x input channels, every tap) of a weight gradient: (error, (n0, k0))"""
    N, K = ref.shape[:2]
    return max((rel(dw[n:n + bn, k:k + bk], ref[n:n + bn, k:k + bk]), (n, k)) for n in range(0, N, bn) for k in range(0, K, bk))


# ---- 3x3 forward / dgrad ---------------------------------------------------------------------------------------------------
# (S, Cin, Cout, B): the smallest shapes that reach each form of the tile kernels (B odd where a tile holds two images: the last
# tile is half empty) ...
TILE_SHAPES = [(8, 96, 160, 5), (16, 128, 64, 3), (32, 64, 32, 2), (32, 64, 64, 2)]
TILE_SHAPE_N64 = (8, 64, 128, 5)          # ... an 8 x 8 layer whose BOTH channel counts are multiples of 64, for the (128 px, 2 blocks) form
# ... and of the split-K kernel: K = 64 -> 2 K-slices (x 2 pixel slices), K >= 128 -> 4; B odd: a half-empty last slice / workgroup
SK_SHAPES = [(4, 64, 96, 7), (4, 256, 64, 7), (8, 128, 32, 3), (8, 64, 64, 3)]
ALL_CONV_SHAPES = TILE_SHAPES + [TILE_SHAPE_N64] + SK_SHAPES


def scope_group(S):
    """images per scale scope of the forward / dgrad kernels: a pair on the 4 x 4 and 8 x 8 maps, one image above"""
    return 2 if S <= 8 else 1


def conv_base(shape):
    S, ci, co, B = shape
    g = gen(1000 * S + ci + co + B)
    w = torch.randn(co, ci, 3, 3, generator=g) / (3 * ci ** 0.5)
    return w, torch.randn(B, ci, S, S, generator=g), torch.randn(B, co, S, S, generator=g)


def conv_inputs(shape):
    """k_ramp x pair_scale x global factors: yields (tag, x, w, dy); x ramps over Cin (the forward's reduction axis), dy over
    Cout (the dgrad's)."""
    w, x0, dy0 = conv_base(shape)
    grp = scope_group(shape[0])
    for ramp in RAMPS:
        for gx, gd in GLOBALS:
            x = pair_scale(k_ramp(x0, ramp), PAIR_X, grp) * gx
            dy = pair_scale(k_ramp(dy0, ramp), PAIR_DY, grp) * gd
            yield (ramp, gx, gd), x, w, dy


def conv_zero_inputs(shape):
    """yields (tag, x, w, dy, zero images): a leading all-zero chunk under data near the top of fp32's range (the scale
    falls from its cap by ~2^170 when the second chunk arrives), and an all-zero scope beside live ones."""
    w, x0, dy0 = conv_base(shape)
    S, ci, co, B = shape
    zi = [0, 1] if B > 2 else [0]
    yield "leading zero chunk", zero_chunk(x0 * 1e18), w, zero_chunk(dy0 * 1e12), []
    yield "all-zero pair", zero_images(x0, zi), w, zero_images(dy0, zi), zi


def conv_ref(x, w, dy, dtype):
    """y = conv(x, w), dx = its gradient for dy, computed in `dtype` on the CPU"""
    xo = x.to(dtype).requires_grad_(True)
    y = F.conv2d(xo, w.to(dtype), padding=1)
    (dx,) = torch.autograd.grad(y, xo, dy.to(dtype))
    return y.detach(), dx


# ---- 3x3 weight gradients --------------------------------------------------------------------------------------------------
WG_C = 256                                                    # 256 -> 256: BN = BK = 32, 64 blocks, 16 tiles in 4 splits of 4
WG_SHAPES = [(32, 2), (16, 8), (8, 32), (4, 128)]             # (S, B): every one 16 tiles of 128 pixels
WG_SETS = ("x ascending", "x descending", "dy ascending", "dy descending", "opposed", "x step", "dy step")
WG_LO, WG_HI, WG_STEP = -12, 12, 12


def wg_bands(S):
    """stream units per image: the 128-pixel tile of wgrad_h2 is 8 rows of a 16 x 16 image and 4 rows of a 32 x 32 one -- a
    ramp per IMAGE would never change inside a split there (B = 2 at 32 x 32: a split is half an image)"""
    return max(1, S * S // 128)


def wg_step_unit(S):
    """the step's first unit: the middle of tile 6 (or tile 6, where a unit is a tile), the third tile of the second split"""
    upt = max(1, 128 // (S * S))                              # units per tile
    return 6 * upt + upt // 2


def wg_inputs(S, B, which):
    g = gen(S + B)
    x, dy = torch.randn(B, WG_C, S, S, generator=g), torch.randn(B, WG_C, S, S, generator=g)
    nb, at = wg_bands(S), wg_step_unit(S)
    ramp = lambda t, kind: stream_ramp(t, kind, WG_LO, WG_HI, nb)
    step = lambda t: stream_ramp(t, "step", 0, WG_STEP, nb, at)
    return {"x ascending": lambda: (ramp(x, "ascending"), dy), "x descending": lambda: (ramp(x, "descending"), dy),
            "dy ascending": lambda: (x, ramp(dy, "ascending")), "dy descending": lambda: (x, ramp(dy, "descending")),
            "opposed": lambda: (ramp(x, "ascending"), ramp(dy, "descending")),
            "x step": lambda: (step(x), dy), "dy step": lambda: (x, step(dy))}[which]()


def wgrad3_ref(x, dy, dtype):
    w = torch.zeros(dy.shape[1], x.shape[1], 3, 3, dtype=dtype, requires_grad=True)
    (dw,) = torch.autograd.grad(F.conv2d(x.to(dtype), w, padding=1), w, dy.to(dtype))
    return dw


# ---- 1x1 weight gradients --------------------------------------------------------------------------------------------------
# (K, N, S, B): NT = 3, four pixel slices; NT = 2, two slices; eight roles, one slice, two 4 x 4 images per step
PW_SHAPES = [(32, 96, 8, 8), (64, 64, 8, 8), (128, 384, 4, 16)]
PW_SETS = ("x ascending", "dy ascending", "opposed", "x spike", "dy spike")
PW_SPIKE = 2.0 ** 20
# "opposed" keeps every image's products level, so dY's LATE images count as much as the first while they sit under the scale
# the first one set; here ONE split walks the whole batch, and at the 2^24 of WG_LO .. WG_HI the late images would lie 2^24
# below their wave's maximum -- past the 2^17 to which csrc/h2_common.h keeps all bits (measured on MI355X at 2^24: worst block
# 1.3e-5 where the fp32 form has 1.6e-7, which is that limit's arithmetic: 2^-13 on the last image, 1 / sqrt(8) of the norm).
# NARROWED to 2^16 (the span, not the structure); the one-sided ramps keep 2^24.
PW_OPP_LO, PW_OPP_HI = -8, 8


def pw_spike_at(K, N, S, B):
    """(image, channel, pixel) of the spike: the last image, a pixel of the LAST 32-pixel step"""
    return B - 1, 5, S * S - 5


def pw_inputs(shape, which):
    K, N, S, B = shape
    g = gen(K + N + S + B)
    x, dy = torch.randn(B, K, S, S, generator=g), torch.randn(B, N, S, S, generator=g)
    if which == "x ascending":
        x = stream_ramp(x, "ascending", WG_LO, WG_HI)
    elif which == "dy ascending":
        dy = stream_ramp(dy, "ascending", WG_LO, WG_HI)
    elif which == "opposed":
        x, dy = stream_ramp(x, "ascending", PW_OPP_LO, PW_OPP_HI), stream_ramp(dy, "descending", PW_OPP_LO, PW_OPP_HI)
    else:
        b, c, p = pw_spike_at(*shape)
        t = (x if which == "x spike" else dy).clone()
        t.reshape(B, -1, S * S)[b, c, p] = PW_SPIKE * (1.0 + 0.25 * c / 8)        # (not a power of two)
        x, dy = (t, dy) if which == "x spike" else (x, t)
    return x, dy


def pw_ref(x, dy, dtype):
    B, K = x.shape[:2]
    N = dy.shape[1]
    dw = torch.einsum("bnp,bkp->nk", dy.to(dtype).reshape(B, N, -1), x.to(dtype).reshape(B, K, -1))
    return dw, dy.to(dtype).sum(dim=(0, 2, 3))


def pw_rest(which, shape, dw):
    """the weight gradient without the spike's column (x spike) or row (dy spike): the terms the lowered scale carried over"""
    c = pw_spike_at(*shape)[1]
    keep = [i for i in range(dw.shape[1 if which == "x spike" else 0]) if i != c]
    return dw[:, keep] if which == "x spike" else dw[keep]
