"""Writes shift.npz: scipy.ndimage.shift(x, (0, 0, v, h), mode='grid-wrap') (order 3) of a seeded fp32 batch for a few
fractional (v, h), the reference of Diffusion.shift_2d_matrix's device path.  Run: python tests/golden/make_shift_golden.py"""
import os

import numpy as np
from scipy import ndimage

SHIFTS = [(0.5, 0.25), (-1.75, 3.0), (0.0, 0.125), (2.5, -0.5), (-0.3, -7.9)]      # (v, h): negative, > 1, one axis whole

if __name__ == "__main__":
    rng = np.random.default_rng(20)
    x = rng.standard_normal((2, 3, 32, 32)).astype(np.float32)
    out = np.stack([ndimage.shift(x, (0, 0, v, h), mode="grid-wrap") for v, h in SHIFTS])
    assert out.dtype == np.float32
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "shift.npz"), x=x,
                        shifts=np.asarray(SHIFTS, dtype=np.float64), out=out)
