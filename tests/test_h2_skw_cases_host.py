"""The inputs of tests/test_gpu_h2_skw.py are fair: on its shapes torch's plain CPU fp32 convolution passes the gates that the
GPU test puts on the slice-walking split-K kernel (rel-L2 <= 1e-5 against fp64 per image, exact zeros on all-zero scopes), as
tests/test_h2_cases_host.py shows for the shapes of tests/test_gpu_h2_scales.py."""
import pytest
import torch

import h2_cases as H

SHAPES = [(4, 256, 64, 13), (4, 128, 96, 9), (4, 64, 64, 9)]      # tests/test_gpu_h2_skw.py
_ids = lambda s: "x".join(str(v) for v in s)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_skw_conv_inputs_pass_in_fp32(shape):
    for tag, x, w, dy in H.conv_inputs(shape):
        assert torch.isfinite(x).all() and torch.isfinite(dy).all()
        y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
        y32, dx32 = H.conv_ref(x, w, dy, torch.float32)
        ey, ed = H.per_image(y32, y64), H.per_image(dx32, dx64)
        assert ey[0] <= H.TOL and ed[0] <= H.TOL, (shape, tag, ey, ed)
    for tag, x, w, dy, zi in H.conv_zero_inputs(shape):
        y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
        y32, dx32 = H.conv_ref(x, w, dy, torch.float32)
        assert torch.isfinite(y32).all() and torch.isfinite(dx32).all()
        assert not y32[zi].any() and not dx32[zi].any()
        assert H.per_image(y32, y64)[0] <= H.TOL and H.per_image(dx32, dx64)[0] <= H.TOL, (shape, tag)
