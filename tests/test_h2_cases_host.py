"""The inputs of tests/test_gpu_h2_scales.py are fair: on every one of them torch's plain CPU fp32 convolution / matrix product
passes the gates that the GPU tests put on the f16x2 kernels (rel-L2 < 1e-5 against fp64 per slice that owns a scale).  So a
gate missed on the device is the kernel's fault, not the input's.  What was narrowed is said in tests/h2_cases.py: PAIR_DY
for fp32's own sake (the gradient tensor's scopes differ by 2^12, not 2^30, because 1e-30 * 2^-30 is an fp32 subnormal), and
PW_OPP_LO / HI for the documented limit of csrc/h2_common.h (fp32 passes that one at the full span too)."""
import pytest
import torch

import h2_cases as H

_ids = lambda s: "x".join(str(v) for v in s)


def test_builders():
    x = torch.ones(5, 96, 4, 4)
    a = H.k_ramp(x, "ascending")
    assert torch.allclose(a[0, ::32, 0, 0], torch.tensor([1e-6, 10 ** -1.5, 1e3])) and torch.equal(H.k_ramp(x, "flat"), x)
    assert torch.equal(H.k_ramp(a, "descending")[:, 32:64], a[:, 32:64] * 10 ** -1.5)
    assert torch.equal(H.k_ramp(x[:, :32], "ascending"), x[:, :32])                  # one chunk: nothing to ramp over
    p = H.pair_scale(x, (-30, 0, 30))
    assert [float(p[b, 0, 0, 0]) for b in range(5)] == [2.0 ** -30, 2.0 ** -30, 1.0, 1.0, 2.0 ** 30]     # B odd: half a pair
    assert [float(v) for v in H.pair_scale(x, (-30, 0, 30), group=1)[:, 0, 0, 0]] == [2.0 ** -30, 1.0, 2.0 ** 30, 2.0 ** -30, 1.0]
    s = H.stream_ramp(torch.ones(2, 1, 32, 32), "ascending", -12, 12, bands=8)
    assert float(s[0, 0, 0, 0]) == 2.0 ** -12 and float(s[1, 0, 31, 0]) == 2.0 ** 12 and float(s[0, 0, 4, 0]) == 2.0 ** -10
    assert torch.equal(s, H.stream_ramp(torch.ones(2, 1, 32, 32), "descending", -12, 12, bands=8).flip(0, 2))
    st = H.stream_ramp(torch.ones(8, 1, 4, 4), "step", 0, 12, at=5)
    assert [float(v) for v in st[:, 0, 0, 0]] == [1.0] * 5 + [4096.0] * 3
    z = H.zero_chunk(torch.ones(1, 64, 2, 2))
    assert not z[:, :32].any() and z[:, 32:].all()
    assert H.rel(torch.zeros(3), torch.zeros(3)) == 0.0 and H.rel(torch.tensor([0.0, 1e-40]), torch.zeros(2)) == float("inf")
    assert H.per_block(torch.ones(64, 64, 3, 3), torch.ones(64, 64, 3, 3))[0] == 0.0


def test_steps_fall_inside_a_split():
    """every 3x3 weight-gradient shape: 16 tiles of 128 pixels, the step's first unit inside tile 6 = the third tile of split 1"""
    for S, B in H.WG_SHAPES:
        assert B * S * S == 16 * 128
        unit_px = S * S // H.wg_bands(S)
        tile, off = divmod(H.wg_step_unit(S) * unit_px, 128)
        assert tile == 6 and (off > 0 or unit_px >= 128)
    for shape in H.PW_SHAPES:
        K, N, S, B = shape
        b, c, p = H.pw_spike_at(*shape)
        assert (b * S * S + p) // 32 == B * S * S // 32 - 1 and c < min(K, N)


@pytest.mark.parametrize("shape", H.ALL_CONV_SHAPES, ids=_ids)
def test_conv_inputs_pass_in_fp32(shape):
    for tag, x, w, dy in H.conv_inputs(shape):
        assert torch.isfinite(x).all() and torch.isfinite(dy).all()
        y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
        y32, dx32 = H.conv_ref(x, w, dy, torch.float32)
        ey, ed = H.per_image(y32, y64), H.per_image(dx32, dx64)
        assert ey[0] < H.TOL and ed[0] < H.TOL, (shape, tag, ey, ed)
    for tag, x, w, dy, zi in H.conv_zero_inputs(shape):
        y64, dx64 = H.conv_ref(x, w, dy, torch.float64)
        y32, dx32 = H.conv_ref(x, w, dy, torch.float32)
        assert torch.isfinite(y32).all() and torch.isfinite(dx32).all()
        assert not y32[zi].any() and not dx32[zi].any()
        assert H.per_image(y32, y64)[0] < H.TOL and H.per_image(dx32, dx64)[0] < H.TOL, (shape, tag)


@pytest.mark.parametrize("which", H.WG_SETS)
@pytest.mark.parametrize("S,B", H.WG_SHAPES, ids=lambda v: str(v))
def test_wgrad_inputs_pass_in_fp32(S, B, which):
    x, dy = H.wg_inputs(S, B, which)
    e = H.per_block(H.wgrad3_ref(x, dy, torch.float32), H.wgrad3_ref(x, dy, torch.float64))
    assert e[0] < H.TOL, (S, B, which, e)


@pytest.mark.parametrize("which", H.PW_SETS)
@pytest.mark.parametrize("shape", H.PW_SHAPES, ids=_ids)
def test_pointwise_wgrad_inputs_pass_in_fp32(shape, which):
    x, dy = H.pw_inputs(shape, which)
    (dw32, db32), (dw64, db64) = H.pw_ref(x, dy, torch.float32), H.pw_ref(x, dy, torch.float64)
    e = H.per_block(dw32, dw64)
    assert e[0] < H.TOL and H.rel(db32, db64) < H.TOL_BIAS, (shape, which, e, H.rel(db32, db64))
    if "spike" in which:
        assert H.rel(H.pw_rest(which, shape, dw32), H.pw_rest(which, shape, dw64)) < H.TOL
