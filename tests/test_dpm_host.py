"""CPU-side tests of DPM-Solver++(2M) sampling: the log-SNR timestep rule and its argument checks, the per-step coefficient
table against an fp64 restatement (bit for bit, order policy included), the sampler's argument checks, and the C ABI of the
two new entry points with their argument checks (which return before any device is touched)."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def _diff(T=1000):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu")


def _lam(ah, t):
    a = float(ah[t])
    return math.log(math.sqrt(a)) - math.log(math.sqrt(1.0 - a))


def test_logsnr_timesteps_at_the_default_schedule():
    d = _diff()
    assert d.logsnr_timesteps(10) == [999, 891, 769, 623, 444, 241, 95, 32, 8, 1]
    assert d.logsnr_timesteps(20) == [999, 949, 897, 842, 782, 718, 648, 571, 485, 391, 293, 203, 131, 81, 48, 28, 15, 8, 3, 1]
    assert d.logsnr_timesteps(1) == [999]
    assert d.logsnr_timesteps(2) == [999, 1]
    assert d.logsnr_timesteps(999) == list(range(999, 0, -1))


def _nearest(ah, T, S, k):
    """The definition's r_k before the two passes: argmin over t in [1, T-1] of |lam(t) - L_k|, the first (smallest t) on a tie."""
    lam = [_lam(ah, t) for t in range(T)]
    L = lam[T - 1] + (k / (S - 1)) * (lam[1] - lam[T - 1])
    return min(range(1, T), key=lambda t: (abs(lam[t] - L), t))


@pytest.mark.parametrize("S", [1, 2, 3, 14, 15, 50, 500, 998, 999])
def test_logsnr_timesteps_invariants(S):
    d = _diff()
    T = 1000
    r = d.logsnr_timesteps(S)
    assert len(r) == S and r[0] == T - 1 and r[-1] == (T - 1 if S == 1 else 1)
    assert all(isinstance(v, int) for v in r)
    assert all(a > b for a, b in zip(r, r[1:]))
    assert all(1 <= v <= T - 1 for v in r)
    if 3 <= S <= 50:                                           # the definition, restated per k with a plain argmin
        ah = d.alpha_hat
        want = [T - 1] + [_nearest(ah, T, S, k) for k in range(1, S - 1)] + [1]
        for k in range(S - 2, -1, -1):
            want[k] = max(want[k], want[k + 1] + 1)
        want = [min(v, T - 1 - k) for k, v in enumerate(want)]
        assert r == want


def test_logsnr_timesteps_on_other_schedules():
    for T in (2, 3, 10, 100, 1001):
        d = _diff(T)
        for S in sorted({1, 2, 3, T // 2, T - 2, T - 1}):
            if not 1 <= S <= T - 1:
                continue
            r = d.logsnr_timesteps(S)
            assert len(r) == S and r[0] == T - 1 and r[-1] == (T - 1 if S == 1 else 1)
            assert all(a > b for a, b in zip(r, r[1:]))
        assert d.logsnr_timesteps(T - 1) == list(range(T - 1, 0, -1))


def test_logsnr_timesteps_argument_errors():
    d = _diff()
    for bad in (0, -3, 1000, 5000, 2.0, True, "50", None):
        with pytest.raises(ValueError):
            d.logsnr_timesteps(bad)
    r3 = d.logsnr_timesteps(3)
    assert d.dpmpp_pairs(3) == list(zip(r3, r3[1:] + [0])) and r3[0] == 999 and r3[-1] == 1
    assert d.dpmpp_pairs([999, 500, 1]) == [(999, 500), (500, 1), (1, 0)]
    for bad in ([], [999, 999, 1], [5, 10], [1000, 1], [999, 0], [999, 2.5], [True], "abc", 3.5, 0, 1000):
        with pytest.raises(ValueError):
            d.dpmpp_pairs(bad)


def _coef_restated(ah, pairs):
    """The issue's definition, fp64 throughout, rounded once per value to fp32."""
    alpha = lambda t: math.sqrt(float(ah[t]))
    sigma = lambda t: math.sqrt(1.0 - float(ah[t]))
    lam = lambda t: math.log(alpha(t)) - math.log(sigma(t))
    S = len(pairs)
    hs = [lam(tp) - lam(t) for t, tp in pairs]
    rows = []
    for k, (t, tp) in enumerate(pairs):
        B = -alpha(tp) * math.expm1(-hs[k])
        if k == 0 or (k == S - 1 and S < 15):
            b0, b1 = B, 0.0
        else:
            r = hs[k - 1] / hs[k]
            b0, b1 = B * (1 + 1 / (2 * r)), -B / (2 * r)
        rows.append([np.float32(v) for v in (alpha(t), sigma(t), sigma(tp) / sigma(t), b0, b1)])
    return torch.tensor(np.array(rows, dtype=np.float32))


@pytest.mark.parametrize("steps", [1, 2, 3, 10, 14, 15, 20, 50, [999, 500, 20, 3]])
def test_coefficient_table_matches_the_fp64_definition_bit_for_bit(steps):
    d = _diff()
    pairs = d.dpmpp_pairs(steps)
    got = d.dpmpp_coefficients(pairs)
    want = _coef_restated(d.alpha_hat, pairs)
    S = len(pairs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, 5)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # the order policy: first order at k = 0, and at the last step when S < 15; B1 = 0 exactly there and only there
    first = [k for k in range(S) if float(got[k, 4]) == 0.0]
    assert first == ([0, S - 1] if 1 < S < 15 else [0])
    assert [d.dpmpp_order(k, S) for k in range(S)] == [1 if k in first else 2 for k in range(S)]
    # an order-1 row is DDIM with eta = 0: B0 = alpha(tp) - sigma(tp) alpha(t) / sigma(t)
    t, tp = pairs[0]
    a_t, a_p = float(d.alpha_hat[t]), float(d.alpha_hat[tp])
    assert math.isclose(float(got[0, 3]), math.sqrt(a_p) - math.sqrt(1 - a_p) * math.sqrt(a_t) / math.sqrt(1 - a_t),
                        rel_tol=1e-6, abs_tol=1e-7)


def test_header_declares_and_types_the_dpmpp_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_dpmpp_step"] == (I, [P, P, P, P, P, P, L, P])
    assert sigs["afd_dpmpp_step_cfg"] == (I, [P, P, P, P, F, P, P, P, L, P])


def test_dpmpp_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    with pytest.raises(afdm.AfdError, match="afd_dpmpp_step: .*NULL"):
        lib.afd_dpmpp_step(None, None, None, None, None, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_dpmpp_step_cfg: .*NULL"):
        lib.afd_dpmpp_step_cfg(None, None, None, None, 3.0, None, None, None, 8, None)
    # non-NULL but never dereferenced: each check returns before a launch
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    at = lambda i: base + 4 * i                               # element i of the buffer
    x, e, c, o, o2, x0, xp = at(0), at(16), at(48), at(64), at(80), at(96), at(112)
    for q in (x, e, c, o, x0):                                # each required pointer in turn
        args = [x, e, None, c, o, x0]
        args[[x, e, None, c, o, x0].index(q)] = None
        with pytest.raises(afdm.AfdError, match="afd_dpmpp_step: .*NULL"):
            lib.afd_dpmpp_step(*args, 8, None)
    for n in (0, -4):
        with pytest.raises(afdm.AfdError, match="afd_dpmpp_step: n must be positive"):
            lib.afd_dpmpp_step(x, e, xp, c, o, x0, n, None)
        with pytest.raises(afdm.AfdError, match="afd_dpmpp_step_cfg: n must be positive"):
            lib.afd_dpmpp_step_cfg(x, e, xp, c, 3.0, o, o2, x0, n, None)
    n = 8
    # x0_out overlapping x, eps, x_out, or part of x0_prev
    for bad in (x, at(4), e, at(20), o, at(60), at(108)):
        with pytest.raises(afdm.AfdError, match="afd_dpmpp_step: x0_out must not overlap"):
            lib.afd_dpmpp_step(x, e, xp, c, o, bad, n, None)
    # eps2 of the guided form holds 2n values: x0_out inside its second half overlaps it; x_out2 too
    for bad in (at(16 + n + 2), at(80), at(84)):
        with pytest.raises(afdm.AfdError, match="afd_dpmpp_step_cfg: x0_out must not overlap"):
            lib.afd_dpmpp_step_cfg(x, e, xp, c, 3.0, o, o2, bad, n, None)
    with pytest.raises(afdm.AfdError, match="afd_dpmpp_step_cfg: x0_out must not overlap"):
        lib.afd_dpmpp_step_cfg(x, e, xp, c, 3.0, o, o2, at(116), n, None)         # part of x0_prev


def test_public_signatures_take_a_sampler():
    import afdm
    D = afdm.Diffusion
    for fn in (D.sample, D.revert):
        sp = inspect.signature(fn).parameters
        assert sp["sampler"].default is None and list(sp)[-1] == "sampler"
    for fn in (D.sample_concurrent, D.sample_sharded, D.sample_shift, D.sample_rotation_sweep, D.inpaint):
        assert "sampler" not in inspect.signature(fn).parameters


def test_dpmpp_requests_that_are_refused_before_touching_a_device():
    import afdm
    d = _diff()
    m = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    with pytest.raises(ValueError, match="unknown sampler"):
        d.sample(m, n=2, image_channels=1, steps=10, sampler="dpm")
    with pytest.raises(ValueError, match="unknown sampler"):
        d.revert(m, n=2, image_channels=1, steps=10, sampler=2)
    with pytest.raises(ValueError, match="needs steps"):
        d.sample(m, n=2, image_channels=1, sampler="dpmpp_2m")
    with pytest.raises(ValueError, match="eta"):
        d.sample(m, n=2, image_channels=1, steps=10, eta=0.5, sampler="dpmpp_2m")
    with pytest.raises(NotImplementedError, match="theta"):
        d.sample(m, n=2, image_channels=1, theta=30, steps=10, sampler="dpmpp_2m")
    with pytest.raises(ValueError):
        d.sample(m, n=2, image_channels=1, steps=1000, sampler="dpmpp_2m")
    with pytest.raises(ValueError):
        d.revert(m, n=1, image_channels=1, steps=[10, 20], sampler="dpmpp_2m")
    assert m.training and m._t_range is None
