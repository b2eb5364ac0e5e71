"""CPU-side tests of DDIM sampling over strided timesteps: the timestep subsequence and its argument checks, the snapshot rule,
the C ABI of the four new entry points and their argument checks (which return before any device is touched)."""
import ctypes
import inspect
import math

import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def _diff(T):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu")


def test_ddim_timesteps_formula():
    d = _diff(1000)
    assert d.ddim_timesteps(999) == list(range(999, 0, -1))             # S = T - 1: the DDPM chain's own indices
    assert d.ddim_timesteps(1) == [999]
    assert d.ddim_timesteps(2) == [999, 1]
    assert d.ddim_timesteps(7) == [999, 832, 666, 500, 333, 167, 1]
    for T in (2, 3, 10, 100, 1000, 1001):
        d = _diff(T)
        for S in sorted({1, 2, 3, 7, 50, T // 2, T - 2, T - 1}):
            if not 1 <= S <= T - 1:
                continue
            taus = d.ddim_timesteps(S)
            assert len(taus) == S and taus[0] == T - 1 and all(a > b for a, b in zip(taus, taus[1:]))
            if S > 1:
                assert taus[-1] == 1 and taus == [1 + (k * (T - 2)) // (S - 1) for k in range(S)][::-1]
            assert all(isinstance(v, int) for v in taus)


def test_ddim_argument_errors():
    d = _diff(1000)
    for bad in (0, -3, 1000, 5000, 2.0, True, "50", None):
        with pytest.raises(ValueError):
            d.ddim_timesteps(bad)
    assert d._ddim_pairs([999, 500, 1], 0.0) == [(999, 500), (500, 1), (1, 0)]
    assert d._ddim_pairs(3, 0.5) == [(999, 500), (500, 1), (1, 0)]
    assert d._ddim_pairs((7,), 0) == [(7, 0)]
    for bad in ([], [999, 999, 1], [5, 10], [1000, 1], [999, 0], [999, 2.5], [True], "abc", 3.5, 0, 1000):
        with pytest.raises(ValueError):
            d._ddim_pairs(bad, 0.0)
    for eta in (-1e-6, -1.0, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            d._ddim_pairs(50, eta)


def test_snapshot_rule_is_the_ddpm_rule_on_the_full_chain():
    import afdm
    d = _diff(1000)
    pairs = d._ddim_pairs(999, 0.0)
    assert pairs == [(i, i - 1) for i in range(999, 0, -1)]
    assert [t for t, tp in pairs if afdm.Diffusion.ddim_snapshot(t, tp)] == [i for i in range(999, 0, -1) if i % 100 == 0]
    # 50 steps of the 1000-step chain: every step that crosses a multiple of 100 is kept
    kept = [(t, tp) for t, tp in d._ddim_pairs(50, 0.0) if d.ddim_snapshot(t, tp)]
    assert len(kept) == 9 and all(tp // 100 == t // 100 - 1 for t, tp in kept)


def test_header_declares_and_types_the_ddim_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_ddim_step"] == (I, [P, P, P, P, I, I, F, P, L, P])
    assert sigs["afd_ddim_step_dev"] == (I, [P, P, P, P, P, P, F, P, L, P])
    assert sigs["afd_ddim_step_cfg"] == (I, [P, P, P, P, I, I, F, F, P, P, L, P])
    assert sigs["afd_ddim_step_cfg_dev"] == (I, [P, P, P, P, P, P, F, F, P, P, L, P])


def test_ddim_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    with pytest.raises(afdm.AfdError, match="afd_ddim_step: .*NULL"):
        lib.afd_ddim_step(None, None, None, None, 5, 1, 0.0, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_dev: .*NULL"):
        lib.afd_ddim_step_dev(None, None, None, None, None, None, 0.0, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_cfg: .*NULL"):
        lib.afd_ddim_step_cfg(None, None, None, None, 5, 1, 0.0, 3.0, None, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_cfg_dev: .*NULL"):
        lib.afd_ddim_step_cfg_dev(None, None, None, None, None, None, 0.0, 3.0, None, None, 8, None)
    # non-NULL but never dereferenced: each check returns before a launch
    buf = (ctypes.c_float * 64)()
    q = ctypes.addressof(buf)
    for t, tp in ((5, 5), (5, 7), (5, -1), (0, 0)):
        with pytest.raises(afdm.AfdError, match=r"afd_ddim_step: need 0 <= t_prev < t"):
            lib.afd_ddim_step(q, q, None, q, t, tp, 0.0, q, 8, None)
        with pytest.raises(afdm.AfdError, match=r"afd_ddim_step_cfg: need 0 <= t_prev < t"):
            lib.afd_ddim_step_cfg(q, q, None, q, t, tp, 0.0, 3.0, q, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step: eta"):
        lib.afd_ddim_step(q, q, None, q, 5, 1, -0.5, q, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_dev: eta"):
        lib.afd_ddim_step_dev(q, q, None, q, q, q, float("nan"), q, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_cfg_dev: n must be positive"):
        lib.afd_ddim_step_cfg_dev(q, q, None, q, q, q, 0.0, 3.0, q, None, 0, None)
    with pytest.raises(afdm.AfdError, match="afd_ddim_step_cfg: eta"):
        lib.afd_ddim_step_cfg(q, q, None, q, 5, 1, -1.0, 3.0, q, None, 8, None)


def test_public_signatures_take_steps_and_eta():
    import afdm
    D = afdm.Diffusion
    for fn in (D.sample, D.revert, D.sample_concurrent):
        sp = inspect.signature(fn).parameters
        assert sp["steps"].default is None and sp["eta"].default == 0.0
    sp = inspect.signature(D.sample).parameters
    assert list(sp)[:10] == ["self", "model", "n", "image_channels", "theta", "noise_source", "return_float", "graph", "labels",
                             "cfg_scale"]


def test_ddim_requests_that_are_refused_before_touching_a_device():
    import afdm
    d = _diff(1000)
    m = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    with pytest.raises(NotImplementedError, match="theta"):
        d.sample(m, n=2, image_channels=1, theta=30, steps=50)
    with pytest.raises(ValueError, match="eta"):
        d.sample(m, n=2, image_channels=1, steps=50, eta=-0.1)
    with pytest.raises(ValueError, match="eta applies to the DDIM sampler"):
        d.sample(m, n=2, image_channels=1, eta=0.5)
    with pytest.raises(ValueError):
        d.sample(m, n=2, image_channels=1, steps=1000)
    with pytest.raises(ValueError):
        d.revert(m, n=1, image_channels=1, steps=[10, 20])
    with pytest.raises(ValueError):
        d.sample_concurrent(m, n=2, image_channels=1, steps=0)
    with pytest.raises(NotImplementedError):
        d.sample_sharded(m, n=2, image_channels=1, steps=50)
    with pytest.raises(NotImplementedError):
        d.sample_shift(m, n=2, image_channels=1, shift=2, steps=50)
    with pytest.raises(NotImplementedError):
        d.sample_rotation_sweep(m, n=2, image_channels=1, thetas=[0, 30], steps=50)
    with pytest.raises(NotImplementedError):
        d.sample_rotation_sweep_sharded(m, n=2, image_channels=1, thetas=[0, 30], steps=50)
    assert m.training and m._t_range is None
