"""CPU-side tests of reference-guided sampling (ILVR): the public signatures, the header's types of the two refine entry points,
their argument checks (which return before any launch), the argument checks of Diffusion.ilvr (which raise before any device
work), and the default operator phi_L in fp64: symmetric, eigenvalues in [0, 1]."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_long


def _diff(T=1000, img=32):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=img, device="cpu")


def _model(num_classes=None):
    import afdm
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3, **kw)


def test_ilvr_public_signatures():
    import afdm
    from afdm import ops
    sp = inspect.signature(afdm.Diffusion.ilvr).parameters
    assert list(sp) == ["self", "model", "reference", "factor", "t_stop", "taps", "steps", "eta", "labels", "cfg_scale",
                        "noise_source", "graph", "return_float"]
    assert sp["factor"].default == 4 and sp["t_stop"].default == 0 and sp["taps"].default is None and sp["steps"].default is None
    assert sp["eta"].default == 0.0 and sp["labels"].default is None and sp["cfg_scale"].default == 0.0
    assert sp["noise_source"].default == "reference" and sp["graph"].default is None and sp["return_float"].default is False
    assert "sampler" not in sp
    sp = inspect.signature(afdm.Diffusion.reference_from_lowres).parameters
    assert list(sp) == ["self", "low", "factor", "taps"] and sp["taps"].default is None
    assert list(inspect.signature(ops.lowpass_refine).parameters) == ["x", "ref", "noise", "alpha_hat", "t_prev", "taps", "levels",
                                                                      "out", "out2"]
    assert list(inspect.signature(ops.lowpass_refine_dev).parameters) == ["x", "ref", "noise", "alpha_hat", "t_prev_dev", "taps",
                                                                          "levels", "out", "out2"]
    assert list(inspect.signature(ops.lowpass_project).parameters) == ["v", "taps", "levels"]
    assert list(inspect.signature(afdm.ilvr_results).parameters) == ["model_data", "reference", "kw"]
    from afdm import tasks
    assert tasks.ilvr_results is afdm.ilvr_results


def test_header_declares_and_types_the_refine_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_lowpass_refine"] == (I, [P, P, P, P, I, P, I, I, P, P, L, I, P])
    assert sigs["afd_lowpass_refine_dev"] == (I, [P, P, P, P, P, P, I, I, P, P, L, I, P])


def test_refine_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    E = afdm.AfdError
    # non-NULL but never dereferenced: every check returns before a launch.  Six buffers 1 KiB apart in one arena, of which the
    # 2 planes of 8 x 8 that the calls below describe use the first 512 bytes each.
    arena = (ctypes.c_float * (6 * 256))()
    x, ref, z, ah, out, out2 = (ctypes.addressof(arena) + 1024 * i for i in range(6))
    taps = (ctypes.c_float * 289)()
    k = ctypes.addressof(taps)
    tpd = ctypes.addressof((ctypes.c_int64 * 1)())

    def host(x=x, ref=ref, z=z, ah=ah, tp=5, k=k, N=3, lv=1, out=out, out2=out2, planes=2, S=8):
        return lib.afd_lowpass_refine(x, ref, z, ah, tp, k, N, lv, out, out2, planes, S, None)

    def dev(x=x, ref=ref, z=z, ah=ah, tpd=tpd, k=k, N=3, lv=1, out=out, out2=out2, planes=2, S=8):
        return lib.afd_lowpass_refine_dev(x, ref, z, ah, tpd, k, N, lv, out, out2, planes, S, None)

    for name, fn in (("afd_lowpass_refine", host), ("afd_lowpass_refine_dev", dev)):
        for arg in ("x", "ref", "ah", "k", "out"):
            with pytest.raises(E, match=f"{name}: .*NULL"):
                fn(**{arg: None})
        for planes in (0, -3):
            with pytest.raises(E, match=f"{name}: planes must be positive"):
                fn(planes=planes)
        for N in (2, 6, 14, 17, 0, -3):
            with pytest.raises(E, match=f"{name}: N must be odd and at most 15"):
                fn(N=N)
        for S in (0, 2, 6, 12, 48, 128, -8):
            with pytest.raises(E, match=f"{name}: S must be a power of two"):
                fn(S=S)
        for S, lv in ((8, 0), (8, -1), (8, 3), (4, 2), (64, 6), (64, 40)):
            with pytest.raises(E, match=f"{name}: levels"):
                fn(S=S, lv=lv, planes=1 if S == 64 else 2)
        # ref or noise overlapping an output
        with pytest.raises(E, match=f"{name}: ref and noise must not overlap"):
            fn(ref=out)
        with pytest.raises(E, match=f"{name}: ref and noise must not overlap"):
            fn(ref=out2 + 4 * 100)
        with pytest.raises(E, match=f"{name}: ref and noise must not overlap"):
            fn(z=out + 4)
        with pytest.raises(E, match=f"{name}: ref and noise must not overlap"):
            fn(z=out2)
        # x_out is x itself, or apart from it
        with pytest.raises(E, match=f"{name}: x_out must be x itself or apart"):
            fn(out=x + 4)
        with pytest.raises(E, match=f"{name}: x_out must be x itself or apart"):
            fn(out2=x)
    with pytest.raises(E, match="afd_lowpass_refine_dev: .*NULL"):
        dev(tpd=None)
    for tp in (-1, -1000):
        with pytest.raises(E, match="afd_lowpass_refine: t_prev must not be negative"):
            host(tp=tp)
    with pytest.raises(E, match="afd_lowpass_refine: noise must not be NULL when t_prev > 0"):
        host(z=None, tp=1)
    with pytest.raises(E, match="afd_lowpass_refine_dev: noise must not be NULL"):
        dev(z=None)


def test_ilvr_argument_errors_before_any_device_work():
    d = _diff()
    m = _model()
    ref = torch.zeros(2, 1, 32, 32)
    for N in (2, 6):
        with pytest.raises(ValueError, match="N odd"):
            d.ilvr(m, ref, taps=torch.ones(N, N) / (N * N))
    with pytest.raises(ValueError, match="N odd and at most 15"):
        d.ilvr(m, ref, taps=np.ones((17, 17), dtype=np.float32))
    with pytest.raises(ValueError, match="taps"):
        d.ilvr(m, ref, taps=torch.ones(3, 5))
    with pytest.raises(ValueError, match="taps"):
        d.ilvr(m, ref, taps=torch.ones(9))
    for factor in (3, 1, 32, 64, 0, -2, 2.0, True, None):
        with pytest.raises(ValueError, match="factor"):
            d.ilvr(m, ref, factor=factor)
    for t_stop in (-1, 1001, 2.5, None, True):
        with pytest.raises(ValueError, match="t_stop"):
            d.ilvr(m, ref, t_stop=t_stop)
    with pytest.raises(ValueError, match="shape"):
        d.ilvr(m, torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError, match="shape"):
        d.ilvr(m, torch.zeros(1, 32, 32))
    with pytest.raises(ValueError, match="shape"):
        d.ilvr(m, torch.zeros(0, 1, 32, 32))
    with pytest.raises(ValueError, match="fp32"):
        d.ilvr(m, ref.double())
    with pytest.raises(ValueError, match="fp32"):
        d.ilvr(m, ref.numpy())
    with pytest.raises(ValueError, match="eta applies to the DDIM sampler"):
        d.ilvr(m, ref, eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        d.ilvr(m, ref, steps=50, eta=-1.0)
    with pytest.raises(ValueError):
        d.ilvr(m, ref, steps=1000)
    with pytest.raises(ValueError, match="cfg_scale needs class labels"):
        d.ilvr(m, ref, cfg_scale=3.0)
    with pytest.raises(ValueError, match="label embedding"):
        d.ilvr(m, ref, labels=[0, 1])
    with pytest.raises(ValueError, match="expected 2 labels"):
        d.ilvr(_model(num_classes=4), ref, labels=[0, 1, 2])
    with pytest.raises(TypeError):
        d.ilvr(m, ref, steps=10, sampler="dpmpp_2m")
    for img in (48, 128, 2):
        with pytest.raises(NotImplementedError, match="power of two"):
            _diff(img=img).ilvr(m, torch.zeros(2, 1, img, img))
    for low, factor in ((torch.zeros(2, 1, 16, 16), 4), (torch.zeros(2, 1, 8, 8).double(), 4), (torch.zeros(1, 8, 8), 4)):
        with pytest.raises(ValueError, match="low must"):
            d.reference_from_lowres(low, factor)
    with pytest.raises(ValueError, match="factor"):
        d.reference_from_lowres(torch.zeros(2, 1, 8, 8), 3)
    assert m.training and m._t_range is None


@pytest.mark.parametrize("levels", [1, 2])
def test_default_operator_is_symmetric_with_eigenvalues_in_the_unit_interval(levels):
    """phi_L = 4^L U^L D^L with the filter `ilvr` uses by default, as a 256 x 256 fp64 matrix built from the oracle's resamplers."""
    import afdm
    from oracle import ref_ops as R
    taps, got_levels = _diff(img=16)._ilvr_operator("ilvr", 2 ** levels, None)
    assert got_levels == levels and taps.N == 9
    assert np.array_equal(taps.arr, afdm.circularLowpassKernel(math.pi / 2, 9, beta=8).numpy())
    k = torch.from_numpy(taps.arr).double()
    v = torch.eye(256, dtype=torch.float64).reshape(256, 1, 16, 16)
    for _ in range(levels):
        v = R.filt_down2(v, k)
    for _ in range(levels):
        v = 4.0 * R.filt_up2(v, k)
    M = v.reshape(256, 256).T.numpy()
    assert np.abs(M - M.T).max() <= 1e-12
    ev = np.linalg.eigvalsh(0.5 * (M + M.T))
    print(f"phi_{levels}: eigenvalues in [{ev.min():.3e}, {ev.max():.6f}]")
    assert ev.min() >= -1e-12 and ev.max() <= 1.0
    assert ev.max() > 0.5                                       # (the 4^L gain is there: without it the largest is below 0.25)
