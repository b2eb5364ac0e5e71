"""CPU-side tests of the EMA of the weights: the public names, the C ABI of the three entry points and their argument checks
(which return before any device is touched), and the per-tensor path of `EMA` on CPU modules against the reference's rule."""
import copy
import ctypes
import math

import pytest
import torch

P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}


def test_ema_is_exported_where_the_reference_has_it():
    import afdm
    from modules.ddpm_utils import EMA
    assert EMA is afdm.EMA
    e = EMA(0.995)
    assert e.beta == 0.995 and e.step == 0
    for name in ("update_model_average", "update_average", "step_ema", "reset_parameters"):
        assert callable(getattr(e, name))
    import inspect
    assert inspect.signature(EMA.step_ema).parameters["step_start_ema"].default == 2000
    a = afdm.argument()
    assert a.ema_beta is None and a.ema_start == 2000


def test_header_declares_and_types_the_ema_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_ema_step"] == (I, [P, P, L, I, F, F, P])
    assert sigs["afd_adamw_ema_tick"] == (I, [P, F, F, P, I, P])
    assert sigs["afd_adamw_ema_step"] == (I, [P, P, P, P, L, P, F, F, F, F, F, F, P, L, P, F, F, P])


def test_ema_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_float * 64)()
    q = ctypes.addressof(buf)
    with pytest.raises(afdm.AfdError, match="afd_ema_step: .*NULL"):
        lib.afd_ema_step(None, q, 8, 0, 0.9, 0.1, None)
    with pytest.raises(afdm.AfdError, match="afd_ema_step: .*NULL"):
        lib.afd_ema_step(q, None, 8, 0, 0.9, 0.1, None)
    for n in (0, -4):
        with pytest.raises(afdm.AfdError, match="afd_ema_step: n must be positive"):
            lib.afd_ema_step(q, q, n, 0, 0.9, 0.1, None)
    for b, omb in ((-0.1, 1.1), (1.5, -0.5), (float("nan"), 0.5), (0.5, float("nan"))):
        with pytest.raises(afdm.AfdError, match="afd_ema_step: beta"):
            lib.afd_ema_step(q, q, 8, 0, b, omb, None)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ema_tick: .*NULL"):
        lib.afd_adamw_ema_tick(None, 0.9, 0.999, q, 0, None)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ema_tick: .*NULL"):
        lib.afd_adamw_ema_tick(q, 0.9, 0.999, None, 0, None)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ema_tick: start"):
        lib.afd_adamw_ema_tick(q, 0.9, 0.999, q, -1, None)

    def step(p=q, g=q, m=q, v=q, n_active=8, st=q, ema=q, n_ema=8, es=q, beta=0.9, omb=0.1):
        lib.afd_adamw_ema_step(p, g, m, v, n_active, st, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, ema, n_ema, es, beta, omb, None)
    for k in ("p", "g", "m", "v", "st", "ema", "es"):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ema_step: .*NULL"):
            step(**{k: None})
    with pytest.raises(afdm.AfdError, match="afd_adamw_ema_step: n_active and n_ema must be positive"):
        step(n_active=0)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ema_step: n_active and n_ema must be positive"):
        step(n_ema=-1)
    with pytest.raises(afdm.AfdError, match=r"afd_adamw_ema_step: n_active > n_ema"):
        step(n_active=9, n_ema=8)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ema_step: beta"):
        step(beta=1.01, omb=-0.01)


def _pair(seed=0):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(13, 7), torch.nn.GELU(), torch.nn.Linear(7, 5), torch.nn.BatchNorm1d(5))
    return net, copy.deepcopy(net)


def test_slow_path_copies_then_blends_bit_for_bit_in_place():
    import afdm
    beta = 0.9
    model, ema_model = _pair()
    with torch.no_grad():
        for p in ema_model.parameters():
            p.add_(1.0)                                          # so that a copy is visible
    ptrs = [p.data_ptr() for p in ema_model.parameters()]
    ema = afdm.EMA(beta)
    g = torch.Generator().manual_seed(1)
    want = [p.detach().clone() for p in ema_model.parameters()]
    for call in range(1, 7):
        with torch.no_grad():                                    # "an optimizer step"
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
            model[3].running_mean.add_(0.5)
        ema.step_ema(ema_model, model, step_start_ema=2)
        cur = [p.detach() for p in model.parameters()]
        if call <= 2:
            want = [c.clone() for c in cur]
            assert torch.equal(ema_model[3].running_mean, model[3].running_mean)       # buffers copied on reset
        else:
            want = [w * beta + (1 - beta) * c for w, c in zip(want, cur)]              # the reference's expression, restated
            assert not torch.equal(ema_model[3].running_mean, model[3].running_mean)   # ... and left alone on blend
        for w, p in zip(want, ema_model.parameters()):
            assert torch.equal(p.detach(), w), call
        assert ema.step == call
    assert ema.step == 6
    assert [p.data_ptr() for p in ema_model.parameters()] == ptrs
    assert not torch.equal(want[0], next(model.parameters()).detach())      # blending happened


def test_update_average_is_the_reference_expression():
    import afdm
    e = afdm.EMA(0.995)
    new = torch.randn(100)
    assert e.update_average(None, new) is new
    old = torch.randn(100)
    assert torch.equal(e.update_average(old, new), old * 0.995 + (1 - 0.995) * new)


def test_ema_value_errors():
    import afdm
    for bad in (-0.01, 1.01, float("nan"), "x", None):
        with pytest.raises(ValueError, match="beta"):
            afdm.EMA(bad)
    afdm.EMA(0)
    afdm.EMA(1)
    model, ema_model = _pair()
    e = afdm.EMA(0.9)
    with pytest.raises(ValueError, match="ema_model is model"):
        e.step_ema(model, model)
    other = torch.nn.Sequential(torch.nn.Linear(13, 7), torch.nn.GELU(), torch.nn.Linear(7, 6), torch.nn.BatchNorm1d(6))
    with pytest.raises(ValueError, match="architecture"):
        e.step_ema(other, model)
    with pytest.raises(ValueError, match="architecture"):
        e.update_model_average(torch.nn.Sequential(torch.nn.Linear(13, 7)), model)
    assert e.step == 0


def test_unet_slow_path_on_cpu_matches_load_state_dict_then_blend():
    import afdm
    afdm.set_seed(3)
    model = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    afdm.set_seed(4)
    ema_model = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    e = afdm.EMA(0.99)
    e.step_ema(ema_model, model, step_start_ema=1)
    for (k, a), b in zip(ema_model.state_dict().items(), model.state_dict().values()):
        assert torch.equal(a, b), k
    old = {k: v.clone() for k, v in ema_model.state_dict().items()}
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.5)
    e.step_ema(ema_model, model, step_start_ema=1)
    for (k, a), b in zip(ema_model.state_dict().items(), model.state_dict().values()):
        assert torch.equal(a, old[k] * 0.99 + (1 - 0.99) * b), k


def test_train_step_requires_ema_and_ema_model_together():
    import afdm
    model, ema_model = _pair()
    for kw in ({"ema": afdm.EMA(0.9)}, {"ema_model": ema_model}):
        with pytest.raises(ValueError, match="ema and ema_model"):
            afdm.TrainStep(model, None, lr=1e-3, **kw)
