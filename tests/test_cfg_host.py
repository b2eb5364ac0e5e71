"""CPU-side tests of class-conditional sampling with classifier-free guidance: the C ABI declares and types the new entry
points, the public signatures carry the new arguments, and the host-side checks and the label-dropout draw behave."""
import ctypes
import inspect
import math

import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def test_header_declares_and_types_the_cfg_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_label_embed_add_fwd"] == (I, [P, P, P, P, I, I, I, P])
    assert sigs["afd_denoise_step_cfg"] == (I, [P, P, P, P, P, P, I, F, P, P, L, P])
    assert sigs["afd_denoise_step_cfg_dev"] == (I, [P, P, P, P, P, P, P, F, P, P, L, P])
    assert sigs["afd_embed_add_fwd"] == sigs["afd_label_embed_add_fwd"]          # the old entry point keeps its ABI


def test_cfg_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    with pytest.raises(afdm.AfdError, match="afd_label_embed_add_fwd"):
        lib.afd_label_embed_add_fwd(None, None, None, None, 1, 1, 1, None)
    with pytest.raises(afdm.AfdError, match="afd_denoise_step_cfg"):
        lib.afd_denoise_step_cfg(None, None, None, None, None, None, 5, 3.0, None, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_denoise_step_cfg_dev"):
        lib.afd_denoise_step_cfg_dev(None, None, None, None, None, None, None, 3.0, None, None, 8, None)


def test_public_signatures_take_labels_cfg_scale_and_p_uncond():
    import afdm
    sp = inspect.signature(afdm.Diffusion.sample).parameters
    assert sp["labels"].default is None and sp["cfg_scale"].default == 0.0
    # the existing arguments keep their order and defaults
    assert list(sp)[:8] == ["self", "model", "n", "image_channels", "theta", "noise_source", "return_float", "graph"]
    tp = inspect.signature(afdm.TrainStep.__init__).parameters
    assert tp["p_uncond"].default == 0.0 and tp["conditional"].default is False
    assert afdm.NULL_LABEL == -1 and afdm.ops.NULL_LABEL == -1


def test_p_uncond_needs_a_conditional_step():
    import afdm
    with pytest.raises(ValueError, match="conditional=True"):
        afdm.TrainStep(None, None, lr=3e-4, p_uncond=0.1)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        afdm.TrainStep(None, None, lr=3e-4, conditional=True, p_uncond=1.5)


def test_label_dropout_mask_is_reproducible_from_the_cpu_generator():
    from afdm.training import label_dropout_mask
    torch.manual_seed(11)
    a = [label_dropout_mask(64, 0.25) for _ in range(3)]
    torch.manual_seed(11)
    b = [label_dropout_mask(64, 0.25) for _ in range(3)]
    for u, v in zip(a, b):
        assert u.dtype == torch.bool and u.shape == (64,) and not u.is_cuda and torch.equal(u, v)
    torch.manual_seed(11)
    assert torch.equal(a[0], torch.rand(64) < 0.25)                     # one uniform draw per sample, in order
    frac = float(torch.cat(a).float().mean())
    assert 0.1 < frac < 0.4
    assert not label_dropout_mask(32, 0.0).any() and label_dropout_mask(32, 1.0).all()


def test_sample_rejects_bad_label_requests_before_touching_a_device():
    import afdm
    diff = afdm.Diffusion(noise_steps=5, img_size=32, device="cpu")
    cond = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3, num_classes=5)
    uncond = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    with pytest.raises(ValueError, match="label embedding"):
        diff.sample(uncond, n=2, image_channels=1, labels=[0, 1])
    with pytest.raises(ValueError, match="expected 2 labels"):
        diff.sample(cond, n=2, image_channels=1, labels=[0, 1, 2])
    with pytest.raises(ValueError, match="integers"):
        diff.sample(cond, n=2, image_channels=1, labels=torch.tensor([0.0, 1.0]))
    with pytest.raises(NotImplementedError):
        diff.sample(cond, n=2, image_channels=1, theta=30, labels=[0, 1])
    with pytest.raises(ValueError, match="needs class labels"):
        diff.sample(cond, n=2, image_channels=1, cfg_scale=3.0)
