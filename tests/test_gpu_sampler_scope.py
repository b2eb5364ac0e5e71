"""GPU tests of the scope every loop over the model runs in (Diffusion._model_scope): after an exception in an eager step the
samplers leave the model in train mode with its timestep hint cleared, as after a normal return, and the evaluations put back
the mode and the hint they found.  DDIM, DPM-Solver++ and inpainting have their own cases next to their other tests."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
T, N = 6, 2


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _boom(afdm, dev, at):
    """A UNet whose forward number `at` raises, and the process that samples from it."""

    class Boom(afdm.UNet):
        calls = 0

        def forward(self, *a, **kw):
            Boom.calls += 1
            if Boom.calls == at:
                raise RuntimeError(f"boom at forward {at}")
            return super().forward(*a, **kw)

    afdm.set_seed(42)
    model = Boom(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)
    return Boom, model, afdm.Diffusion(noise_steps=T, img_size=32, device=dev)


CALLS = {
    "sample": lambda d, m: d.sample(m, n=N, image_channels=3, noise_source="device", steps=None),
    "revert": lambda d, m: d.revert(m, n=N, image_channels=3, noise_source="device"),
    "sample_rotation_sweep": lambda d, m: d.sample_rotation_sweep(m, N, 3, [0.0, 30.0]),
    "sample_shift": lambda d, m: d.sample_shift(m, n=N, image_channels=3, shift=2, noise_source="device"),
    "sample_concurrent": lambda d, m: d.sample_concurrent(m, n=N, image_channels=3, steps=None, graph=False, batch=1, streams=2),
}


@pytest.mark.parametrize("name", list(CALLS))
def test_sampler_restores_the_model_after_an_exception(A, name):
    """The third forward, an eager step of each of these, raises: the model is back in train mode and unhinted."""
    afdm, dev = A
    Boom, model, diff = _boom(afdm, dev, at=3)
    assert model.training and model._t_range is None
    with pytest.raises(RuntimeError, match="boom at forward 3"):
        CALLS[name](diff, model)
    torch.cuda.synchronize()
    assert Boom.calls == 3
    assert model.training
    assert model._t_range is None


def test_calc_bpd_puts_back_the_mode_and_hint_it_found_after_an_exception(A):
    """The evaluations' flavour of the scope: a model found in eval mode with a hint of its own gets both back."""
    afdm, dev = A
    Boom, model, diff = _boom(afdm, dev, at=1)
    model.eval()
    model._t_range = 17
    images = torch.rand(N, 3, 32, 32) * 2 - 1
    with pytest.raises(RuntimeError, match="boom at forward 1"):
        diff.calc_bpd(model, images, noise_source="device")
    assert Boom.calls == 1
    assert not model.training
    assert model._t_range == 17
