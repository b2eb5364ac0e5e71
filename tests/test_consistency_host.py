"""Consistency distillation, host side: the coefficient table of the parametrisation, the level tables of a teacher's chain, the C
ABI of the kernels and the argument errors of ConsistencyStep, consistency_distill, consistency_sample and ddpm_run's key.  No
GPU (the kernels, the step, the loop and the sampler are checked in test_gpu_consistency.py)."""
import ctypes
import math

import pytest
import torch

P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int


def _diff(T=1000, **kw):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu", **kw)


@pytest.mark.parametrize("sd,s", [(0.5, 10.0), (1.0, 1.0), (0.25, 3)])
def test_consistency_coefficients_follow_the_formula(sd, s):
    tab = _diff().consistency_coefficients(sd, s)
    assert tab.dtype == torch.float64 and tuple(tab.shape) == (1000, 2) and not tab.is_cuda and tab.is_contiguous()
    assert tab[0].tolist() == [1.0, 0.0]                              # the boundary condition, exactly
    for t in (1, 2, 17, 500, 999):
        st = float(s) * t
        assert tab[t, 0].item() == pytest.approx(sd * sd / (st * st + sd * sd), rel=1e-15, abs=0)
        assert tab[t, 1].item() == pytest.approx(st / math.sqrt(st * st + sd * sd), rel=1e-15, abs=0)
    assert bool((tab[1:, 0] < tab[:-1, 0]).all()) and bool((tab[1:, 1] > tab[:-1, 1]).all())
    assert bool((tab[:, 0] > 0).all()) and bool((tab[1:, 1] > 0).all()) and bool((tab[:, 1] < 1).all())


def test_consistency_coefficients_defaults_and_errors():
    d = _diff()
    tab = d.consistency_coefficients()
    assert torch.equal(tab, d.consistency_coefficients(sigma_data=0.5, timestep_scaling=10.0))
    assert tab[1, 0].item() == pytest.approx(0.25 / 100.25, rel=1e-15) and tab[1, 1].item() == pytest.approx(10.0 / math.sqrt(100.25), rel=1e-15)
    assert tuple(_diff(12).consistency_coefficients().shape) == (12, 2)
    for bad in (0, -1.0, float("nan"), float("inf"), None, "0.5", True):
        with pytest.raises(ValueError, match="consistency_coefficients: sigma_data"):
            d.consistency_coefficients(sigma_data=bad)
        with pytest.raises(ValueError, match="consistency_coefficients: timestep_scaling"):
            d.consistency_coefficients(timestep_scaling=bad)


def test_consistency_levels_are_the_slices_of_the_chain():
    d = _diff()
    for chain in (d.ddim_timesteps(8), d.ddim_timesteps(7), [999], [500, 3], d.ddim_timesteps(50)):
        levels = list(chain) + [0]
        t, t_prev = d.consistency_levels(chain)
        for got, want in ((t, levels[:-1]), (t_prev, levels[1:])):
            assert got.dtype == torch.long and not got.is_cuda and got.tolist() == want
        assert t_prev.tolist()[-1] == 0 and torch.equal(t[1:], t_prev[:-1]) and bool((t_prev < t).all()) and int(t.min()) >= 1


@pytest.mark.parametrize("chain", ([3, 500], [500, 500], [1000, 3], [5, 0], [], 8, [999.0, 1.0], [999, True]))
def test_consistency_levels_rejects_bad_chains(chain):
    with pytest.raises(ValueError):
        _diff().consistency_levels(chain)


def test_consistency_levels_needs_a_decreasing_alpha_hat():
    d = _diff(10)
    assert d.consistency_levels([9, 5, 3])[0].tolist() == [9, 5, 3]
    d.alpha_hat = d.alpha_hat.clone()
    d.alpha_hat[5] = d.alpha_hat[9]
    with pytest.raises(ValueError, match="alpha_hat must strictly decrease"):
        d.consistency_levels([9, 5, 3])


def test_loss_weightings_are_unchanged():
    import afdm
    assert afdm.Diffusion.LOSS_WEIGHTINGS == ("min_snr", "truncated_snr")


def test_header_declares_and_library_exports_the_consistency_entry_points():
    import afdm
    from afdm._lib import LIBPATH, parse_header
    sigs = parse_header()
    assert sigs["afd_consistency_fn"] == (ctypes.c_int, [P, P, P, P, P, I, P, L, L, P])
    assert sigs["afd_consistency_target"] == (ctypes.c_int, [P, P, P, P, P, P, P, I, P, P, L, L, P])
    assert sigs["afd_consistency_step"] == (ctypes.c_int, [P, P, P, P, P, I, I, I, P, L, L, P])
    assert sigs["afd_consistency_step_dev"] == (ctypes.c_int, [P, P, P, P, P, I, P, P, P, L, L, P])
    cdll = ctypes.CDLL(LIBPATH)
    for name in ("afd_consistency_fn", "afd_consistency_target", "afd_consistency_step", "afd_consistency_step_dev"):
        assert hasattr(cdll, name), f"{name} declared in include/afd.h but not exported"
    for name in ("consistency_fn", "consistency_target", "consistency_step", "consistency_step_dev"):
        assert callable(getattr(afdm.ops, name))
    assert afdm.ConsistencyStep is afdm.training.ConsistencyStep and afdm.consistency_distill is afdm.training.consistency_distill


def test_consistency_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_float * 4096)()
    at = lambda i: ctypes.addressof(buf) + 4 * i
    # B = 2, chw = 8: 16 floats per tensor, 2 int64 (4 floats) per timestep tensor
    # fn:     out, z, t, alpha_hat, coef, kind, f_out, B, chw, stream
    fn = [at(0), at(64), at(128), at(256), at(1024), 1, at(320), 2, 8, None]
    # target: out_tgt, z_prev, z_t, t, t_prev, alpha_hat, coef, kind, x_tilde, eps_tilde, B, chw, stream
    tgt = [at(0), at(64), at(384), at(128), at(192), at(256), at(1024), 1, at(320), at(512), 2, 8, None]
    # step:   out, z, noise, alpha_hat, coef, kind, t, t_next, x_out, n_rows, chw, stream
    stp = [at(0), at(64), at(384), at(256), at(1024), 1, 5, 2, at(320), 2, 8, None]
    # dev:    out, z, noise, alpha_hat, coef, kind, t_dev, t_next_dev, x_out, n_rows, chw, stream
    dev = [at(0), at(64), at(384), at(256), at(1024), 1, at(128), at(192), at(320), 2, 8, None]
    for f, args, ptrs, ikind, idims in ((lib.afd_consistency_fn, fn, (0, 1, 2, 3, 4, 6), 5, (7, 8)),
                                        (lib.afd_consistency_target, tgt, (0, 1, 2, 3, 4, 5, 6, 8, 9), 7, (10, 11)),
                                        (lib.afd_consistency_step, stp, (0, 1, 3, 4, 8), 5, (9, 10)),
                                        (lib.afd_consistency_step_dev, dev, (0, 1, 3, 4, 6, 7, 8), 5, (9, 10))):
        name = f.__name__
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            with pytest.raises(afdm.AfdError, match=f"{name}: .*NULL"):
                f(*bad)
        for k in (-1, 3, 7):
            bad = list(args)
            bad[ikind] = k
            with pytest.raises(afdm.AfdError, match=f"{name}: kind must be"):
                f(*bad)
        for i in idims:
            for v in (0, -4):
                bad = list(args)
                bad[i] = v
                with pytest.raises(afdm.AfdError, match=f"{name}: .*positive"):
                    f(*bad)
    # an output may be an input itself, never a shifted view of one, a timestep tensor, the noise or the other output
    for i_in in (0, 1):
        bad = list(fn)
        bad[6] = fn[i_in] + 4
        with pytest.raises(afdm.AfdError, match="afd_consistency_fn: f_out must be out or z itself or apart"):
            lib.afd_consistency_fn(*bad)
    bad = list(fn)
    bad[6] = fn[2]
    with pytest.raises(afdm.AfdError, match="afd_consistency_fn: .*must not overlap t"):
        lib.afd_consistency_fn(*bad)
    for i_out in (8, 9):
        for i_in in (0, 1, 2):
            bad = list(tgt)
            bad[i_out] = tgt[i_in] + 8
            with pytest.raises(afdm.AfdError, match="afd_consistency_target: x_tilde and eps_tilde must each be"):
                lib.afd_consistency_target(*bad)
        for i_t in (3, 4):
            bad = list(tgt)
            bad[i_out] = tgt[i_t]
            with pytest.raises(afdm.AfdError, match="afd_consistency_target: x_tilde and eps_tilde must each be"):
                lib.afd_consistency_target(*bad)
    bad = list(tgt)
    bad[9] = bad[8]
    with pytest.raises(afdm.AfdError, match="afd_consistency_target: x_tilde and eps_tilde must each be"):
        lib.afd_consistency_target(*bad)
    for f, args in ((lib.afd_consistency_step, stp), (lib.afd_consistency_step_dev, dev)):
        for i_in in (0, 1):
            bad = list(args)
            bad[8] = args[i_in] + 4
            with pytest.raises(afdm.AfdError, match=f"{f.__name__}: x_out must be out or z itself or apart"):
                f(*bad)
        bad = list(args)
        bad[8] = args[2] + 4                                          # over the noise
        with pytest.raises(afdm.AfdError, match=f"{f.__name__}: x_out must be .*must not overlap noise"):
            f(*bad)
    bad = list(dev)
    bad[8] = dev[6]
    with pytest.raises(afdm.AfdError, match="afd_consistency_step_dev: x_out must be .*t_dev or t_next_dev"):
        lib.afd_consistency_step_dev(*bad)
    # the host levels of the step: 0 <= t_next < t, and noise unless t_next == 0
    for t, tn in ((5, 5), (2, 5), (5, -1), (0, 0)):
        bad = list(stp)
        bad[6], bad[7] = t, tn
        with pytest.raises(afdm.AfdError, match="afd_consistency_step: need 0 <= t_next < t"):
            lib.afd_consistency_step(*bad)
    bad = list(stp)
    bad[2] = None
    with pytest.raises(afdm.AfdError, match="afd_consistency_step: noise must not be NULL unless t_next == 0"):
        lib.afd_consistency_step(*bad)
    # the torch-level wrappers: host tensors, unknown kinds, a table of the wrong type
    x = torch.zeros(2, 3, 4, 4)
    t, ah, coef = torch.tensor([2, 2]), torch.full((10,), 0.5), torch.zeros(10, 2, dtype=torch.float64)
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.consistency_fn(x, x, t, ah, coef, "v")
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.consistency_target(x, x, x, t, t, ah, coef, "x0")
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.consistency_step(x, x, x, ah, coef, "x0", 5, 2)
    with pytest.raises(afdm.AfdError, match="unknown prediction 'velocity'"):
        afdm.ops.consistency_fn(x, x, t, ah, coef, "velocity")
    with pytest.raises(afdm.AfdError, match="unknown prediction 'velocity'"):
        afdm.ops.consistency_step(x, x, x, ah, coef, "velocity", 5, 2)


class _Boom:
    """Any use of it (a loader iterated, a model copied or called) is device work started too early."""

    def __getattr__(self, name):
        raise AssertionError(f"touched {name} before the arguments were checked")

    def __iter__(self):
        raise AssertionError("iterated the loader before the arguments were checked")


def test_consistency_step_and_targets_check_before_device_work():
    import afdm
    d = _diff(prediction="v")
    chain = d.ddim_timesteps(8)
    m, other = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="student is teacher"):
        afdm.ConsistencyStep(m, m, d, chain, 1e-4)
    for key, val in (("ema", afdm.EMA(0.9)), ("ema_model", other), ("ema_start", 0), ("t_sampler", "loss_second_moment"),
                     ("t_sampler", None)):
        with pytest.raises(ValueError, match=f"ConsistencyStep: {key} is not supported"):
            afdm.ConsistencyStep(_Boom(), other, d, chain, 1e-4, **{key: val})
    lv = _diff(prediction="v", variance="learned")
    with pytest.raises(ValueError, match="variance='learned'"):
        afdm.ConsistencyStep(_Boom(), other, lv, chain, 1e-4)
    with pytest.raises(ValueError, match="strictly decreasing"):
        afdm.ConsistencyStep(_Boom(), other, d, [3, 500], 1e-4)
    with pytest.raises(ValueError, match="target_beta"):
        afdm.ConsistencyStep(_Boom(), other, d, chain, 1e-4, target_beta=1.0)
    with pytest.raises(ValueError, match="sigma_data"):
        afdm.ConsistencyStep(_Boom(), other, d, chain, 1e-4, sigma_data=0.0)
    coef = d.consistency_coefficients()
    with pytest.raises(ValueError, match="variance='learned'"):
        lv.consistency_targets(_Boom(), _Boom(), torch.zeros(1, 3, 32, 32), torch.tensor([0]), chain, coef)
    with pytest.raises(ValueError, match=r"must lie in \[0, 8\)"):
        d.consistency_targets(_Boom(), _Boom(), torch.zeros(1, 3, 32, 32), torch.tensor([8]), chain, coef)
    with pytest.raises(ValueError, match="integer positions"):
        d.consistency_targets(_Boom(), _Boom(), torch.zeros(1, 3, 32, 32), torch.tensor([0.5]), chain, coef)


@pytest.mark.parametrize("steps,iters", [(0, 10), (1000, 10), (8, 0), (8.0, 10), (8, 2.5), (True, 10), (8, None)])
def test_consistency_distill_checks_its_arguments_first(steps, iters):
    import afdm
    with pytest.raises(ValueError, match="consistency_distill: "):
        afdm.consistency_distill(_Boom(), _diff(), _Boom(), steps, iters, 1e-4, "cuda")


def test_consistency_distill_rejects_reserved_keywords_and_reaches_the_model_otherwise():
    import afdm
    d = _diff()
    for key in ("ema", "ema_model", "ema_start", "t_sampler"):
        with pytest.raises(ValueError, match=f"consistency_distill: {key} is not supported"):
            afdm.consistency_distill(_Boom(), d, _Boom(), 8, 10, 1e-4, "cuda", **{key: None})
    with pytest.raises(ValueError, match="consistency_distill: target_beta"):
        afdm.consistency_distill(_Boom(), d, _Boom(), 8, 10, 1e-4, "cuda", target_beta=1.5)
    with pytest.raises(ValueError, match="variance='learned'"):
        afdm.consistency_distill(_Boom(), _diff(variance="learned"), _Boom(), 8, 10, 1e-4, "cuda")
    with pytest.raises(AssertionError, match="touched"):              # good arguments pass the checks and reach the model
        afdm.consistency_distill(_Boom(), d, _Boom(), 8, 10, 1e-4, "cuda")


def test_consistency_sample_checks_before_device_work():
    d = _diff()
    for steps in (0, 1000, [3, 500], [], [999, 999], 2.5, [1000], None):
        with pytest.raises(ValueError):
            d.consistency_sample(_Boom(), 2, 3, steps)
    with pytest.raises(ValueError, match="sigma_data"):
        d.consistency_sample(_Boom(), 2, 3, 2, sigma_data=-1.0)
    with pytest.raises(ValueError, match="timestep_scaling"):
        d.consistency_sample(_Boom(), 2, 3, [999], timestep_scaling=float("inf"))
    with pytest.raises(ValueError, match="variance='learned'"):
        _diff(variance="learned").consistency_sample(_Boom(), 2, 3, 2)
    with pytest.raises(TypeError):                                    # guidance is not offered
        d.consistency_sample(_Boom(), 2, 3, 2, cfg_scale=3.0)


@pytest.mark.parametrize("cfg", ({"steps": 8, "iters": 2}, {"steps": 8, "sample_steps": 2}, {"iters": 2, "sample_steps": 2},
                                 {"steps": 8, "iters": 2, "sample_steps": 2, "rounds": 1}, [8, 2, 2], {}))
def test_ddpm_run_validates_the_consistency_key_before_anything_else(cfg, tmp_path, monkeypatch):
    import afdm
    monkeypatch.chdir(tmp_path)
    params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1, "device": "cuda",
              "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(tmp_path / "absent.csv"), "f_kernel": 3,
              "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False, "gen_per_batch": 4, "gen_total": 4,
              "collage_n_per_image": 4, "collage_n": 4, "seed": 42, "prediction": "v", "consistency": cfg}
    with pytest.raises(ValueError, match="ddpm_run: consistency"):
        afdm.ddpm_run(params)
    assert not list(tmp_path.iterdir())                               # nothing was written


def test_ddpm_run_takes_one_of_distill_and_consistency(tmp_path, monkeypatch):
    import afdm
    monkeypatch.chdir(tmp_path)
    params = {"unet_v": 3, "dataset": "MNIST", "epochs": 1, "batchsize": 8, "image_size": 32, "image_channels": 1, "device": "cuda",
              "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(tmp_path / "absent.csv"), "f_kernel": 3,
              "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False, "gen_per_batch": 4, "gen_total": 4,
              "collage_n_per_image": 4, "collage_n": 4, "seed": 42, "prediction": "v",
              "consistency": {"steps": 8, "iters": 2, "sample_steps": 2}, "distill": {"start_steps": 4, "end_steps": 2, "iters": 2}}
    with pytest.raises(ValueError, match="distill and consistency both"):
        afdm.ddpm_run(params)
    assert not list(tmp_path.iterdir())
    assert afdm.tasks.consistency_path("/a/ckpt_X_3.pt", 8) == "/a/ckpt_X_3_consistency8.pt"
