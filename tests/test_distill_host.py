"""Progressive distillation, host side: the level tables of a teacher's chain, halving, the step-index draw, the truncated-SNR
weights, progressive_distill's argument errors and the C ABI of the two target kernels.  No GPU (the kernels, the step and the
loop are checked in test_gpu_distill.py)."""
import ctypes

import pytest
import torch

P, L, I = ctypes.c_void_p, ctypes.c_long, ctypes.c_int


def _diff(T=1000, **kw):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu", **kw)


def test_distill_levels_are_the_slices_of_the_chain():
    d = _diff()
    chain = d.ddim_timesteps(8)
    levels = chain + [0]
    t, t_mid, t_prev = d.distill_levels(chain)
    for got, want in ((t, levels[0:-1:2]), (t_mid, levels[1::2]), (t_prev, levels[2::2])):
        assert got.dtype == torch.long and not got.is_cuda and got.tolist() == want
    assert t.tolist() == [999, 713, 428, 143] and t_prev.tolist()[-1] == 0 and t_mid.tolist()[-1] == 1
    assert torch.equal(t[1:], t_prev[:-1])                            # student step k + 1 starts where step k ends


@pytest.mark.parametrize("chain", ([999, 500, 3], [999], [3, 500], [500, 500], [1000, 3], [5, 0], [], 8, [999.0, 1.0]))
def test_distill_levels_rejects_bad_chains(chain):
    with pytest.raises(ValueError):
        _diff().distill_levels(chain)


def test_distill_levels_needs_a_decreasing_alpha_hat():
    d = _diff(10)
    assert d.distill_levels([9, 5, 3, 1])[0].tolist() == [9, 3]
    d.alpha_hat = d.alpha_hat.clone()
    d.alpha_hat[5] = d.alpha_hat[9]                                  # the level at t = 5 is no cleaner than the one at t = 9
    with pytest.raises(ValueError, match="alpha_hat must strictly decrease"):
        d.distill_levels([9, 5, 3, 1])


@pytest.mark.parametrize("T,N,R", [(1000, 4, 1), (1000, 4, 3), (1000, 1, 5), (300, 2, 7), (12, 2, 1)])
def test_halve_chain_keeps_the_start_and_the_order(T, N, R):
    import afdm
    d = _diff(T)
    chain = d.ddim_timesteps(N * 2 ** R)
    for _ in range(R):
        d.distill_levels(chain)                                      # every round's chain is a valid teacher chain
        assert afdm.Diffusion.halve_chain(chain) == chain[0::2]
        chain = d.halve_chain(chain)
    assert len(chain) == N and chain[0] == T - 1 and chain[-1] >= 1
    assert all(a > b for a, b in zip(chain, chain[1:]))


def test_sample_distill_steps_draws_like_randint():
    import afdm
    torch.manual_seed(7)
    want = torch.randint(0, 4, (16,))
    after = torch.rand(3)
    torch.manual_seed(7)
    got = afdm.Diffusion.sample_distill_steps(16, 4)
    assert got.dtype == torch.long and torch.equal(got, want) and torch.equal(torch.rand(3), after)
    assert int(got.min()) >= 0 and int(got.max()) < 4


@pytest.mark.parametrize("schedule", ("linear", "cosine"))
def test_truncated_snr_weights(schedule):
    import afdm
    assert afdm.Diffusion.LOSS_WEIGHTINGS == ("min_snr", "truncated_snr")
    a = _diff(schedule=schedule).alpha_hat.double()
    snr = a / (1.0 - a)
    trunc = torch.clamp(snr, min=1.0)
    want = {"eps": trunc / snr, "x0": trunc, "v": trunc / (snr + 1.0)}
    for pred in ("eps", "v", "x0"):
        d = _diff(schedule=schedule, prediction=pred)
        w = d.snr_weights("truncated_snr")
        assert w.dtype == torch.float64 and tuple(w.shape) == (1000,) and torch.equal(w, want[pred])
        assert torch.equal(w, d.snr_weights("truncated_snr", gamma=None))             # snr_gamma is ignored for it
        # min_snr is what it was: the parent's expression
        clipped = torch.clamp(snr, max=5.0)
        parent = {"eps": clipped / snr, "x0": clipped, "v": clipped / (snr + 1.0)}[pred]
        assert torch.equal(d.snr_weights(), parent) and torch.equal(d.snr_weights("min_snr", 5.0), parent)
        with pytest.raises(ValueError, match="gamma"):
            d.snr_weights("min_snr", gamma=0)
        for bad in ("p2", None, "max_snr"):
            with pytest.raises(ValueError, match="snr_weights: unknown kind"):
                d.snr_weights(bad)
    # the x0 error's weight is max(snr, 1) in every parametrisation: 1 at the noisy end for v, never below 1 for x0
    assert float(want["x0"].min()) == 1.0 and float(want["eps"].min()) == 1.0 and float(want["v"].max()) <= 1.0


class _Boom:
    """Any use of it (a loader iterated, a model copied or called) is device work started too early."""

    def __getattr__(self, name):
        raise AssertionError(f"progressive_distill touched {name} before checking its arguments")

    def __iter__(self):
        raise AssertionError("progressive_distill iterated the loader before checking its arguments")


@pytest.mark.parametrize("start,end", [(12, 5), (8, 8), (4, 8), (12, 4), (1024, 512), (8, 0), (8.0, 4), (True, 1)])
def test_progressive_distill_checks_its_arguments_first(start, end):
    import afdm
    with pytest.raises(ValueError, match="progressive_distill: "):
        afdm.progressive_distill(_Boom(), _diff(), _Boom(), start, end, 10, 1e-4, "cuda")


def test_progressive_distill_accepts_the_largest_chain_only_up_to_T_minus_1():
    import afdm
    d = _diff(9)                                                      # T - 1 = 8 is allowed, 16 is not
    with pytest.raises(ValueError, match=r"start_steps must lie in \[2, 8\]"):
        afdm.progressive_distill(_Boom(), d, _Boom(), 16, 4, 1, 1e-4, "cuda")
    with pytest.raises(AssertionError, match="touched"):             # 8 passes the checks and reaches the model
        afdm.progressive_distill(_Boom(), d, _Boom(), 8, 4, 1, 1e-4, "cuda")


def test_header_declares_and_library_exports_the_distill_entry_points():
    import afdm
    from afdm._lib import LIBPATH, parse_header
    sigs = parse_header()
    assert sigs["afd_distill_mid"] == (ctypes.c_int, [P, P, P, P, P, I, P, L, L, P])
    assert sigs["afd_distill_target"] == (ctypes.c_int, [P, P, P, P, P, P, P, I, P, P, L, L, P])
    cdll = ctypes.CDLL(LIBPATH)
    for name in ("afd_distill_mid", "afd_distill_target"):
        assert hasattr(cdll, name), f"{name} declared in include/afd.h but not exported"
    assert callable(afdm.ops.distill_mid) and callable(afdm.ops.distill_target)
    assert afdm.DistillStep is afdm.training.DistillStep and afdm.progressive_distill is afdm.training.progressive_distill


def test_distill_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_float * 4096)()
    at = lambda i: ctypes.addressof(buf) + 4 * i
    # B = 2, chw = 8: 16 floats per tensor, 2 int64 (4 floats) per timestep tensor
    mid = [at(0), at(64), at(128), at(192), at(256), 1, at(320), 2, 8, None]
    tgt = [at(0), at(64), at(384), at(128), at(192), at(448), at(256), 1, at(320), at(512), 2, 8, None]
    for fn, args, ptrs, ikind, idims in ((lib.afd_distill_mid, mid, (0, 1, 2, 3, 4, 6), 5, (7, 8)),
                                         (lib.afd_distill_target, tgt, (0, 1, 2, 3, 4, 5, 6, 8, 9), 7, (10, 11))):
        name = fn.__name__
        for i in ptrs:
            bad = list(args)
            bad[i] = None
            with pytest.raises(afdm.AfdError, match=f"{name}: .*NULL"):
                fn(*bad)
        for k in (-1, 3, 7):
            bad = list(args)
            bad[ikind] = k
            with pytest.raises(afdm.AfdError, match=f"{name}: kind must be"):
                fn(*bad)
        for i in idims:
            for v in (0, -4):
                bad = list(args)
                bad[i] = v
                with pytest.raises(afdm.AfdError, match=f"{name}: .*positive"):
                    fn(*bad)
    # an output may be an input itself, never a shifted view of one, a timestep tensor or the other output
    for i_out, i_in in ((6, 0), (6, 1)):
        bad = list(mid)
        bad[i_out] = mid[i_in] + 4
        with pytest.raises(afdm.AfdError, match="afd_distill_mid: z_mid must be out1 or z_t itself or apart"):
            lib.afd_distill_mid(*bad)
    bad = list(mid)
    bad[6] = mid[3]
    with pytest.raises(afdm.AfdError, match="afd_distill_mid: .*must not overlap t or t_mid"):
        lib.afd_distill_mid(*bad)
    for i_out in (8, 9):
        for i_in in (0, 1, 2):
            bad = list(tgt)
            bad[i_out] = tgt[i_in] + 8
            with pytest.raises(afdm.AfdError, match="afd_distill_target: x_tilde and eps_tilde must each be"):
                lib.afd_distill_target(*bad)
        bad = list(tgt)
        bad[i_out] = tgt[5]
        with pytest.raises(afdm.AfdError, match="afd_distill_target: x_tilde and eps_tilde must each be"):
            lib.afd_distill_target(*bad)
    bad = list(tgt)
    bad[9] = bad[8]
    with pytest.raises(afdm.AfdError, match="afd_distill_target: x_tilde and eps_tilde must each be"):
        lib.afd_distill_target(*bad)
    # the torch-level wrappers: host tensors, unknown kinds
    x = torch.zeros(2, 3, 4, 4)
    t, ah = torch.tensor([2, 2]), torch.full((10,), 0.5)
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.distill_mid(x, x, t, t, ah, "v")
    with pytest.raises(afdm.AfdError, match="HIP device"):
        afdm.ops.distill_target(x, x, x, t, t, t, ah, "x0")
    with pytest.raises(afdm.AfdError, match="unknown prediction 'velocity'"):
        afdm.ops.distill_mid(x, x, t, t, ah, "velocity")


def test_distill_step_and_targets_check_before_device_work():
    import afdm
    d = _diff(prediction="v")
    m = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="student is teacher"):
        afdm.DistillStep(m, m, d, d.ddim_timesteps(8), 1e-4)
    with pytest.raises(ValueError, match="even number of steps"):
        afdm.DistillStep(m, torch.nn.Linear(2, 2), d, d.ddim_timesteps(7), 1e-4)
    lv = _diff(prediction="v", variance="learned")
    with pytest.raises(ValueError, match="variance='learned'"):
        afdm.DistillStep(m, torch.nn.Linear(2, 2), lv, lv.ddim_timesteps(8), 1e-4)
    with pytest.raises(ValueError, match="variance='learned'"):
        lv.distill_targets(m, torch.zeros(1, 3, 32, 32), torch.tensor([0]), lv.ddim_timesteps(8))
    with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
        d.distill_targets(m, torch.zeros(1, 3, 32, 32), torch.tensor([4]), d.ddim_timesteps(8))
