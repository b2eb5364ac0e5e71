"""CPU-side tests of inpainting (RePaint): the resampling schedule against the definition restated here, the argument checks
of Diffusion.inpaint (which raise before any device work), and the C ABI of the nine new entry points with their own checks
(which return before any launch)."""
import ctypes
import inspect
import math

import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float


def _diff(T=1000, img=32):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=img, device="cpu")


def _moves_restated(chain, j, r):
    """RePaint's get_schedule_jump (Lugmayr et al. 2022), re-indexed onto chain positions, as the issue defines it."""
    levels, S = list(chain) + [0], len(chain)
    left = {p: r - 1 for p in range(j, S) if (S - 1 - p) % j == 0}
    moves, p = [], 0
    while p < S:
        moves.append((levels[p], levels[p + 1]))
        p += 1
        if left.get(p, 0) > 0:
            left[p] -= 1
            moves.append((levels[p], levels[p - j]))
            p -= j
    return moves


def _chains():
    d = _diff()
    yield list(range(999, 0, -1))
    for S in (1, 2, 7, 50, 250):
        yield d.ddim_timesteps(S)
    yield [900, 40, 3]


def test_repaint_moves_equal_the_restated_schedule():
    import afdm
    for chain in _chains():
        for j in (1, 2, 3, 10, 20):
            for r in (1, 2, 3, 10):
                got = afdm.Diffusion.repaint_moves(chain, j, r)
                assert got == _moves_restated(chain, j, r), (len(chain), j, r)


def test_repaint_moves_count_at_the_papers_setting():
    import afdm
    chain = _diff().ddim_timesteps(250)
    for r in (1, 2, 5, 10):
        moves = afdm.Diffusion.repaint_moves(chain, 10, r)
        down = [m for m in moves if m[0] > m[1]]
        up = [m for m in moves if m[0] < m[1]]
        assert len(down) == 250 + 24 * (r - 1) * 10
        assert len(up) == 24 * (r - 1)
    assert len([m for m in afdm.Diffusion.repaint_moves(chain, 10, 10) if m[0] > m[1]]) == 2410   # RePaint's 2410 forwards


def test_repaint_moves_without_jumps_is_the_plain_chain():
    import afdm
    d = _diff()
    for chain in _chains():
        for j in (1, 5, 10, 10000):
            assert afdm.Diffusion.repaint_moves(chain, j, 1) == list(zip(chain, chain[1:] + [0]))
    assert afdm.Diffusion.repaint_moves(d.ddim_timesteps(50), 10, 1) == d._ddim_pairs(50, 0.0)


def test_repaint_moves_reach_every_level_and_end_at_zero():
    import afdm
    for chain in _chains():
        for j, r in ((1, 3), (2, 2), (10, 10), (3, 5)):
            moves = afdm.Diffusion.repaint_moves(chain, j, r)
            levels = chain + [0]
            assert moves[0][0] == chain[0] and moves[-1] == (chain[-1], 0)
            assert [tp for _, tp in moves].count(0) == 1                           # the chain's last step runs once
            for (a, b), (c, _) in zip(moves, moves[1:]):
                assert b == c                                                       # moves are contiguous
            pos = {v: k for k, v in enumerate(levels)}
            for a, b in moves:
                assert a in pos and b in pos
                assert pos[b] == pos[a] + 1 or (b > a and pos[a] - pos[b] == j)  # one step down, or j positions up
            assert set(levels) <= {v for m in moves for v in m}


def test_repaint_moves_reject_bad_arguments():
    import afdm
    chain = list(range(10, 0, -1))
    for j, r in ((0, 1), (1, 0), (-2, 3), (2.0, 2), (2, 2.5), (True, 2), (2, None), ("3", 2)):
        with pytest.raises(ValueError, match="jump_"):
            afdm.Diffusion.repaint_moves(chain, j, r)
    for bad in ([], [3, 3, 1], [1, 2], [2, 1, 0]):
        with pytest.raises(ValueError, match="chain"):
            afdm.Diffusion.repaint_moves(bad, 2, 2)


def _model(num_classes=None):
    import afdm
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3, **kw)


def test_inpaint_argument_errors_before_any_device_work():
    d = _diff()
    m = _model()
    img = torch.zeros(2, 1, 32, 32)
    ok = torch.ones(2, 1, 32, 32)
    with pytest.raises(ValueError, match="0 or 1"):
        d.inpaint(m, img, torch.full((1, 1, 32, 32), 0.5))
    with pytest.raises(ValueError, match="0 or 1"):
        d.inpaint(m, img, torch.tensor([0, 1, 2]).repeat(11)[:32])
    with pytest.raises(ValueError, match="0 or 1"):
        d.inpaint(m, img, torch.full((32,), float("nan")))
    with pytest.raises(ValueError, match="broadcast"):
        d.inpaint(m, img, torch.ones(3, 1, 32, 32))
    with pytest.raises(ValueError, match="broadcast"):
        d.inpaint(m, img, torch.ones(1, 1, 1, 32, 32))
    with pytest.raises(ValueError, match="broadcast"):
        d.inpaint(m, img, torch.ones(16, 16))
    with pytest.raises(ValueError, match="shape"):
        d.inpaint(m, torch.zeros(2, 1, 16, 16), torch.ones(1))
    with pytest.raises(ValueError, match="shape"):
        d.inpaint(m, torch.zeros(1, 32, 32), torch.ones(1))
    with pytest.raises(ValueError, match="fp32"):
        d.inpaint(m, img.double(), ok)
    with pytest.raises(ValueError, match="fp32"):
        d.inpaint(m, img.numpy(), ok)
    for kw in ({"jump_length": 0}, {"jump_n_sample": 0}, {"jump_length": 2.0}, {"jump_n_sample": True}):
        with pytest.raises(ValueError, match="jump_"):
            d.inpaint(m, img, ok, **kw)
    with pytest.raises(ValueError, match="eta applies to the DDIM sampler"):
        d.inpaint(m, img, ok, eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        d.inpaint(m, img, ok, steps=50, eta=-1.0)
    with pytest.raises(ValueError):
        d.inpaint(m, img, ok, steps=1000)
    with pytest.raises(ValueError, match="cfg_scale needs class labels"):
        d.inpaint(m, img, ok, cfg_scale=3.0)
    with pytest.raises(ValueError, match="label embedding"):
        d.inpaint(m, img, ok, labels=[0, 1])
    with pytest.raises(ValueError, match="expected 2 labels"):
        d.inpaint(_model(num_classes=4), img, ok, labels=[0, 1, 2])
    assert m.training and m._t_range is None


def test_inpaint_public_signature():
    import afdm
    sp = inspect.signature(afdm.Diffusion.inpaint).parameters
    assert list(sp) == ["self", "model", "images", "mask", "steps", "eta", "labels", "cfg_scale", "jump_length", "jump_n_sample",
                        "noise_source", "graph", "return_float"]
    assert sp["steps"].default is None and sp["eta"].default == 0.0 and sp["jump_length"].default == 10
    assert sp["jump_n_sample"].default == 1 and sp["noise_source"].default == "reference" and sp["graph"].default is None
    assert callable(afdm.inpaint_results)


def test_header_declares_and_types_the_inpaint_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_denoise_step_masked"] == (I, [P, P, P, P, P, P, P, P, I, P, L, P])
    assert sigs["afd_denoise_step_masked_dev"] == (I, [P, P, P, P, P, P, P, P, P, P, L, P])
    assert sigs["afd_denoise_step_masked_cfg"] == (I, [P, P, P, P, P, P, P, P, I, F, P, P, L, P])
    assert sigs["afd_denoise_step_masked_cfg_dev"] == (I, [P, P, P, P, P, P, P, P, P, F, P, P, L, P])
    assert sigs["afd_ddim_step_masked"] == (I, [P, P, P, P, P, P, I, I, F, P, L, P])
    assert sigs["afd_ddim_step_masked_dev"] == (I, [P, P, P, P, P, P, P, P, F, P, L, P])
    assert sigs["afd_ddim_step_masked_cfg"] == (I, [P, P, P, P, P, P, I, I, F, F, P, P, L, P])
    assert sigs["afd_ddim_step_masked_cfg_dev"] == (I, [P, P, P, P, P, P, P, P, F, F, P, P, L, P])
    assert sigs["afd_renoise"] == (I, [P, P, P, I, I, P, L, P])


def test_inpaint_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    E = afdm.AfdError
    for name, args in (("afd_denoise_step_masked", (None,) * 8 + (5, None, 8, None)),
                       ("afd_denoise_step_masked_dev", (None,) * 10 + (8, None)),
                       ("afd_denoise_step_masked_cfg", (None,) * 8 + (5, 3.0, None, None, 8, None)),
                       ("afd_denoise_step_masked_cfg_dev", (None,) * 9 + (3.0, None, None, 8, None)),
                       ("afd_ddim_step_masked", (None,) * 6 + (5, 1, 0.0, None, 8, None)),
                       ("afd_ddim_step_masked_dev", (None,) * 8 + (0.0, None, 8, None)),
                       ("afd_ddim_step_masked_cfg", (None,) * 6 + (5, 1, 0.0, 3.0, None, None, 8, None)),
                       ("afd_ddim_step_masked_cfg_dev", (None,) * 8 + (0.0, 3.0, None, None, 8, None)),
                       ("afd_renoise", (None, None, None, 1, 5, None, 8, None))):
        with pytest.raises(E, match=f"{name}: .*NULL"):
            getattr(lib, name)(*args)
    # non-NULL but never dereferenced: each check returns before a launch.  q, x0 and mask are distinct buffers.
    buf, b0, bm = (ctypes.c_float * 64)(), (ctypes.c_float * 64)(), (ctypes.c_uint8 * 64)()
    q, x0, mk = ctypes.addressof(buf), ctypes.addressof(b0), ctypes.addressof(bm)
    # n <= 0
    with pytest.raises(E, match="afd_denoise_step_masked: n must be positive"):
        lib.afd_denoise_step_masked(q, q, q, x0, mk, q, q, q, 5, q, 0, None)
    with pytest.raises(E, match="afd_denoise_step_masked_dev: n must be positive"):
        lib.afd_denoise_step_masked_dev(q, q, q, x0, mk, q, q, q, q, q, -4, None)
    with pytest.raises(E, match="afd_ddim_step_masked_cfg_dev: n must be positive"):
        lib.afd_ddim_step_masked_cfg_dev(q, q, q, x0, mk, q, q, q, 0.0, 3.0, q, None, 0, None)
    with pytest.raises(E, match="afd_renoise: n must be positive"):
        lib.afd_renoise(q, q, q, 1, 5, q, 0, None)
    # the step order
    for i in (0, -3):
        with pytest.raises(E, match=r"afd_denoise_step_masked: need i >= 1"):
            lib.afd_denoise_step_masked(q, q, q, x0, mk, q, q, q, i, q, 8, None)
        with pytest.raises(E, match=r"afd_denoise_step_masked_cfg: need i >= 1"):
            lib.afd_denoise_step_masked_cfg(q, q, q, x0, mk, q, q, q, i, 3.0, q, None, 8, None)
    for t, tp in ((5, 5), (5, 7), (5, -1), (0, 0)):
        with pytest.raises(E, match=r"afd_ddim_step_masked: need 0 <= t_prev < t"):
            lib.afd_ddim_step_masked(q, q, q, x0, mk, q, t, tp, 0.0, q, 8, None)
        with pytest.raises(E, match=r"afd_ddim_step_masked_cfg: need 0 <= t_prev < t"):
            lib.afd_ddim_step_masked_cfg(q, q, q, x0, mk, q, t, tp, 0.0, 3.0, q, None, 8, None)
    for a, b in ((5, 5), (5, 1), (-1, 3)):
        with pytest.raises(E, match=r"afd_renoise: need 0 <= t_from < t_to"):
            lib.afd_renoise(q, q, q, a, b, q, 8, None)
    # eta
    with pytest.raises(E, match="afd_ddim_step_masked: eta"):
        lib.afd_ddim_step_masked(q, q, q, x0, mk, q, 5, 1, -0.5, q, 8, None)
    with pytest.raises(E, match="afd_ddim_step_masked_dev: eta"):
        lib.afd_ddim_step_masked_dev(q, q, q, x0, mk, q, q, q, float("nan"), q, 8, None)
    with pytest.raises(E, match="afd_ddim_step_masked_cfg: eta"):
        lib.afd_ddim_step_masked_cfg(q, q, q, x0, mk, q, 5, 1, -1.0, 3.0, q, None, 8, None)
    with pytest.raises(E, match="afd_ddim_step_masked_cfg_dev: eta"):
        lib.afd_ddim_step_masked_cfg_dev(q, q, q, x0, mk, q, q, q, -1.0, 3.0, q, None, 8, None)
    # the known region needs the noise whenever t_prev > 0
    with pytest.raises(E, match="afd_denoise_step_masked: noise must not be NULL"):
        lib.afd_denoise_step_masked(q, q, None, x0, mk, q, q, q, 2, q, 8, None)
    with pytest.raises(E, match="afd_ddim_step_masked_cfg: noise must not be NULL"):
        lib.afd_ddim_step_masked_cfg(q, q, None, x0, mk, q, 5, 1, 0.0, 3.0, q, None, 8, None)
    # x0 and mask must not overlap the outputs
    with pytest.raises(E, match="afd_denoise_step_masked: x0 and mask must not overlap"):
        lib.afd_denoise_step_masked(q, q, q, q, mk, q, q, q, 5, q, 8, None)
    with pytest.raises(E, match="afd_ddim_step_masked: x0 and mask must not overlap"):
        lib.afd_ddim_step_masked(q, q, q, x0, q + 8, q, 5, 1, 0.0, q, 8, None)
    with pytest.raises(E, match="afd_ddim_step_masked_cfg: x0 and mask must not overlap"):
        lib.afd_ddim_step_masked_cfg(q, q, q, x0, mk, q, 5, 1, 0.0, 3.0, q, x0 + 4, 8, None)
