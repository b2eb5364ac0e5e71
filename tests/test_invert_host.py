"""CPU-side tests of the real-image methods (DDIM inversion with fixed-point refinement, decode, SDEdit, interpolation): the
public signatures, `ddim_timesteps_from`, the levels `invert` climbs, the header's types of the five new entry points and their
argument checks (which return before any launch), and the argument checks of the methods (which raise before the model or a
device is touched)."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
ENTRY_POINTS = {"afd_ddim_invert_step": [P, P, P, I, I, P, L, P],
                "afd_ddim_invert_step_dev": [P, P, P, P, P, P, L, P],
                "afd_ddim_invert_step_cfg": [P, P, P, I, I, F, P, P, L, P],
                "afd_ddim_invert_step_cfg_dev": [P, P, P, P, P, F, P, P, L, P],
                "afd_slerp_rows": [P, P, P, P, L, L, L, P]}


def _diff(T=1000, img=32):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=img, device="cpu")


def _model(num_classes=None):
    import afdm
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3, **kw)


def _params(fn):
    return inspect.signature(fn).parameters


# ---- signatures ----------------------------------------------------------------------------------------------------------------
def test_public_signatures_and_defaults():
    import afdm
    from afdm import ops, tasks
    D = afdm.Diffusion
    assert list(_params(D.ddim_timesteps_from)) == ["self", "t0", "steps"]
    sp = _params(D.invert)
    assert list(sp) == ["self", "model", "images", "steps", "refine", "labels", "cfg_scale", "graph"]
    assert sp["refine"].default == 0 and sp["labels"].default is None and sp["cfg_scale"].default == 0.0 and sp["graph"].default is None
    assert sp["steps"].default is inspect.Parameter.empty
    sp = _params(D.decode)
    assert list(sp) == ["self", "model", "latents", "steps", "eta", "labels", "cfg_scale", "noise_source", "graph", "return_float"]
    assert sp["eta"].default == 0.0 and sp["labels"].default is None and sp["cfg_scale"].default == 0.0
    assert sp["noise_source"].default == "reference" and sp["graph"].default is None and sp["return_float"].default is False
    sp = _params(D.sdedit)
    assert list(sp) == ["self", "model", "images", "t0", "steps", "eta", "labels", "cfg_scale", "noise_source", "graph", "return_float"]
    assert sp["eta"].default == 0.0 and sp["labels"].default is None and sp["cfg_scale"].default == 0.0
    assert sp["noise_source"].default == "reference" and sp["graph"].default is None and sp["return_float"].default is False
    sp = _params(D.interpolate)
    assert list(sp) == ["self", "model", "a", "b", "weights", "steps", "refine", "labels", "cfg_scale", "graph", "return_float"]
    assert sp["refine"].default == 0 and sp["labels"].default is None and sp["cfg_scale"].default == 0.0
    assert sp["graph"].default is None and sp["return_float"].default is False
    for fn in (D.invert, D.decode, D.sdedit, D.interpolate):
        assert "sampler" not in _params(fn)
    sp = _params(D._ddim_loop)
    assert list(sp)[-1] == "start" and sp["start"].default is None
    sp = _params(afdm.reconstruct_results)
    assert list(sp) == ["model_data", "images", "n", "steps", "refine", "kw"] and sp["steps"].default == 50 and sp["refine"].default == 0
    assert sp["kw"].kind is inspect.Parameter.VAR_KEYWORD
    sp = _params(afdm.edit_results)
    assert list(sp) == ["model_data", "images", "t0", "kw"] and sp["kw"].kind is inspect.Parameter.VAR_KEYWORD
    assert tasks.reconstruct_results is afdm.reconstruct_results and tasks.edit_results is afdm.edit_results
    assert list(_params(ops.ddim_invert_step)) == ["x", "eps", "alpha_hat", "s", "u", "out"]
    assert list(_params(ops.ddim_invert_step_dev)) == ["x", "eps", "alpha_hat", "s_dev", "u_dev", "out"]
    assert list(_params(ops.ddim_invert_step_cfg)) == ["x", "eps2", "alpha_hat", "s", "u", "cfg_scale", "out", "out2"]
    assert list(_params(ops.ddim_invert_step_cfg_dev)) == ["x", "eps2", "alpha_hat", "s_dev", "u_dev", "cfg_scale", "out", "out2"]
    assert list(_params(ops.slerp)) == ["a", "b", "weights"]


def test_existing_sampler_signatures_are_unchanged():
    import afdm
    D = afdm.Diffusion
    assert list(_params(D.sample)) == ["self", "model", "n", "image_channels", "theta", "noise_source", "return_float", "graph",
                                       "labels", "cfg_scale", "steps", "eta", "sampler"]
    assert list(_params(D.revert)) == ["self", "model", "n", "image_channels", "noise_source", "graph", "steps", "eta", "sampler"]
    assert list(_params(D.inpaint)) == ["self", "model", "images", "mask", "steps", "eta", "labels", "cfg_scale", "jump_length",
                                        "jump_n_sample", "noise_source", "graph", "return_float"]
    sp = _params(D.sample)
    assert sp["steps"].default is None and sp["eta"].default == 0.0 and sp["sampler"].default is None and sp["graph"].default is None


# ---- the timesteps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,t0", [(1000, 999), (1000, 400), (1000, 7), (50, 20), (3, 1)])
def test_ddim_timesteps_from_is_the_closed_form(T, t0):
    d = _diff(T)
    for S in sorted({1, 2, 3, 7, t0} & set(range(1, t0 + 1))):
        taus = d.ddim_timesteps_from(t0, S)
        want = [t0] if S == 1 else [1 + (k * (t0 - 1)) // (S - 1) for k in range(S)][::-1]
        assert taus == want and all(type(t) is int for t in taus)
        assert taus[0] == t0 and len(taus) == S and all(a > b for a, b in zip(taus, taus[1:])) and taus[-1] >= 1
        if S > 1:
            assert taus[-1] == 1
        assert d.ddim_timesteps_from(np.int64(t0), np.int64(S)) == want
    assert d.ddim_timesteps_from(t0, t0) == list(range(t0, 0, -1))
    for S in sorted({1, 2, 3, 7, T - 1} & set(range(1, T))):
        assert d.ddim_timesteps_from(T - 1, S) == d.ddim_timesteps(S)


def test_ddim_timesteps_from_refusals():
    d = _diff()
    for t0, S in ((0, 1), (1000, 5), (-3, 1), (10, 11), (10, 0), (10, -1), (999, 1000)):
        with pytest.raises(ValueError, match="Diffusion.ddim_timesteps_from: needs 1 <= steps <= t0 <= 999"):
            d.ddim_timesteps_from(t0, S)
    for t0, S in ((10.0, 5), (10, 5.0), (True, 1), (10, True), (None, 3), (10, None), ("10", 3), (10, [3])):
        with pytest.raises(ValueError, match="Diffusion.ddim_timesteps_from: .* must be an int"):
            d.ddim_timesteps_from(t0, S)


@pytest.mark.parametrize("steps", [1, 2, 5, 50, 999, [999], [700, 350, 20], [999, 998, 1], np.array([500, 3])])
def test_invert_levels_are_the_samplers_pairs_reversed_and_swapped(steps):
    d = _diff()
    pairs = d._ddim_pairs(steps, 0.0)
    moves = d._invert_moves(steps)
    assert moves == [(tp, t) for t, tp in pairs][::-1]
    taus = [t for t, _ in pairs]
    levels = [0] + taus[::-1]
    assert moves == list(zip(levels, levels[1:]))
    assert moves[0][0] == 0 and moves[-1][1] == taus[0] and all(0 <= s < u <= 999 for s, u in moves)
    assert all(u >= 1 for _, u in moves)                             # the model is evaluated at u, never at 0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    Lb = lib()
    for name, want in ENTRY_POINTS.items():
        assert name in sigs, name
        restype, argtypes = sigs[name]
        assert restype is ctypes.c_int and argtypes == want, name
        assert hasattr(Lb.cdll, name) and callable(getattr(Lb, name))          # exported by the library, wrapped by the binding


def test_invert_step_entry_points_reject_bad_arguments_before_any_launch():
    import afdm
    lib = afdm.lib()
    E = afdm.AfdError
    # non-NULL but never dereferenced: every check returns before a launch.  Buffers 1 KiB apart in one arena; n = 64 floats uses
    # 256 bytes of each (512 of eps2).
    arena = (ctypes.c_float * (6 * 256))()
    x, eps, ah, out, out2, idx = (ctypes.addressof(arena) + 1024 * i for i in range(6))

    forms = {
        "afd_ddim_invert_step": lambda x=x, eps=eps, ah=ah, s=3, u=9, out=out, out2=None, n=64: lib.afd_ddim_invert_step(x, eps, ah, s, u, out, n, None),
        "afd_ddim_invert_step_dev": lambda x=x, eps=eps, ah=ah, s=idx, u=idx + 8, out=out, out2=None, n=64: lib.afd_ddim_invert_step_dev(x, eps, ah, s, u, out, n, None),
        "afd_ddim_invert_step_cfg": lambda x=x, eps=eps, ah=ah, s=3, u=9, out=out, out2=out2, n=64: lib.afd_ddim_invert_step_cfg(x, eps, ah, s, u, 3.0, out, out2, n, None),
        "afd_ddim_invert_step_cfg_dev": lambda x=x, eps=eps, ah=ah, s=idx, u=idx + 8, out=out, out2=out2, n=64: lib.afd_ddim_invert_step_cfg_dev(x, eps, ah, s, u, 3.0, out, out2, n, None),
    }
    for name, fn in forms.items():
        dev, cfg = name.endswith("_dev"), "_cfg" in name
        for arg in ("x", "eps", "ah", "out") + (("s", "u") if dev else ()):
            with pytest.raises(E, match=f"{name}: .*NULL"):
                fn(**{arg: None})
        for n in (0, -5):
            with pytest.raises(E, match=f"{name}: n must be positive"):
                fn(n=n)
        if not dev:
            for s, u in ((9, 9), (10, 9), (-1, 5), (0, 0), (5, -2)):
                with pytest.raises(E, match=f"{name}: need 0 <= s < u"):
                    fn(s=s, u=u)
        with pytest.raises(E, match=f"{name}: x_out and x_out2 must not overlap eps"):
            fn(out=eps)
        with pytest.raises(E, match=f"{name}: x_out and x_out2 must not overlap eps"):
            fn(out=eps + 4 * 63)
        if cfg:
            with pytest.raises(E, match=f"{name}: x_out and x_out2 must not overlap eps2"):
                fn(out=eps + 4 * 100)                             # inside the second half of eps2
            with pytest.raises(E, match=f"{name}: x_out and x_out2 must not overlap eps2"):
                fn(out2=eps + 4)
        with pytest.raises(E, match=f"{name}: x_out and x_out2 must each be x itself or apart"):
            fn(out=x + 4)


def test_slerp_entry_point_rejects_bad_arguments_before_any_launch():
    import afdm
    lib = afdm.lib()
    E = afdm.AfdError
    arena = (ctypes.c_float * (8 * 256))()
    a, b, w = (ctypes.addressof(arena) + 1024 * i for i in range(3))
    out = ctypes.addressof(arena) + 4096                           # 2 pairs x 3 weights x 64 floats = 1536 bytes

    def call(a=a, b=b, w=w, out=out, pairs=2, W=3, row=64):
        return lib.afd_slerp_rows(a, b, w, out, pairs, W, row, None)

    for arg in ("a", "b", "w", "out"):
        with pytest.raises(E, match="afd_slerp_rows: .*NULL"):
            call(**{arg: None})
    for kw in ({"pairs": 0}, {"W": 0}, {"row": 0}, {"pairs": -1}, {"W": -2}, {"row": -64}):
        with pytest.raises(E, match="afd_slerp_rows: pairs, W and row must be positive"):
            call(**kw)
    with pytest.raises(E, match="afd_slerp_rows: a row holds at most 12288"):
        call(row=12289)
    with pytest.raises(E, match="at most 2\\^31 - 1 output rows"):
        call(pairs=1 << 20, W=1 << 11)
    for kw in ({"a": a + 2}, {"out": out + 1}, {"w": w + 3}):
        with pytest.raises(E, match="4-byte aligned"):
            call(**kw)
    for kw in ({"out": a}, {"out": b + 4 * 100}, {"out": w + 8}, {"a": out + 1024}):
        with pytest.raises(E, match="afd_slerp_rows: out must not overlap"):
            call(**kw)


# ---- the methods' refusals -----------------------------------------------------------------------------------------------------------
def test_argument_errors_before_the_model_or_a_device_is_touched():
    d = _diff()
    m = _model()
    mk = _model(num_classes=4)
    img = torch.zeros(2, 1, 32, 32)
    bad_images = [(torch.zeros(2, 1, 16, 16), "shape"), (torch.zeros(1, 32, 32), "shape"), (torch.zeros(0, 1, 32, 32), "shape"),
                  (img.double(), "fp32"), (img.numpy(), "fp32")]
    bad_steps = [1000, 0, -3, [500, 999], [10, 10], [], [1000, 5], [5, 0], [5.0, 2.0], "abc", 2.5]
    calls = {
        "invert": lambda images=img, steps=5, **kw: d.invert(kw.pop("model", m), images, steps, **kw),
        "decode": lambda images=img, steps=5, **kw: d.decode(kw.pop("model", m), images, steps, **kw),
        "sdedit": lambda images=img, steps=5, **kw: d.sdedit(kw.pop("model", m), images, kw.pop("t0", 400), steps, **kw),
        "interpolate": lambda images=img, steps=5, **kw: d.interpolate(kw.pop("model", m), images, kw.pop("b", img),
                                                                       kw.pop("weights", [0.0, 0.5, 1.0]), steps, **kw),
    }
    for name, call in calls.items():
        for bad, what in bad_images:
            with pytest.raises(ValueError, match=f"Diffusion.{name}: .*{what}"):
                call(images=bad)
        for steps in bad_steps:
            if name == "sdedit" and isinstance(steps, int):
                continue                                            # (an int goes through ddim_timesteps_from: below)
            with pytest.raises(ValueError):
                call(steps=steps)
        with pytest.raises(ValueError, match=f"Diffusion.{name}: cfg_scale needs class labels"):
            call(cfg_scale=3.0)
        with pytest.raises(ValueError, match=f"Diffusion.{name}: labels were passed but the model has no label embedding"):
            call(labels=[0, 1])
        with pytest.raises(ValueError, match=f"Diffusion.{name}: expected 2 labels"):
            call(model=mk, labels=[0, 1, 2])
        with pytest.raises(ValueError, match=f"Diffusion.{name}: labels must be integers"):
            call(model=mk, labels=[0.5, 1.0])
        with pytest.raises(TypeError):
            call(sampler="dpmpp_2m")
    for name in ("invert", "interpolate"):
        for refine in (-1, 1.0, True, None, "2"):
            with pytest.raises(ValueError, match=f"Diffusion.{name}: refine must be an int >= 0"):
                calls[name](refine=refine)
    for name in ("decode", "sdedit"):
        with pytest.raises(ValueError, match="eta"):
            calls[name](eta=-0.5)
        with pytest.raises(ValueError, match=f"Diffusion.{name}: steps is required"):
            calls[name](steps=None)
    # decode: latents are named as such
    with pytest.raises(ValueError, match="Diffusion.decode: latents must have shape"):
        d.decode(m, torch.zeros(2, 1, 16, 16), 5)
    # sdedit: t0, and an explicit sequence that does not start there
    for t0 in (0, 1000, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="Diffusion.sdedit: t0 must be an int in \\[1, 999\\]"):
            calls["sdedit"](t0=t0)
    with pytest.raises(ValueError, match="Diffusion.sdedit: an explicit steps sequence must start at t0 = 400"):
        calls["sdedit"](steps=[300, 100, 1])
    with pytest.raises(ValueError, match="Diffusion.sdedit: an explicit steps sequence must start at t0 = 400"):
        calls["sdedit"](steps=[999, 400, 1])
    with pytest.raises(ValueError, match="Diffusion.ddim_timesteps_from"):
        calls["sdedit"](t0=3, steps=5)                              # more steps than levels below t0
    with pytest.raises(ValueError, match="Diffusion.ddim_timesteps_from"):
        calls["sdedit"](steps=0)
    # interpolate: b and the weights
    with pytest.raises(ValueError, match="Diffusion.interpolate: b must have shape"):
        calls["interpolate"](b=torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError, match="Diffusion.interpolate: a and b must have one shape"):
        calls["interpolate"](b=torch.zeros(3, 1, 32, 32))
    for weights in ([], [[0.0, 1.0]], 0.5, [0.0, float("nan")], [float("inf")], ["a"], None, torch.zeros(2, 2)):
        with pytest.raises(ValueError, match="Diffusion.interpolate: weights must be a non-empty 1-D sequence of finite numbers"):
            calls["interpolate"](weights=weights)
    # a learned-variance process refuses a model with the wrong number of output channels, as `sample` does
    import afdm
    dl = afdm.Diffusion(noise_steps=1000, img_size=32, device="cpu", variance="learned")
    with pytest.raises(ValueError, match="Diffusion.invert: the model emits 1 channels"):
        dl.invert(m, img, 5)
    assert m.training and m._t_range is None and mk.training and mk._t_range is None


def test_results_wrappers_check_their_arguments_before_the_checkpoint_is_read():
    import afdm
    px = torch.zeros(4, 1, 32, 32, dtype=torch.uint8)
    data = {"modelpath": "/nonexistent/checkpoint.pt"}               # never read: the checks come first
    for n in (0, 5, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="reconstruct_results: n must be an int in \\[1, 4\\]"):
            afdm.reconstruct_results(data, px, n)
    for images in (px.float(), px[0], px.numpy().astype(np.float32)):
        with pytest.raises(ValueError, match="reconstruct_results: images must be a DeviceDataset or"):
            afdm.reconstruct_results(data, images, 1)
