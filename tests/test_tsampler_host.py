"""Loss-aware timestep sampling, host side: the C ABI's new entry points, argument validation, and the fp64 numpy restatement
of DESIGN.md section 6m (`Oracle`), checked here against two hand-worked cases.  tests/test_gpu_tsampler.py gates the device
code on that restatement."""
import ctypes
import math

import numpy as np
import pytest

ENTRY_POINTS = ("afd_loss_rows", "afd_lvar_loss_rows", "afd_tsampler_tick", "afd_tsampler_draw", "afd_lvar_loss_fwd_tw",
                "afd_lvar_loss_bwd_tw")


class Oracle:
    """The sampler's semantics in numpy fp64.  State: hist (T, H), count (T,).  lo = 1, n = T - 1."""

    def __init__(self, T, H=10, uniform_prob=0.001, w_base=None, lo=1):
        self.T, self.H, self.up, self.lo, self.n = T, H, float(uniform_prob), lo, T - lo
        self.hist = np.zeros((T, H), dtype=np.float64)
        self.count = np.zeros(T, dtype=np.int32)
        self.w_base = np.ones(T, dtype=np.float32) if w_base is None else np.asarray(w_base, dtype=np.float32)
        self.refresh()

    def update(self, t, rows):
        for tb, l in zip(np.asarray(t).tolist(), np.asarray(rows, dtype=np.float64).tolist()):      # batch order
            if not math.isfinite(l):
                continue
            if self.count[tb] == self.H:
                self.hist[tb, :-1] = self.hist[tb, 1:].copy()
                self.hist[tb, -1] = l
            else:
                self.hist[tb, self.count[tb]] = l
                self.count[tb] += 1
        self.refresh()

    def refresh(self):
        lo, n, T = self.lo, self.n, self.T
        self.warm = bool(np.all(self.count[lo:] == self.H))
        q = np.sqrt(np.mean(self.hist[lo:] ** 2, axis=1))
        p, iw = np.zeros(T), np.ones(T)
        if self.warm and q.sum() != 0:
            p[lo:] = (q / q.sum()) * (1.0 - self.up) + self.up / n
            iw[lo:] = 1.0 / (n * p[lo:])
        else:
            p[lo:] = 1.0 / n
        c = np.cumsum(p[lo:])
        c = c / c[-1]
        c[-1] = 1.0
        self.prob, self.iw, self.cdf = p, iw, c
        self.wtab = (self.w_base.astype(np.float64) * iw).astype(np.float32)
        self.vwtab = iw.astype(np.float32)

    def draw(self, u):
        k = np.searchsorted(self.cdf, np.asarray(u, dtype=np.float64), side="right")
        return self.lo + np.minimum(k, self.n - 1)

    def step_loss(self, t, rows):
        """L = (1 / B) sum_b iw[t_b] l_b"""
        t = np.asarray(t)
        return float(np.mean(self.iw[t] * np.asarray(rows, dtype=np.float64)))


# ---- the oracle against two hand-worked cases: T = 4, H = 2 ------------------------------------------------------------------------
def test_oracle_before_warm_up_by_hand():
    o = Oracle(4, H=2, uniform_prob=0.2, w_base=[1.0, 0.5, 2.0, 4.0])
    # t = 1 takes 9, 1 and then 7: its history is full at the third, shifts left and ends as [1, 7]; the NaN row is skipped,
    # so t = 3 has seen nothing and t = 2 one value
    o.update([1, 2, 1, 3, 1], [9.0, 2.0, 1.0, float("nan"), 7.0])
    assert o.hist.tolist() == [[0.0, 0.0], [1.0, 7.0], [2.0, 0.0], [0.0, 0.0]]
    assert o.count.tolist() == [0, 2, 1, 0]
    assert not o.warm
    assert o.prob.tolist() == [0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0]
    assert np.allclose(o.cdf, [1.0 / 3.0, 2.0 / 3.0, 1.0], rtol=1e-15, atol=0) and o.cdf[-1] == 1.0
    assert o.iw.tolist() == [1.0, 1.0, 1.0, 1.0]
    assert o.wtab.tolist() == [1.0, 0.5, 2.0, 4.0] and o.vwtab.tolist() == [1.0, 1.0, 1.0, 1.0]      # exactly the base weights
    assert o.draw([0.0, 0.33, 0.34, 0.67, 1.0 - 2.0 ** -53]).tolist() == [1, 1, 2, 3, 3]


def test_oracle_after_warm_up_by_hand():
    o = Oracle(4, H=2, uniform_prob=0.2, w_base=[1.0, 0.5, 2.0, 4.0])
    o.update([1, 2, 1, 3, 1], [9.0, 2.0, 1.0, float("nan"), 7.0])
    o.update([3, 2, 3], [1.0, 2.0, 1.0])
    assert o.hist.tolist() == [[0.0, 0.0], [1.0, 7.0], [2.0, 2.0], [1.0, 1.0]] and o.count.tolist() == [0, 2, 2, 2]
    assert o.warm
    # q = sqrt(mean of squares) = 5, 2, 1: sum 8; p = (q / 8) 0.8 + 0.2 / 3; iw = 1 / (3 p)
    p = [0.0, 0.5 + 0.2 / 3.0, 0.2 + 0.2 / 3.0, 0.1 + 0.2 / 3.0]
    assert np.allclose(o.prob, p, rtol=1e-15, atol=0)
    assert abs(o.prob.sum() - 1.0) < 1e-15
    assert np.allclose(o.iw, [1.0, 1.0 / 1.7, 1.0 / 0.8, 1.0 / 0.5], rtol=1e-15, atol=0)
    assert np.allclose(o.cdf, [p[1], p[1] + p[2], 1.0], rtol=1e-15, atol=0) and o.cdf[-1] == 1.0
    assert np.allclose(o.wtab, [1.0, 0.5 / 1.7, 2.0 / 0.8, 4.0 / 0.5], rtol=1e-7, atol=0)
    assert np.allclose(o.vwtab, [1.0, 1.0 / 1.7, 1.25, 2.0], rtol=1e-7, atol=0)
    assert o.draw([0.0, 0.56, 0.57, 0.83, 0.84, 1.0 - 2.0 ** -53]).tolist() == [1, 1, 2, 2, 3, 3]
    # the importance-weighted loss of a batch: (1 / B) sum iw[t_b] l_b
    assert math.isclose(o.step_loss([1, 3], [1.7, 3.0]), (1.0 + 6.0) / 2.0, rel_tol=1e-15)
    # an all-zero history is warm and falls back to the uniform distribution
    z = Oracle(4, H=2)
    z.count[1:] = 2
    z.refresh()
    assert z.warm and z.prob.tolist() == [0.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0] and z.iw.tolist() == [1.0] * 4


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_new_entry_points():
    from afdm import lib
    from afdm._lib import parse_header
    sigs = parse_header()
    L = lib()
    vp, lg, db, it = ctypes.c_void_p, ctypes.c_long, ctypes.c_double, ctypes.c_int
    want = {
        "afd_loss_rows": [vp] * 6 + [it, vp, lg, lg, vp],
        "afd_lvar_loss_rows": [vp] * 9 + [it, db, vp, lg, lg, vp],
        "afd_tsampler_tick": [vp, vp, lg, vp, vp, lg, lg, lg, db] + [vp] * 7,
        "afd_tsampler_draw": [vp, vp, lg, lg, vp, lg, vp],
        "afd_lvar_loss_fwd_tw": [vp] * 10 + [it, db, vp, vp, vp, lg, lg, vp],
        "afd_lvar_loss_bwd_tw": [vp] * 10 + [it, db, vp, vp, lg, lg, vp],
    }
    assert set(want) == set(ENTRY_POINTS)
    for name in ENTRY_POINTS:
        assert name in sigs, name
        restype, argtypes = sigs[name]
        assert restype is ctypes.c_int and argtypes == want[name], name
        assert hasattr(L.cdll, name) and callable(getattr(L, name))          # exported by the library, wrapped by the binding
    # the forms without the second table keep their signatures
    assert sigs["afd_lvar_loss_fwd"][1] == [vp] * 9 + [it, db, vp, vp, vp, lg, lg, vp]
    assert sigs["afd_lvar_loss_bwd"][1] == [vp] * 9 + [it, db, vp, vp, lg, lg, vp]


def test_entry_points_reject_bad_arguments_before_any_launch():
    """AFD_EINVAL comes from the host-side checks, so it needs no device: NULL pointers, sizes <= 0, H < 1, uniform_prob outside
    [0, 1), lo outside [0, T)."""
    from afdm import AfdError, lib
    L = lib()
    p = 4096                                             # any non-NULL value: nothing is dereferenced before the checks pass
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_loss_rows(p, p, p, p, p, None, 0, None, 4, 8, None)
    with pytest.raises(AfdError, match="B and chw must be positive"):
        L.afd_loss_rows(p, p, p, p, p, None, 0, p, 0, 8, None)
    with pytest.raises(AfdError, match="kind must be"):
        L.afd_loss_rows(p, p, p, p, p, None, 3, p, 4, 8, None)
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_lvar_loss_rows(p, p, p, p, p, p, p, None, None, 0, 0.0, p, 4, 8, None)
    with pytest.raises(AfdError, match="vlb_scale"):
        L.afd_lvar_loss_rows(p, p, p, p, p, p, p, p, None, 0, -1.0, p, 4, 8, None)
    with pytest.raises(AfdError, match="B and chw must be positive"):
        L.afd_lvar_loss_rows(p, p, p, p, p, p, p, p, None, 0, 0.0, p, 4, 0, None)
    tick = lambda **kw: L.afd_tsampler_tick(*[{**dict(t=p, rows=p, B=8, hist=p, count=p, T=12, H=3, lo=1, up=0.001, w=None, prob=p,
                                                      cdf=p, wtab=p, vw=None, warm=p, st=None), **kw}[k]
                                              for k in ("t", "rows", "B", "hist", "count", "T", "H", "lo", "up", "w", "prob", "cdf",
                                                        "wtab", "vw", "warm", "st")])
    for name in ("t", "rows", "hist", "count", "prob", "cdf", "wtab", "warm"):
        with pytest.raises(AfdError, match="must not be NULL"):
            tick(**{name: None})
    for kw in (dict(B=0), dict(T=0), dict(H=0), dict(B=-1)):
        with pytest.raises(AfdError, match="B and T must be positive and H >= 1"):
            tick(**kw)
    for lo in (-1, 12, 13):
        with pytest.raises(AfdError, match=r"lo must lie in \[0, T\)"):
            tick(lo=lo)
    for up in (-0.1, 1.0, 2.0, float("nan")):
        with pytest.raises(AfdError, match=r"uniform_prob must lie in \[0, 1\)"):
            tick(up=up)
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_tsampler_draw(p, None, 1, 12, p, 8, None)
    with pytest.raises(AfdError, match="B and T must be positive"):
        L.afd_tsampler_draw(p, p, 1, 12, p, 0, None)
    with pytest.raises(AfdError, match=r"lo must lie in \[0, T\)"):
        L.afd_tsampler_draw(p, p, 12, 12, p, 8, None)
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_lvar_loss_fwd_tw(p, p, p, p, p, p, p, p, None, None, 0, 0.0, None, None, p, 4, 8, None)
    with pytest.raises(AfdError, match="must not be NULL"):
        L.afd_lvar_loss_bwd_tw(p, p, p, p, p, p, p, p, None, None, 0, 0.0, p, None, 4, 8, None)


# ---- Python arguments --------------------------------------------------------------------------------------------------------------
class _Diff:
    """Enough of a Diffusion for the constructors' argument checks, which run before any device work."""
    noise_steps, variance, prediction = 12, "fixed", "v"


def test_sampler_and_step_argument_errors():
    import afdm
    import modules.ddpm_utils as U
    from afdm import DistillStep, LossSecondMomentSampler, TrainStep
    assert U.LossSecondMomentSampler is LossSecondMomentSampler and afdm.training.T_SAMPLERS == ("loss_second_moment",)
    for bad in (0, -1, 2.5, True, None, "10"):
        with pytest.raises(ValueError, match="history_per_term"):
            LossSecondMomentSampler(_Diff(), history_per_term=bad)
    for bad in (-0.1, 1.0, 1.5, float("nan"), True, None, "0.1"):
        with pytest.raises(ValueError, match="uniform_prob"):
            LossSecondMomentSampler(_Diff(), uniform_prob=bad)
    for bad in ("uniform", "Loss_second_moment", "", 1, True, object()):
        with pytest.raises(ValueError, match="unknown t_sampler"):
            TrainStep(None, _Diff(), lr=1e-3, t_sampler=bad)
    with pytest.raises(ValueError, match="t_sampler does not work with data parallelism"):
        TrainStep(None, _Diff(), lr=1e-3, t_sampler="loss_second_moment", distributed=True)
    with pytest.raises(ValueError, match="DistillStep: t_sampler is not supported"):
        DistillStep(object(), object(), _Diff(), [8, 4, 0], lr=1e-3, t_sampler="loss_second_moment")
    a = afdm.argument(t_sampler="loss_second_moment", t_sampler_history=4, t_sampler_uniform_prob=0.01)
    assert (a.t_sampler, a.t_sampler_history, a.t_sampler_uniform_prob) == ("loss_second_moment", 4, 0.01)
    b = afdm.argument()
    assert (b.t_sampler, b.t_sampler_history, b.t_sampler_uniform_prob) == (None, None, None)
    assert afdm.training.t_sampler_path("models/run/ckpt_x.pt") == "models/run/ckpt_x_tsampler.pt"
