"""CPU-side tests of gradient-norm clipping and the learning-rate schedule: the C ABI of the new entry points and their argument
checks (which return before any device is touched), `LRSchedule` against torch's LambdaLR, `clip_coefficient` against torch's
clip_grad_norm_, and the keyword checks of FusedAdamW / TrainStep."""
import ctypes
import itertools
import math

import pytest
import torch

P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float

KINDS = ("constant", "linear", "cosine")
WARMUPS = (0, 1, 3)
MIN_RATIOS = (0.0, 0.1, 1.0)


def schedule_grid():
    """(kind, warmup, total, min_ratio): all three kinds, warmup in {0, 1, 3}, total in {warmup, 10, 1000}, min_ratio in {0, .1, 1}"""
    for kind, warmup, min_ratio in itertools.product(KINDS, WARMUPS, MIN_RATIOS):
        for total in (warmup, 10, 1000):
            yield kind, warmup, total, min_ratio


def test_header_declares_and_types_the_new_entry_points():
    import afdm
    from afdm._lib import LIBPATH, parse_header
    sigs = parse_header()
    assert sigs["afd_grad_sqnorm_n_partials"] == (I, [])
    assert sigs["afd_grad_sqnorm_partials"] == (I, [P, L, F, P, I, P])
    assert sigs["afd_adamw_ctl_tick"] == (I, [P, F, F, P, I, P, I, P, P, P])
    assert sigs["afd_adamw_ctl_step"] == (I, [P, P, P, P, L, P, P, F, F, F, F, F, P, L, P, F, F, P])
    cdll = ctypes.CDLL(LIBPATH)
    for name in ("afd_grad_sqnorm_n_partials", "afd_grad_sqnorm_partials", "afd_adamw_ctl_tick", "afd_adamw_ctl_step"):
        assert hasattr(cdll, name), name
    n = afdm.lib().afd_grad_sqnorm_n_partials()
    assert isinstance(n, int) and 1 <= n <= 1024


def test_opt_ctl_struct_matches_the_header():
    from afdm._lib import HEADER
    from afdm.training import _OptCtl, _LR_KINDS
    src = open(HEADER).read()
    body = src[src.index("typedef struct afd_opt_ctl {"):src.index("} afd_opt_ctl;")]
    names = []
    for line in body.splitlines()[1:]:
        decl = line.split("/*")[0].strip().rstrip(";")
        if decl:
            names += [n.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f[0] for f in _OptCtl._fields_]
    for kind, value in _LR_KINDS.items():
        assert f"#define AFD_LR_{kind.upper()} {value}" in src


def _cfg(**kw):
    from afdm.training import _OptCtl
    d = dict(base_lr=1e-3, warmup=0, total=10, kind=2, min_ratio=0.0, max_norm=1.0, skip_nonfinite=0)
    d.update(kw)
    return _OptCtl(d["base_lr"], d["warmup"], d["total"], d["kind"], d["min_ratio"], d["max_norm"], d["skip_nonfinite"])


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    buf = (ctypes.c_double * 2048)()
    q = ctypes.addressof(buf)
    far = q + 8192                                                # (the partials, apart from "g")
    NP = lib.afd_grad_sqnorm_n_partials()
    with pytest.raises(afdm.AfdError, match="afd_grad_sqnorm_partials: .*NULL"):
        lib.afd_grad_sqnorm_partials(None, 8, 1.0, far, NP, None)
    with pytest.raises(afdm.AfdError, match="afd_grad_sqnorm_partials: .*NULL"):
        lib.afd_grad_sqnorm_partials(q, 8, 1.0, None, NP, None)
    for n in (0, -3):
        with pytest.raises(afdm.AfdError, match="afd_grad_sqnorm_partials: n must be positive"):
            lib.afd_grad_sqnorm_partials(q, n, 1.0, far, NP, None)
    for bad in (0, NP - 1, NP + 1):
        with pytest.raises(afdm.AfdError, match="afd_grad_sqnorm_partials: n_partials"):
            lib.afd_grad_sqnorm_partials(q, 8, 1.0, far, bad, None)
    with pytest.raises(afdm.AfdError, match="afd_grad_sqnorm_partials: .*overlap"):
        lib.afd_grad_sqnorm_partials(q, 8, 1.0, q, NP, None)

    def tick(state=q, es=None, start=0, parts=far, n_parts=NP, cfg="default", ctl=q, **kw):
        c = _cfg(**kw) if cfg == "default" else cfg
        lib.afd_adamw_ctl_tick(state, 0.9, 0.999, es, start, parts, n_parts, None if c is None else ctypes.byref(c), ctl, None)
    for k in ("state", "cfg", "ctl"):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: .*NULL"):
            tick(**{k: None})
    for bad in (float("nan"), float("inf"), -1e-3):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: base_lr"):
            tick(base_lr=bad)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: warmup"):
        tick(warmup=-1)
    for kind in (1, 2):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: total < warmup"):
            tick(kind=kind, warmup=5, total=4)
    for kind in (-1, 3):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: unknown schedule kind"):
            tick(kind=kind)
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: min_ratio"):
            tick(min_ratio=bad)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: max_norm"):
        tick(max_norm=float("nan"))
    for bad in (0, 1025):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: n_partials"):
            tick(n_parts=bad)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_tick: ema_start"):
        tick(es=q, start=-1)

    def step(p=q, g=q, m=q, v=q, n_active=8, st=q, ctl=q, ema=None, n_ema=0, es=None, beta=0.0, omb=0.0):
        lib.afd_adamw_ctl_step(p, g, m, v, n_active, st, ctl, 0.9, 0.999, 1e-8, 0.01, 1.0, ema, n_ema, es, beta, omb, None)
    for k in ("p", "g", "m", "v", "st", "ctl"):
        with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_step: .*NULL"):
            step(**{k: None})
    with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_step: n_active must be positive"):
        step(n_active=0)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_step: .*ema_state is NULL"):
        step(ema=q, n_ema=8, beta=0.9, omb=0.1)
    with pytest.raises(afdm.AfdError, match=r"afd_adamw_ctl_step: 0 < n_active <= n_ema"):
        step(ema=q, es=q, n_active=9, n_ema=8, beta=0.9, omb=0.1)
    with pytest.raises(afdm.AfdError, match="afd_adamw_ctl_step: beta"):
        step(ema=q, es=q, n_ema=8, beta=1.01, omb=-0.01)


def _lambda_lr_values(kind, warmup, total, min_ratio, base_lr, n):
    """param_groups[0]["lr"] over n updates of a CPU AdamW driven by LambdaLR with the usual warm-up lambdas, written here
    independently of LRSchedule."""
    def lam(k):
        if k < warmup:
            return float(k) / float(max(1, warmup))
        if kind == "constant":
            return 1.0
        pr = min(1.0, float(k - warmup) / float(max(1, total - warmup)))
        if kind == "cosine":
            return min_ratio + (1.0 - min_ratio) * (0.5 * (1.0 + math.cos(math.pi * pr)))
        return min_ratio + (1.0 - min_ratio) * (1.0 - pr)
    w = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.AdamW([w], lr=base_lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    out = []
    for _ in range(n):
        out.append(opt.param_groups[0]["lr"])
        w.grad = torch.ones(3)
        opt.step()
        sched.step()
    return out


def test_lr_schedule_equals_lambda_lr_exactly():
    import afdm
    base_lr = 3e-4
    n_cases = 0
    for kind, warmup, total, min_ratio in schedule_grid():
        sch = afdm.LRSchedule(kind, warmup=warmup, total=total, min_ratio=min_ratio)
        want = _lambda_lr_values(kind, warmup, total, min_ratio, base_lr, total + 3)
        for k, w in enumerate(want):
            assert sch.lr(base_lr, k) == w, (kind, warmup, total, min_ratio, k)
            assert sch.factor(k) * base_lr == w
        n_cases += 1
    assert n_cases == 81


def test_lr_schedule_edges():
    import afdm
    for kind in ("linear", "cosine"):
        s = afdm.LRSchedule(kind, warmup=3, total=3, min_ratio=0.1)          # total == warmup: the decay is over at once
        assert [s.factor(k) for k in range(3)] == [0.0, 1 / 3, 2 / 3]
        assert s.factor(3) == 1.0                                            # pr = 0 at k = warmup
        assert s.factor(4) == pytest.approx(0.1, abs=1e-16) and s.factor(50) == s.factor(4)
        s = afdm.LRSchedule(kind, warmup=2, total=10, min_ratio=0.25)
        assert s.factor(10) == pytest.approx(0.25, abs=1e-16)
        assert s.factor(11) == s.factor(10) == s.factor(10 ** 6)             # past total: stays at min_ratio
        assert all(s.factor(k) >= s.factor(k + 1) for k in range(2, 12))
    s = afdm.LRSchedule("constant", warmup=4)
    assert s.total == 4 and s.factor(0) == 0.0 and s.factor(3) == 0.75 and s.factor(4) == 1.0 and s.factor(10 ** 9) == 1.0
    assert afdm.LRSchedule().factor(0) == 1.0                                # no warm-up: the base rate from the first update
    assert afdm.LRSchedule("cosine", total=10).lr(2.0, 5) == 2.0 * (0.5 * (1.0 + math.cos(math.pi * 0.5)))


def test_lr_schedule_value_errors():
    import afdm
    with pytest.raises(ValueError, match="kind"):
        afdm.LRSchedule("exponential", total=10)
    for kind in ("linear", "cosine"):
        with pytest.raises(ValueError, match="needs total"):
            afdm.LRSchedule(kind)
        with pytest.raises(ValueError, match="total < warmup"):
            afdm.LRSchedule(kind, warmup=5, total=4)
    for bad in (-1, 1.5, True, "3"):
        with pytest.raises(ValueError, match="warmup"):
            afdm.LRSchedule("constant", warmup=bad)
    with pytest.raises(ValueError, match="total"):
        afdm.LRSchedule("cosine", total=-2)
    for bad in (-0.1, 1.1, float("nan"), "x", None):
        with pytest.raises(ValueError, match="min_ratio"):
            afdm.LRSchedule("cosine", total=10, min_ratio=bad)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("max_norm,clips", ((1.0, True), (100.0, False)))
def test_clip_coefficient_against_torch_clip_grad_norm(max_norm, clips):
    import afdm
    g = torch.Generator().manual_seed(31)
    for _ in range(3):
        gw, gb = torch.randn(11, 37, generator=g), torch.randn(11, generator=g)
        lin = torch.nn.Linear(37, 11)
        lin.weight.grad, lin.bias.grad = gw.clone(), gb.clone()
        total = float(torch.nn.utils.clip_grad_norm_(lin.parameters(), max_norm))
        norm = math.sqrt(float((gw.double() ** 2).sum() + (gb.double() ** 2).sum()))      # ours: fp64
        assert 19.0 < norm < 21.0
        assert abs(norm - total) <= 1e-6 * total
        coef = afdm.clip_coefficient(norm, max_norm)
        assert (coef < 1.0) == clips and (norm > max_norm) == clips       # the regime this case is meant to be in
        if clips:
            assert coef == max_norm / (norm + 1e-6)
            assert float(lin.weight.grad.norm()) < 1.001 * max_norm
        else:
            assert coef == 1.0 and torch.equal(lin.weight.grad, gw) and torch.equal(lin.bias.grad, gb)
        assert _rel_l2(gw * coef, lin.weight.grad) < 1e-6 and _rel_l2(gb * coef, lin.bias.grad) < 1e-6


def test_clip_coefficient_edges():
    import afdm
    assert afdm.clip_coefficient(5.0, None) == 1.0 and afdm.clip_coefficient(5.0, 0.0) == 1.0 and afdm.clip_coefficient(5.0, -1.0) == 1.0
    assert afdm.clip_coefficient(0.0, 1.0) == 1.0
    assert afdm.clip_coefficient(float("inf"), 1.0) == 0.0
    assert math.isnan(afdm.clip_coefficient(float("nan"), 1.0))


def test_keyword_validation_on_cpu():
    import afdm
    lin = torch.nn.Linear(5, 3)
    sch = afdm.LRSchedule("cosine", warmup=1, total=5)
    for cls, args in ((afdm.TrainStep, (lin, None)), (afdm.FusedAdamW, (lin,))):
        for bad in (0, 0.0, -1.0, float("nan"), "1", True):
            with pytest.raises(ValueError, match="max_grad_norm"):
                cls(*args, lr=1e-3, max_grad_norm=bad)
        for bad in ("cosine", 3, {"kind": "cosine"}):
            with pytest.raises(ValueError, match="lr_schedule must be an LRSchedule"):
                cls(*args, lr=1e-3, lr_schedule=bad)
        with pytest.raises(ValueError, match="total < warmup"):
            cls(*args, lr=1e-3, lr_schedule=afdm.LRSchedule("linear", warmup=6, total=5))
    # a CPU FusedAdamW can be built with the feature on (buffers only; no launch)
    opt = afdm.FusedAdamW(lin, lr=1e-3, max_grad_norm=1.0, lr_schedule=sch)
    assert opt.ctl.dtype == torch.float64 and opt.ctl.numel() == len(afdm.training.CTL_FIELDS) == 8
    assert opt.partials.numel() == afdm.lib().afd_grad_sqnorm_n_partials()
    assert opt.n_skipped == 0 and opt.last_grad_norm == 0.0
    plain = afdm.FusedAdamW(torch.nn.Linear(5, 3), lr=1e-3)
    assert plain.ctl is None and plain.partials is None and plain.last_grad_norm is None and plain.last_lr == 1e-3 and plain.n_skipped == 0
    only_sched = afdm.FusedAdamW(torch.nn.Linear(5, 3), lr=1e-3, lr_schedule=sch)
    assert only_sched.ctl is not None and only_sched.partials is None      # a schedule alone needs no norm: no extra launch


def test_argument_fields_and_reexport():
    import afdm
    from modules.ddpm_utils import LRSchedule
    assert LRSchedule is afdm.LRSchedule is afdm.training.LRSchedule
    a = afdm.argument()
    assert a.max_grad_norm is None and a.lr_warmup == 0 and a.lr_schedule is None and a.lr_min_ratio == 0.0
    b = afdm.argument(max_grad_norm=1.0, lr_warmup=5, lr_schedule="cosine", lr_min_ratio=0.1)
    assert (b.max_grad_norm, b.lr_warmup, b.lr_schedule, b.lr_min_ratio) == (1.0, 5, "cosine", 0.1)
    assert a.ema_beta is None and a.ema_start == 2000
