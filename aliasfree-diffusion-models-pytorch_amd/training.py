"""F15: the train step (modules/ddpm_utils.py:483-518) -- AdamW + MSE on the HIP engine, optional
data parallelism (one process per GPU, RCCL all-reduce of one flat fp32 gradient buffer), and
hipGraph replay of the whole step.
"""
import ctypes
import logging
import math
import os
import weakref

import torch
import torch.distributed as dist

from . import ops
from ._lib import lib
from .diffusion import Diffusion


class argument:
    """Attribute bag of run settings (ddpm_utils.py:11-23)."""

    def __init__(self, run_name=None, epochs=None, batch_size=None, image_size=None, image_channels=3,
                 dataset_path=None, device=None, lr=None, noise_steps=None, image_gen_n=4, ema_beta=None, ema_start=2000,
                 max_grad_norm=None, lr_warmup=0, lr_schedule=None, lr_min_ratio=0.0, noise_schedule=None, prediction=None,
                 loss_weighting=None, snr_gamma=None, variance=None, vlb_lambda=None, t_sampler=None, t_sampler_history=None,
                 t_sampler_uniform_prob=None):
        """ema_beta / ema_start (not in the reference's class): with ema_beta set, `train` keeps an EMA of the weights
        (EMA(ema_beta), step_start_ema = ema_start).
        max_grad_norm: `train` clips the gradient to this global L2 norm.  lr_schedule ("constant" | "linear" | "cosine") /
        lr_warmup / lr_min_ratio: `train` runs LRSchedule(lr_schedule, lr_warmup, total = epochs * batches, lr_min_ratio);
        lr_warmup > 0 alone means a warm-up into a constant rate.
        noise_schedule ("linear" | "cosine") / prediction ("eps" | "v" | "x0"): `diffusion_kwargs` turns them into the arguments
        of the run's Diffusion; loss_weighting ("min_snr" | "truncated_snr") / snr_gamma: `train` hands them to its TrainStep.  None = the default.
        variance ("fixed" | "learned") goes to the run's Diffusion and doubles the UNet's output channels when "learned"
        (`model_out_channels`); vlb_lambda is the hybrid loss's weight in `train`'s TrainStep.
        t_sampler ("loss_second_moment") / t_sampler_history / t_sampler_uniform_prob: `train` draws the timesteps from a
        LossSecondMomentSampler(history_per_term, uniform_prob) and saves its state beside the checkpoint."""
        self.run_name, self.epochs, self.batch_size, self.image_size = run_name, epochs, batch_size, image_size
        self.image_channels, self.dataset_path, self.device, self.lr = image_channels, dataset_path, device, lr
        self.noise_steps, self.image_gen_n = noise_steps, image_gen_n
        self.ema_beta, self.ema_start = ema_beta, ema_start
        self.max_grad_norm, self.lr_warmup, self.lr_schedule, self.lr_min_ratio = max_grad_norm, lr_warmup, lr_schedule, lr_min_ratio
        self.noise_schedule, self.prediction = noise_schedule, prediction
        self.loss_weighting, self.snr_gamma = loss_weighting, snr_gamma
        self.variance, self.vlb_lambda = variance, vlb_lambda
        self.t_sampler, self.t_sampler_history, self.t_sampler_uniform_prob = t_sampler, t_sampler_history, t_sampler_uniform_prob


def diffusion_kwargs(args):
    """The Diffusion arguments named by a run's settings (`args.noise_schedule`, `args.prediction`, `args.variance`); empty when
    all are absent or None, so a run without the keys builds the default Diffusion."""
    kw = {}
    if getattr(args, "noise_schedule", None) is not None:
        kw["schedule"] = args.noise_schedule
    if getattr(args, "prediction", None) is not None:
        kw["prediction"] = args.prediction
    if getattr(args, "variance", None) is not None:
        kw["variance"] = args.variance
    return kw


def model_out_channels(args):
    """The UNet's c_out for a run's settings: image_channels, or twice that with variance="learned"."""
    return args.image_channels * (2 if getattr(args, "variance", None) == "learned" else 1)


def set_seed(seed):
    """modules/utils.py:98-105."""
    import random
    import numpy as np
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)
        torch.cuda.manual_seed_all(seed)
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False


def setup_logging(run_name):
    """modules/utils.py:84-88."""
    os.makedirs("models", exist_ok=True)
    os.makedirs("results", exist_ok=True)
    os.makedirs(os.path.join("models", run_name), exist_ok=True)
    os.makedirs(os.path.join("results", run_name), exist_ok=True)


_HOMES = weakref.WeakKeyDictionary()      # model -> the FlatParams its parameters live in (EMA's fast path looks it up)


class FlatParams:
    """Re-homes a model's parameters (and their .grad) as views of two flat fp32 buffers so the optimiser is one
    kernel launch and the DDP exchange is a handful of large all-reduces.  Order: `parameters()` order, except that
    parameters the forward never touches (`model.unused_parameters()`, e.g. variant 4's stage-level `norm1` or
    `label_emb` of an unconditionally trained net) sit at the tail, beyond `n_active`: the reference's
    `torch.optim.AdamW` skips parameters whose grad is None (ddpm_utils.py:489,504-506 after `zero_grad()`), so they
    must see neither the update nor the weight decay.  state_dict()/load_state_dict() keep working (the Parameters are
    the same objects; only their storage moved)."""

    def __init__(self, model, conditional=False):
        """conditional: the train loop will pass class labels (UNet.forward(x, t, y)), so `label_emb` is a live parameter
        (updated and exchanged); the reference's own loop never does (ddpm_utils.py:502), hence the default."""
        params = [p for p in model.parameters()]
        assert params and all(p.dtype == torch.float32 for p in params)
        unused = getattr(model, "unused_parameters", None)
        skip = set()
        if callable(unused):
            try:
                skip = {id(p) for p in unused(conditional=conditional)}
            except TypeError:
                skip = {id(p) for p in unused()}
        self.conditional = conditional
        params = [p for p in params if id(p) not in skip] + [p for p in params if id(p) in skip]
        dev = params[0].device
        self.params = params
        self.numel = sum(p.numel() for p in params)
        self.n_active = sum(p.numel() for p in params if id(p) not in skip)
        self.flat = torch.empty(self.numel, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(self.numel, device=dev, dtype=torch.float32)
        self.offsets = []
        o = 0
        for p in params:
            n = p.numel()
            self.flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
            self.offsets.append(o)
            o += n
        _HOMES[model] = self

    def zero_grad(self):
        self.grad.zero_()
        for p, o in zip(self.params, self.offsets):      # autograd may have replaced .grad; re-attach the views
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * o:
                p.grad = self.grad[o:o + p.numel()].view(p.shape)


_LR_KINDS = {"constant": 0, "linear": 1, "cosine": 2}      # AFD_LR_* of afd.h


def _whole(x, what, who):
    if isinstance(x, bool) or not isinstance(x, int) or x < 0:
        raise ValueError(f"{who}: {what} must be an integer >= 0 (got {x!r})")
    return x


class LRSchedule:
    """Learning-rate factor of the k-th optimiser update (k = 0, 1, ...): linear warm-up over `warmup` updates, then constant,
    or a linear / cosine decay that reaches `min_ratio` at update `total` and stays there:
        k < warmup:   k / max(1, warmup)
        constant:     1
        otherwise:    pr = min(1, (k - warmup) / max(1, total - warmup)),
                      base = 0.5 * (1 + cos(pi * pr))  (cosine)  or  1 - pr  (linear),   min_ratio + (1 - min_ratio) * base
    -- torch.optim.lr_scheduler.LambdaLR with the usual "..._schedule_with_warmup" lambda, evaluated in Python doubles (equal
    to LambdaLR's param_groups[0]["lr"] bit for bit).  Like LambdaLR it gives lr = 0 for the very first update when warmup > 0.
    This class is the host mirror; FusedAdamW(lr_schedule=...) evaluates the same formula on the device (afd_adamw_ctl_tick), from
    its device-resident step counter, so a captured step follows the schedule."""

    def __init__(self, kind="constant", warmup=0, total=None, min_ratio=0.0):
        who = "LRSchedule"
        if kind not in _LR_KINDS:
            raise ValueError(f"{who}: kind must be one of {sorted(_LR_KINDS)} (got {kind!r})")
        self.kind, self.warmup = kind, _whole(warmup, "warmup", who)
        if kind == "constant" and total is None:
            total = self.warmup
        if total is None:
            raise ValueError(f"{who}: a {kind} decay needs total (the number of optimiser updates of the run)")
        self.total = _whole(total, "total", who)
        if kind != "constant" and self.total < self.warmup:
            raise ValueError(f"{who}: total < warmup ({self.total} < {self.warmup})")
        try:
            ok = 0.0 <= float(min_ratio) <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{who}: min_ratio must lie in [0, 1] (got {min_ratio!r})")
        self.min_ratio = float(min_ratio)

    def factor(self, k):
        if k < self.warmup:
            return float(k) / float(max(1, self.warmup))
        if self.kind == "constant":
            return 1.0
        pr = min(1.0, float(k - self.warmup) / float(max(1, self.total - self.warmup)))
        base = 0.5 * (1.0 + math.cos(math.pi * pr)) if self.kind == "cosine" else 1.0 - pr
        return self.min_ratio + (1.0 - self.min_ratio) * base

    def lr(self, base_lr, k):
        return base_lr * self.factor(k)

    def __repr__(self):
        return f"LRSchedule(kind={self.kind!r}, warmup={self.warmup}, total={self.total}, min_ratio={self.min_ratio})"


def clip_coefficient(norm, max_norm):
    """The factor torch.nn.utils.clip_grad_norm_(norm_type=2) scales the gradients by, in Python doubles:
    min(1, max_norm / (norm + 1e-6)); 1 when max_norm is None or <= 0 (no clipping).  Host mirror of afd_adamw_ctl_tick's step 1
    (a NaN norm gives NaN there and here, as torch's clamp does)."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    c = float(max_norm) / (float(norm) + 1e-6)
    return 1.0 if c > 1.0 else c


def _check_opt_ctl(who, max_grad_norm, lr_schedule):
    if max_grad_norm is not None:
        ok = isinstance(max_grad_norm, (int, float)) and not isinstance(max_grad_norm, bool) and max_grad_norm > 0      # (False for NaN)
        if not ok:
            raise ValueError(f"{who}: max_grad_norm must be a number > 0, or None for no clipping (got {max_grad_norm!r})")
    if lr_schedule is not None and not isinstance(lr_schedule, LRSchedule):
        raise ValueError(f"{who}: lr_schedule must be an LRSchedule or None (got {type(lr_schedule).__name__})")


class _OptCtl(ctypes.Structure):               # afd_opt_ctl of afd.h
    _fields_ = [("base_lr", ctypes.c_double), ("warmup", ctypes.c_long), ("total", ctypes.c_long), ("kind", ctypes.c_int),
                ("min_ratio", ctypes.c_double), ("max_norm", ctypes.c_double), ("skip_nonfinite", ctypes.c_int)]


CTL_FIELDS = ("lr", "coef", "norm", "skip", "n_skipped", "sq", "index", "factor")      # FusedAdamW.ctl, afd.h


class FusedAdamW:
    """torch.optim.AdamW(params, lr) semantics (betas .9/.999, eps 1e-8, weight_decay 0.01 --
    the defaults the reference relies on, ddpm_utils.py:489) as ONE kernel over the flat buffers (their first
    `n_active` elements: see FlatParams).
    The step counter and bias corrections live on the device so a captured hipGraph replays correctly.

    max_grad_norm / lr_schedule / skip_nonfinite / track_grad_norm: gradient clipping by the global L2 norm
    (torch.nn.utils.clip_grad_norm_) and a learning-rate schedule (LRSchedule), decided ON THE DEVICE so that they work in a
    captured step, where `lr` passed by value would be frozen and a host-side clip cannot run at all.  With all four at their
    defaults the step is the two launches it always was (afd_adamw_tick + afd_adamw_step, or the EMA pair).  Otherwise:
        [afd_grad_sqnorm_partials]  ->  afd_adamw_ctl_tick  ->  afd_adamw_ctl_step        (at most one launch more)
    the first only when a norm is needed (max_grad_norm, skip_nonfinite or track_grad_norm).  The norm is that of the gradient
    the optimiser consumes, grad * grad_scale over the first n_active elements; under data parallelism it is taken after the
    all-reduce, over the reduced buffer with grad_scale = 1 / world: every rank holds the same bytes and the reduction order is
    fixed, so every rank computes the same coefficient and NO extra collective is needed.
    skip_nonfinite: an update whose gradient norm is inf or NaN is dropped whole (no parameter, moment, step count or EMA
    change) and counted in `n_skipped`.
    `ctl` is the device buffer (float64, CTL_FIELDS) the tick writes and the step reads; `last_grad_norm`, `last_lr`,
    `n_skipped` read it back (one D2H copy, hence a sync, per access -- nothing in `step` synchronises)."""

    def __init__(self, model_or_flat, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, conditional=False,
                 max_grad_norm=None, lr_schedule=None, skip_nonfinite=False, track_grad_norm=False):
        _check_opt_ctl("FusedAdamW", max_grad_norm, lr_schedule)
        self.fp = model_or_flat if isinstance(model_or_flat, FlatParams) else FlatParams(model_or_flat, conditional=conditional)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        dev = self.fp.flat.device
        self.m = torch.zeros_like(self.fp.flat)
        self.v = torch.zeros_like(self.fp.flat)
        self.state = torch.zeros(4, device=dev, dtype=torch.float32)
        self.max_grad_norm, self.lr_schedule = max_grad_norm, lr_schedule
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)
        self._ctl_on = max_grad_norm is not None or lr_schedule is not None or self.skip_nonfinite or self.track_grad_norm
        self._need_norm = max_grad_norm is not None or self.skip_nonfinite or self.track_grad_norm
        self.ctl = self.partials = None
        if self._ctl_on:
            self.ctl = torch.zeros(len(CTL_FIELDS), device=dev, dtype=torch.float64)
            if self._need_norm:
                self.partials = torch.zeros(lib().afd_grad_sqnorm_n_partials(), device=dev, dtype=torch.float64)

    def _cfg(self):
        sch = self.lr_schedule or LRSchedule()
        return _OptCtl(float(self.lr), sch.warmup, sch.total, _LR_KINDS[sch.kind], sch.min_ratio,
                       float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0, int(self.skip_nonfinite))

    def _read_ctl(self, field):
        if self.ctl is None:
            return None
        return float(self.ctl[CTL_FIELDS.index(field)].item())

    @property
    def last_grad_norm(self):
        """L2 norm of the last step's gradient (before clipping); None unless a norm is computed.  One D2H copy."""
        return self._read_ctl("norm") if self._need_norm else None

    @property
    def last_lr(self):
        """The learning rate the last applied update used (the fp32 value).  One D2H copy when a schedule is active."""
        return float(self.lr) if self.ctl is None else self._read_ctl("lr")

    @property
    def n_skipped(self):
        """Updates dropped by skip_nonfinite so far.  One D2H copy."""
        return 0 if self.ctl is None else int(self._read_ctl("n_skipped"))

    def zero_grad(self, set_to_none=False):
        self.fp.zero_grad()

    def step(self, grad_scale=1.0, ema=None):
        """ema: an _EMAHome (TrainStep(ema=...)): the same two launches, in their fused EMA form (afd.h)."""
        L, s, fp = lib(), ops._stream(), self.fp
        state, (b1, b2) = self.state.data_ptr(), self.betas
        bufs = (fp.flat.data_ptr(), fp.grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), fp.n_active, state)
        hyper = (b1, b2, self.eps, self.weight_decay, grad_scale)
        if ema is not None:
            es, start = ema.state.data_ptr(), ema.start
            ema_args = (ema.flat.data_ptr(), ema.flat.numel(), es, ema.beta, ema.one_minus_beta)
        else:
            es, start, ema_args = None, 0, (None, 0, None, 0.0, 0.0)
        if self._ctl_on:
            parts, n_parts = None, 0
            if self._need_norm:
                parts, n_parts = self.partials.data_ptr(), self.partials.numel()
                L.afd_grad_sqnorm_partials(fp.grad.data_ptr(), fp.n_active, grad_scale, parts, n_parts, s)
            ctl = self.ctl.data_ptr()
            L.afd_adamw_ctl_tick(state, b1, b2, es, start, parts, n_parts, ctypes.byref(self._cfg()), ctl, s)
            L.afd_adamw_ctl_step(*bufs, ctl, *hyper, *ema_args, s)
        elif ema is not None:
            L.afd_adamw_ema_tick(state, b1, b2, es, start, s)
            L.afd_adamw_ema_step(*bufs, self.lr, *hyper, *ema_args, s)
        else:
            L.afd_adamw_tick(state, b1, b2, s)
            L.afd_adamw_step(*bufs, self.lr, *hyper, s)
        ops.bump_param_epoch()      # the parameters (and the EMA model's) moved under raw pointers: cached transforms are stale

    def state_buffers(self):
        """Every device buffer a step changes (what TrainStep's capture warm-up saves and puts back)."""
        return (self.fp.flat, self.m, self.v, self.state) + ((self.ctl,) if self.ctl is not None else ())


def _named_shapes(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def _check_pair(ema_model, model):
    if ema_model is model:
        raise ValueError("EMA: ema_model is model: the average needs a separate copy (copy.deepcopy(model))")
    a, b = _named_shapes(model), _named_shapes(ema_model)
    if a != b:
        diff = sorted(set(a.items()) ^ set(b.items()))[:4]
        raise ValueError(f"EMA: ema_model and model differ in architecture (state_dict names or shapes), e.g. {diff}")


class _EMAHome:
    """The fast path's device side: ema_model's parameters re-homed as views of ONE flat fp32 buffer, in the order of the
    model's FlatParams (its unused tail included), so one kernel updates them all from the model's flat buffer.
    `state` is the device int32 {calls, copy} of afd_adamw_ema_tick (TrainStep(ema=...))."""

    def __init__(self, ema_model, model, fp):
        self.ema_model, self.model, self.fp = ema_model, model, fp
        name_of = {id(p): n for n, p in model.named_parameters()}
        eparams = dict(ema_model.named_parameters())
        self.flat = torch.empty(fp.numel, device=fp.flat.device, dtype=torch.float32)      # no grad buffer
        with torch.no_grad():
            for p, o in zip(fp.params, fp.offsets):
                ep, n = eparams[name_of[id(p)]], p.numel()
                self.flat[o:o + n].copy_(ep.data.reshape(-1))
                ep.data = self.flat[o:o + n].view(ep.shape)
                ep.grad = None
        mbufs = dict(model.named_buffers())
        self.buffers = [(b, mbufs[k]) for k, b in ema_model.named_buffers()]
        self.state = torch.zeros(2, device=fp.flat.device, dtype=torch.int32)
        self.start, self.beta, self.one_minus_beta = 0, 0.0, 1.0       # set by TrainStep when it drives the EMA

    def state_buffers(self):
        """FusedAdamW.state_buffers' counterpart: the EMA buffer and its call counter."""
        return self.flat, self.state


class EMA:
    """Exponential moving average of a model's weights: modules/ddpm_utils.py:26-51, same interface and call counting --
    `step_ema` copies the weights (reset_parameters) while `step < step_start_ema` and blends them
    (`old * beta + (1 - beta) * new`) after, incrementing `step` on every call.

    Fast path: when `model` lives in a FlatParams (a TrainStep or FusedAdamW owns it), the first call re-homes `ema_model`'s
    parameters as views of one flat buffer in the same order, and each call after that is ONE afd_ema_step launch (fp32, the same
    three roundings as the torch expression).  Any other pair (CPU included) runs the torch expression per tensor.
    TrainStep(ema=..., ema_model=...) goes further and fuses the update into its AdamW launch (afd_adamw_ema_step); the EMA is then
    advanced by the step and calling `step_ema` by hand raises RuntimeError.

    One deliberate difference from the reference: the update is IN PLACE (`copy_`, or the kernel writing the parameters'
    storage), where the reference rebinds `ma_params.data` to a new tensor on every call -- so the EMA model's parameter storage,
    and any pointer a captured graph or a cached weight image holds into it, stays valid.  Buffers (the UNet has none) are copied
    on reset and left alone on blend, as load_state_dict does."""

    def __init__(self, beta):
        self.beta = beta
        self._betas()
        self.step = 0
        self._home = None
        self._driver = None          # the TrainStep whose AdamW launch advances this EMA

    def _betas(self):
        try:
            b = float(self.beta)
            ok = 0.0 <= b <= 1.0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"EMA: beta must lie in [0, 1] (got {self.beta!r})")
        return b, float(1.0 - b)     # 1 - beta in double, as Python evaluates `(1 - self.beta)`

    def _fast(self, ema_model, model):
        """The _EMAHome of this pair when `model` is homed in a FlatParams (built on first use), else None."""
        h = self._home
        if h is not None and h.ema_model is ema_model and h.model is model and _HOMES.get(model) is h.fp:
            return h
        fp = _HOMES.get(model)
        if fp is None:
            return None
        _check_pair(ema_model, model)
        if any(p.dtype != torch.float32 or p.device != fp.flat.device for p in ema_model.parameters()):
            return None
        self._home = _EMAHome(ema_model, model, fp)
        return self._home

    def _launch(self, h, copy):
        b, omb = self._betas()
        lib().afd_ema_step(h.flat.data_ptr(), h.fp.flat.data_ptr(), h.flat.numel(), int(copy), b, omb, ops._stream())
        ops.bump_param_epoch()       # the EMA model's parameters moved under raw pointers: its cached weight images are stale

    def update_model_average(self, ma_model, current_model):
        h = self._fast(ma_model, current_model)
        if h is not None:
            self._launch(h, copy=False)
            return
        _check_pair(ma_model, current_model)
        self._betas()
        cur = dict(current_model.named_parameters())
        with torch.no_grad():
            for k, ma in ma_model.named_parameters():
                ma.copy_(self.update_average(ma.data, cur[k].data))

    def update_average(self, old, new):
        if old is None:
            return new
        return old * self.beta + (1 - self.beta) * new

    def step_ema(self, ema_model, model, step_start_ema=2000):
        if self._driver is not None:
            raise RuntimeError("EMA.step_ema: this EMA is advanced by a TrainStep(ema=...), inside its AdamW launch; "
                               "calling step_ema as well would update it twice")
        if self.step < step_start_ema:
            self.reset_parameters(ema_model, model)
            self.step += 1
            return
        self.update_model_average(ema_model, model)
        self.step += 1

    def reset_parameters(self, ema_model, model):
        h = self._fast(ema_model, model)
        if h is not None:
            self._launch(h, copy=True)
            with torch.no_grad():
                for eb, mb in h.buffers:
                    eb.copy_(mb)
            return
        _check_pair(ema_model, model)
        cur = dict(model.named_parameters())
        bufs = dict(model.named_buffers())
        with torch.no_grad():
            for k, ep in ema_model.named_parameters():
                ep.copy_(cur[k])
            for k, eb in ema_model.named_buffers():
                eb.copy_(bufs[k])


class GradAllReduce:
    """Data-parallel gradient exchange: SUM all-reduce of the flat gradient buffer in a few contiguous buckets (a few MB
    each: xGMI rings are per-link bound, so few large messages), the mean folded into AdamW's grad_scale.

    Overlap with backward: backward produces parameter gradients in reverse layer order, i.e. from the END of the flat
    buffer.  Every op that writes a parameter's gradient reports it (`wrote`, wired to ops._GradMode.on_write by
    TrainStep; launches deferred to the weight-gradient stream report when they are actually launched); when the last
    parameter of a bucket has been written, a communication stream waits for the streams that wrote into the bucket
    (events) and the bucket's all-reduce starts there while backward goes on with the earlier layers.  `finish()` joins
    them before AdamW (and exchanges whatever was not reported, e.g. after a hipGraph replay of the backward).
    Buckets are cut at top-level module boundaries walking the model backwards (for the UNet: [up1..outc], [bot2,bot3],
    [down3,sa3,bot1], [inc..sa2]: the last one to become ready is the smallest, 2.2 MB).

    Works on any torch.distributed backend: 'nccl' (= RCCL over xGMI) on GPUs; with 'gloo' and device tensors each
    bucket is staged through host memory (CPU tests, several ranks sharing one GPU)."""

    def __init__(self, flat, n_buckets=4, group=None, model=None):
        fp = flat if isinstance(flat, FlatParams) else None
        self.g = fp.grad[:fp.n_active] if fp is not None else flat
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        n = self.g.numel()
        nb = max(1, min(n_buckets, n))
        edges = None
        if fp is not None and model is not None:
            edges = self._module_edges(fp, model, nb)
        if edges is None:
            edges = [n * i // nb for i in range(nb + 1)]
        self.slices = [(edges[i], edges[i + 1]) for i in range(len(edges) - 1) if edges[i + 1] > edges[i]]
        self.via_host = dist.is_initialized() and dist.get_backend(group) == "gloo" and self.g.is_cuda
        self.comm = torch.cuda.Stream() if self.g.is_cuda else None
        self.side = None                                # the weight-gradient stream (set by TrainStep)
        # parameter -> bucket, for the readiness bookkeeping
        self._bucket_of, self._count = {}, [0] * len(self.slices)
        if fp is not None:
            for p_, o in zip(fp.params, fp.offsets):
                if o >= fp.n_active:
                    continue
                k = next(i for i, (a, b) in enumerate(self.slices) if a <= o < b)
                assert o + p_.numel() <= self.slices[k][1], "a parameter straddles two buckets"
                self._bucket_of[id(p_)] = k
                self._count[k] += 1
        self._left, self._seen, self._works, self._launched = list(self._count), set(), [], set()
        self.overlapped_last_step = 0          # buckets whose all-reduce started while backward was still running
        self.started_before_finish = 0         # ... plus those started by the final flush of the weight-gradient queue
        self._in_backward = None

    @staticmethod
    def _module_edges(fp, model, nb):
        """Bucket edges at top-level module boundaries, accumulating from the last module backwards."""
        kids = [m for m in model.children() if any(True for _ in m.parameters())]
        off = {id(p_): o for p_, o in zip(fp.params, fp.offsets)}
        starts = []
        for m in kids:
            os_ = [off[id(p_)] for p_ in m.parameters() if off[id(p_)] < fp.n_active]
            if os_:
                starts.append(min(os_))
        if len(starts) < 2 or starts != sorted(starts) or starts[0] != 0:
            return None
        target, edges, hi = fp.n_active / nb, [fp.n_active], fp.n_active
        for st in reversed(starts[1:]):
            if hi - st >= target and len(edges) < nb:
                edges.append(st)
                hi = st
        edges.append(0)
        return sorted(set(edges))

    # -- readiness bookkeeping (called during backward) ------------------------------------------
    def begin_step(self):
        self._left, self._seen, self._works, self._launched = list(self._count), set(), [], set()
        self._in_backward = None

    def backward_done(self):
        """Called when autograd's backward has returned (before the last queued weight-gradient launches are flushed): the
        buckets started up to here really overlapped backward."""
        self._in_backward = len(self._launched)

    def wrote(self, params):
        """The gradient of each given parameter has been fully written by work already ENQUEUED on the current stream or on
        the weight-gradient stream."""
        if self.world == 1:
            return
        for p_ in params:
            k = self._bucket_of.get(id(p_))
            if k is None or id(p_) in self._seen:
                continue
            self._seen.add(id(p_))
            self._left[k] -= 1
            if self._left[k] == 0:
                self._launch(k)

    def would_complete(self, params):
        """True if reporting `params` as written would complete (and so start the exchange of) some bucket: the hint that
        makes ops.flush_wgrads launch its queued gradient folds now rather than batch them further."""
        if self.world == 1:
            return False
        need = {}
        for p_ in params:
            k = self._bucket_of.get(id(p_))
            if k is not None and id(p_) not in self._seen and k not in self._launched:
                need.setdefault(k, set()).add(id(p_))
        return any(len(v) == self._left[k] for k, v in need.items())

    def _launch(self, k):
        if k in self._launched:
            return
        self._launched.add(k)
        a, b = self.slices[k]
        buf = self.g[a:b]
        if self.comm is None:                            # CPU tensors (gloo): plain async all-reduce
            self._works.append((dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True), None, None))
            return
        self.comm.wait_stream(torch.cuda.current_stream())
        for st in (self.side or ()):
            self.comm.wait_stream(st)
        with torch.cuda.stream(self.comm):
            if self.via_host:
                h = buf.to("cpu", non_blocking=False)
                self._works.append((dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group, async_op=True), h, buf))
            else:
                self._works.append((dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group, async_op=True), None, None))

    def finish(self):
        """Exchange every bucket not started yet, wait for all of them; returns the factor that turns the summed gradient
        into the mean (handed to AdamW as grad_scale)."""
        if self.world == 1:
            return 1.0
        self.started_before_finish = len(self._launched)
        self.overlapped_last_step = self._in_backward if self._in_backward is not None else len(self._launched)
        for k in reversed(range(len(self.slices))):      # last layers first
            self._launch(k)
        for w, h, buf in self._works:
            w.wait()                                     # nccl: the current stream waits for the collective
            if h is not None:
                buf.copy_(h)
        self._works = []
        return 1.0 / self.world

    def __call__(self):
        """Whole exchange at once (no overlap): every bucket, last layers first."""
        self.begin_step()
        return self.finish()


T_SAMPLERS = ("loss_second_moment",)


class LossSecondMomentSampler:
    """Loss-aware timestep sampling (Nichol & Dhariwal 2021, section 3.3): t is drawn with p_t proportional to
    sqrt(E[l_t^2]), estimated from the last `history_per_term` row losses seen at each timestep, mixed with `uniform_prob` of the
    uniform distribution; the loss of a row is then weighted by iw_t = 1 / (n p_t), which keeps the step loss an unbiased
    estimate of the uniform-t loss.  Until every timestep in [1, T) has a full history the draw is uniform and iw_t = 1 exactly.
    DESIGN.md section 6m has the semantics.

    Everything lives on the device and is decided there: `update` is one launch of one workgroup (afd_tsampler_tick) that folds
    a batch of (t, row loss) into the history and rebuilds the distribution and the two tables the loss kernels read (`wtab` =
    base weight * iw, `vwtab` = iw), `draw` is one launch (afd_tsampler_draw); nothing here synchronises.  TrainStep(t_sampler=)
    drives it.  `probabilities`, `weights`, `warmed_up` and `loss_by_timestep` read the device buffers (a copy and, for the two
    host values, a sync per access)."""

    LO = 1              # the smallest timestep Diffusion.sample_timesteps returns

    def __init__(self, diffusion, history_per_term=10, uniform_prob=0.001):
        who = "LossSecondMomentSampler"
        if isinstance(history_per_term, bool) or not isinstance(history_per_term, int) or history_per_term < 1:
            raise ValueError(f"{who}: history_per_term must be an integer >= 1 (got {history_per_term!r})")
        if isinstance(uniform_prob, bool) or not isinstance(uniform_prob, (int, float)) or not 0.0 <= uniform_prob < 1.0:
            raise ValueError(f"{who}: uniform_prob must lie in [0, 1) (got {uniform_prob!r})")
        T = int(diffusion.noise_steps)
        if T < 2:
            raise ValueError(f"{who}: needs noise_steps >= 2 (got {T})")
        self.T, self.H, self.uniform_prob = T, history_per_term, float(uniform_prob)
        dev = diffusion.alpha_hat.device
        self.device = dev
        self.hist = torch.zeros(T, self.H, device=dev, dtype=torch.float64)
        self.count = torch.zeros(T, device=dev, dtype=torch.int32)
        self.prob = torch.zeros(T, device=dev, dtype=torch.float64)
        self.cdf = torch.zeros(T - self.LO, device=dev, dtype=torch.float64)
        self.wtab = torch.zeros(T, device=dev, dtype=torch.float32)
        self.vwtab = torch.zeros(T, device=dev, dtype=torch.float32)
        self.warm = torch.zeros(1, device=dev, dtype=torch.int32)
        self.w_base = None          # (T,) fp32 device table of the loss's own weights (TrainStep(loss_weighting=)), or None for 1
        self._rows = {}             # B -> the (B,) fp64 buffer the step's row-loss launch writes (static under a captured step)
        self._refresh()

    def buffers(self):
        """Every device buffer a step changes: what a captured step's warm-up saves and puts back."""
        return (self.hist, self.count, self.prob, self.cdf, self.wtab, self.vwtab, self.warm)

    def rows_buffer(self, B):
        if B not in self._rows:
            self._rows[B] = torch.zeros(B, device=self.device, dtype=torch.float64)
        return self._rows[B]

    def _refresh(self):
        """Rebuild the distribution and the tables from the history as it stands: a tick whose one row is skipped (NaN)."""
        t = torch.full((1,), self.LO, device=self.device, dtype=torch.long)
        self.update(t, torch.full((1,), float("nan"), device=self.device, dtype=torch.float64))

    def set_base_weights(self, w_base):
        """w_base: the (T,) fp32 device table the loss multiplies each row by apart from the importance weight, or None."""
        if w_base is not None and (not isinstance(w_base, torch.Tensor) or tuple(w_base.shape) != (self.T,)):
            raise ValueError(f"LossSecondMomentSampler: w_base must be a ({self.T},) tensor or None")
        self.w_base = None if w_base is None else w_base.to(self.device, torch.float32).contiguous()
        self._refresh()

    def draw(self, n, u=None, out=None):
        """n timesteps in [1, T) from the current distribution -> (n,) int64 device tensor (`out` when given).  u: (n,) fp64 device
        tensor in [0, 1) [default: torch.rand on the device, so torch's CPU generator does not advance]."""
        if u is None:
            u = torch.rand(n, device=self.device, dtype=torch.float64)
        if not isinstance(u, torch.Tensor) or tuple(u.shape) != (n,):
            raise ValueError(f"LossSecondMomentSampler.draw: u must hold {n} values")
        return ops.tsampler_draw(self.cdf, u, self.LO, out)

    def update(self, t, rows):
        """Fold a batch into the history, in batch order, and rebuild the distribution: t (B,) int64, rows (B,) fp64 row losses
        with the importance weight removed (ops.loss_rows / ops.lvar_loss_rows), both on the device.  Non-finite rows are skipped."""
        ops.tsampler_tick(t, rows, self.hist, self.count, self.LO, self.uniform_prob, self.w_base, self.prob, self.cdf, self.wtab,
                          self.vwtab, self.warm)

    def probabilities(self):
        """(T,) fp64 device copy of p_t (p_0 = 0)."""
        return self.prob.clone()

    def weights(self):
        """(T,) fp32 device copy of the importance weights iw_t = 1 / (n p_t) (1 before warm-up and at t = 0)."""
        return self.vwtab.clone()

    @property
    def warmed_up(self):
        """Whether every timestep in [1, T) has a full history.  One D2H copy."""
        return bool(self.warm.item())

    def loss_by_timestep(self):
        """The per-timestep loss record: ((T,) fp64 mean of each timestep's history, NaN where nothing was seen; (T,) int32
        counts), device copies."""
        count = self.count.clone()
        seen = torch.arange(self.H, device=self.device)[None, :] < count[:, None]
        mean = (self.hist * seen).sum(dim=1) / count.to(torch.float64)
        return torch.where(count > 0, mean, torch.full_like(mean, float("nan"))), count

    def state_dict(self):
        return {"hist": self.hist.cpu(), "count": self.count.cpu(), "history_per_term": self.H, "uniform_prob": self.uniform_prob}

    def load_state_dict(self, state):
        hist, count = torch.as_tensor(state["hist"]), torch.as_tensor(state["count"])
        if tuple(hist.shape) != (self.T, self.H) or tuple(count.shape) != (self.T,) or int(state["history_per_term"]) != self.H:
            raise ValueError(f"LossSecondMomentSampler.load_state_dict: the state is for another (T, history_per_term) than "
                             f"({self.T}, {self.H})")
        self.uniform_prob = float(state["uniform_prob"])
        self.hist.copy_(hist.to(torch.float64))
        self.count.copy_(count.to(torch.int32))
        self._refresh()


def label_dropout_mask(n, p_uncond):
    """(n,) bool mask of the samples whose class label a classifier-free-guidance step drops (replaces by NULL_LABEL): each
    with probability p_uncond, drawn from torch's CPU global generator like Diffusion.sample_timesteps."""
    return torch.rand(n) < p_uncond


class TrainStep:
    """The reference's per-batch body (ddpm_utils.py:499-507) as one callable:
         t -> noise_images -> UNet -> MSE -> zero_grad -> backward -> [all-reduce] -> AdamW.
    `graph=True` captures the device work into a hipGraph on first use (static shapes): the whole step on
    one GPU; with data parallelism everything up to and including backward -- the gradient all-reduce
    (one 23.6 MB exchange) and AdamW then run after the replay.  The CPU-generator timestep draw and the
    H2D copies always stay outside the graph.
    `graph="lanes"` captures the same graph but never launches it: csrc/replay.hip walks its nodes once and re-issues
    them on TWO REAL STREAMS from a C++ loop (weight-gradient kernels on the side stream, cross-lane dependencies as
    events) -- the eager step's stream semantics with ~0.7 instead of 5.6 ms of host time per step and none of a
    hipGraph launch's cross-branch cost: 6.79 / 6.84 / 7.00 ms (lanes / eager / hipGraph) at B = 256, 3.7 / 5.2 / 4.0 at
    B = 16, bit-identical to the eager step.  The noise is drawn outside the replayed list (no generator state in it)."""

    def __init__(self, model, diffusion, lr, graph=False, distributed=None, n_buckets=4, overlap_wgrad=None, conditional=False,
                 p_uncond=0.0, ema=None, ema_model=None, ema_start=2000, max_grad_norm=None, lr_schedule=None, skip_nonfinite=False,
                 track_grad_norm=False, loss_weighting=None, snr_gamma=5.0, vlb_lambda=0.001, t_sampler=None):
        """conditional=True: the step takes class labels (`step(images, y=labels)`, UNet.forward(x, t, y): ddpm_models.py:276-277)
        and `label_emb` is optimised and exchanged like every other parameter.  With the default (the reference's loop,
        ddpm_utils.py:502, never passes labels) `label_emb` stays untouched, as under the reference's AdamW, and passing y raises.
        p_uncond > 0 (needs conditional=True): label dropout for classifier-free guidance -- each sample's label is replaced by
        NULL_LABEL with probability p_uncond, the mask drawn from the CPU generator right after the timesteps
        (label_dropout_mask), outside any captured work.  p_uncond = 0 draws nothing.
        ema (an EMA) with ema_model (a copy of model, e.g. copy.deepcopy(model)): keep an exponential moving average of the weights
        in ema_model -- the reference's `ema.step_ema(ema_model, model, step_start_ema=ema_start)` after every optimizer step.  The
        update is fused into the AdamW launch (afd_adamw_ema_tick + afd_adamw_ema_step instead of afd_adamw_tick + afd_adamw_step:
        no extra launch), in every launch mode and under data parallelism; ema.beta is read here, once.  `ema.step` counts the
        calls to this step (the host mirror of the device counter).
        max_grad_norm / lr_schedule (an LRSchedule; `lr` is its base rate) / skip_nonfinite / track_grad_norm: gradient clipping by
        the global L2 norm and a learning-rate schedule, decided on the device between backward and AdamW (FusedAdamW has the
        semantics): at most one launch more than the default step, none with all four at their defaults, and the same results in
        every launch mode, with ema=, with conditional= and under data parallelism (the norm is taken after the all-reduce; no
        extra collective).  `last_grad_norm`, `last_lr`, `n_skipped` read the device buffer `opt.ctl` (one D2H copy per access).
        With skip_nonfinite a dropped update does not advance the EMA either, while `ema.step` still counts the call.
        The objective: the network is trained towards `diffusion.training_target` for `diffusion.prediction` ("eps", "v" or "x0"),
        and loss_weighting="min_snr" weights each sample's squared error by `diffusion.snr_weights("min_snr", snr_gamma)[t]`
        ("truncated_snr": `diffusion.snr_weights("truncated_snr")[t]`, the weight progressive distillation trains with):
          L = (1 / (B C H W)) sum_b w[t_b] sum_i (pred - target)^2
        normalised by the element count, not by sum w, so data-parallel ranks average losses and gradients exactly as for the
        plain MSE, with no extra collective.  Anything but eps-prediction without weighting runs ops.objective_loss, which forms
        the target inside the loss kernels: the same number of launches as ops.mse_loss, in every launch mode.  The weight table
        is a static device buffer built here, once.
        With diffusion.variance == "learned" (the model is UNet(c_in=C, c_out=2 C)) the step trains the hybrid loss of Nichol &
        Dhariwal 2021, L = L_simple + vlb_lambda (T - 1) L_vlb: L_simple is the objective above on the output's prediction half,
        L_vlb the batch mean of the variational bound's term of each sample's timestep in bits per dimension, with the mean
        stopped, so it trains the variance half alone (ops.lvar_loss: the same number of launches again, in every launch mode,
        with loss_weighting=, ema=, clipping, conditional= and under data parallelism; normalised by the element count like
        L_simple).  `last_vlb` is the last step's L_vlb, a 0-d device tensor.  vlb_lambda is ignored with a fixed variance.
        t_sampler: None (the step as it always was: t from torch's CPU generator, uniform), "loss_second_moment" or a
        LossSecondMomentSampler: the timesteps are drawn on the device with p_t proportional to sqrt(E[l_t^2]) and every row's
        loss is weighted by iw_t = 1 / ((T - 1) p_t), through the tables the loss kernels already read (w = wtab, and vw = vwtab
        for the bound's terms).  Two launches more than the default step, both inside whatever is captured: the per-row losses
        after the loss forward (ops.loss_rows / ops.lvar_loss_rows on the detached output) and the sampler's tick after backward,
        on the main stream behind the loss backward that reads wtab.  The draw runs outside any captured work and writes the
        step's static t buffer.  A caller-supplied t is used as it is and still gets wtab[t].  The loss returned, and `last_vlb`,
        are then the importance-weighted estimates.  Not with data parallelism (each rank would need the others' (t, l): one
        more collective) -- ValueError."""
        _check_opt_ctl("TrainStep", max_grad_norm, lr_schedule)
        if loss_weighting is not None and not (isinstance(loss_weighting, str) and loss_weighting in Diffusion.LOSS_WEIGHTINGS):
            raise ValueError(f"TrainStep: unknown loss_weighting {loss_weighting!r} (None, 'min_snr' or 'truncated_snr')")
        if isinstance(snr_gamma, bool) or not isinstance(snr_gamma, (int, float)) or not snr_gamma > 0 or not math.isfinite(snr_gamma):
            raise ValueError(f"TrainStep: snr_gamma must be a finite number > 0 (got {snr_gamma!r})")
        if (ema is None) != (ema_model is None):
            raise ValueError("TrainStep: ema and ema_model go together (EMA(beta) and a copy of the model): got only one of them")
        if ema is not None and (isinstance(ema_start, bool) or int(ema_start) != ema_start or ema_start < 0):
            raise ValueError(f"TrainStep: ema_start must be an integer >= 0 (got {ema_start!r})")
        if ema is not None and ema._driver is not None:
            raise ValueError("TrainStep: this EMA is already driven by another TrainStep")
        if not 0.0 <= p_uncond <= 1.0:
            raise ValueError(f"TrainStep: p_uncond must lie in [0, 1] (got {p_uncond})")
        if p_uncond > 0 and not conditional:
            raise ValueError("TrainStep: p_uncond > 0 drops class labels, which needs a conditional step (conditional=True)")
        if isinstance(vlb_lambda, bool) or not isinstance(vlb_lambda, (int, float)) or not vlb_lambda >= 0 or not math.isfinite(vlb_lambda):
            raise ValueError(f"TrainStep: vlb_lambda must be a finite number >= 0 (got {vlb_lambda!r})")
        if t_sampler is not None and not isinstance(t_sampler, LossSecondMomentSampler) \
                and not (isinstance(t_sampler, str) and t_sampler in T_SAMPLERS):
            raise ValueError(f"TrainStep: unknown t_sampler {t_sampler!r} (None, 'loss_second_moment' or a LossSecondMomentSampler)")
        if t_sampler is not None and (distributed if distributed is not None else dist.is_initialized()):
            raise ValueError("TrainStep: t_sampler does not work with data parallelism (every rank would need the other ranks' "
                             "timesteps and row losses: one more collective)")
        self.model, self.diffusion = model, diffusion
        self.learned = getattr(diffusion, "variance", "fixed") == "learned"
        self.vlb_lambda = float(vlb_lambda)
        self.last_vlb = None             # L_vlb of the last step (0-d device tensor; a static buffer under graph=True / "lanes")
        if hasattr(diffusion, "check_model"):
            diffusion.check_model(model, None, "TrainStep")
        self.conditional = conditional
        self.p_uncond = float(p_uncond)
        self.last_labels = None          # the labels the last call trained on, after dropout
        self.prediction = getattr(diffusion, "prediction", "eps")
        self.loss_weighting, self.snr_gamma = loss_weighting, float(snr_gamma)
        self.loss_weights = None         # (T,) fp32 device table w[t], or None for the unweighted loss
        if loss_weighting is not None:
            self.loss_weights = diffusion.snr_weights(loss_weighting, snr_gamma).float().to(diffusion.alpha_hat.device).contiguous()
        self.t_sampler = LossSecondMomentSampler(diffusion) if isinstance(t_sampler, str) else t_sampler
        if self.t_sampler is not None:
            if self.t_sampler.T != diffusion.noise_steps:
                raise ValueError(f"TrainStep: the t_sampler was built for {self.t_sampler.T} noise steps, the diffusion has {diffusion.noise_steps}")
            self.t_sampler.set_base_weights(self.loss_weights)
        # weight-gradient kernels on a second stream (ops._GradMode.side): off the critical path of backward, they fill
        # the CUs the dependent chain of small kernels leaves idle.  Measured on MI355X (B=256): eager 12.0 -> 11.1
        # ms/step, captured graph 11.45 -> 11.3 (forks batched 16 layers at a time: every fork is a cross-stream edge
        # in the graph, and 57 of them cost more than the overlap returns).  Layers per fork, eager: 1 / 2 / 4 / 8 / 16 ->
        # 9.77 / 9.67 / 9.66 / 9.87 / 9.95 ms.  (Stream priorities: see _main_hi below.)
        if overlap_wgrad is None:
            overlap_wgrad = True
        n_side = int(os.environ.get("AFD_WGRAD_STREAMS", 1))                                # side streams (tuning hook)
        prio = int(os.environ.get("AFD_WGRAD_PRIO", 0))                                   # side-stream priority (tuning hook; larger = lower)
        self.wgrad_stream = [torch.cuda.Stream(priority=prio) for _ in range(max(1, n_side))] if overlap_wgrad else None
        if overlap_wgrad and torch.cuda.is_available() and os.environ.get("AFD_WGRAD_INSITU", "0") == "1":
            # opt-in: the 3x3 weight gradients on 160 workgroups per launch instead of one per CU -- 26 % slower alone, but beside the
            # dependent chain they leave CUs to it and write fewer slabs (step 7.14 -> 7.07 ms: csrc/bf3_wgrad.hip).  Off by default so
            # that the step and the per-kernel roofline table of bench.py run ONE plan; process-wide, like every plan switch.
            # (Measured with the eight-wave workgroups.  The four-wave workgroups that are the default now share their CUs with
            # the chain instead, and 160 of THEM cost the step 0.33 ms: profiles/wgrad_w4_ab.txt.)
            lib().afd_debug_conv_path(49)
        # layers per fork (AFD_WGRAD_BATCH overrides, read per step: tuning hook).  Round 3, after the convolutions moved to the
        # fp16 matrix pipe (tools/ab_env.py AFD_WGRAD_BATCH, same box): 2 / 4 / 8 / 12 / 16 -> 7.49 / 7.46 / 7.32 / 7.34 / 7.34 ms
        # Re-measured with medians over windows (tools/step_median.py, separate processes): eager 4 / 6 / 8 / 10 / 12 / 16 -> 7.264 / 7.109 /
        # 7.097 / 7.133 / 7.147 / 7.182; captured 8 / 16 / 24 / 32 / 40 / 48 / 64 / 128 -> 7.343 / 7.285 / 7.220 / 7.208 / 7.299 / 7.375 / 7.361 / 7.552
        self.wgrad_batch = 8 if (not graph or graph == "lanes") else 32      # ("lanes" has the eager step's stream semantics)
        self.opt = FusedAdamW(model, lr=lr, conditional=conditional, max_grad_norm=max_grad_norm, lr_schedule=lr_schedule,
                              skip_nonfinite=skip_nonfinite, track_grad_norm=track_grad_norm)
        self.ema, self._ema_home = ema, None
        if ema is not None:
            h = ema._fast(ema_model, model)          # (model now lives in self.opt's FlatParams)
            if h is None:
                raise ValueError("TrainStep: ema_model must hold float32 parameters on the model's device")
            h.start = int(ema_start)
            h.beta, h.one_minus_beta = ema._betas()
            h.state.copy_(torch.tensor([ema.step, 0], dtype=torch.int32))      # the device counter continues the host's
            ema._driver = self
            self._ema_home = h
        want_ddp = distributed if distributed is not None else dist.is_initialized()
        self.ddp = GradAllReduce(self.opt.fp, n_buckets, model=model) if want_ddp else None
        if self.ddp is not None:
            self.ddp.side = self.wgrad_stream
        self._loss_work = None
        # Tuning hook: the dependent chain (forward, dgrads, norms, attention, AdamW) on a HIGH-priority stream, the weight gradients on a
        # normal one -- the idea being that the dispatcher hands free CUs to the chain first.  It does not pay.
        # Measured in separate processes (tools/step_median.py): 7.22 against 7.16 eager, 12.3 against 7.13 with the two-lane replay, 13.3 with a
        # graph captured on it; the weight-gradient stream at high priority instead: 14.0 -- mixed priorities make every cross-stream
        # wait expensive.  Off by default (AFD_MAIN_PRIO=1 turns it on for eager launches).
        self._main_hi = torch.cuda.Stream(priority=-1) if int(os.environ.get("AFD_MAIN_PRIO", 0)) and torch.cuda.is_available() else None
        self.use_graph = bool(graph)
        self.lanes = graph == "lanes"     # the captured step re-issued on two real streams from C++ (csrc/replay.hip)
        self._lanes_handle = None
        self._graph = None
        self._static = None
        self._wino_plan, self._wino_requests = None, None      # ops.WinoStepPlan after the first (recording) step

    last_grad_norm = property(lambda self: self.opt.last_grad_norm, doc=FusedAdamW.last_grad_norm.__doc__)
    last_lr = property(lambda self: self.opt.last_lr, doc=FusedAdamW.last_lr.__doc__)
    n_skipped = property(lambda self: self.opt.n_skipped, doc=FusedAdamW.n_skipped.__doc__)

    def __del__(self):
        h = getattr(self, "_lanes_handle", None)           # the replay list points into the captured graph: free it first
        if h is not None:
            try:
                lib().afd_replay_free(h)
            except Exception:
                pass
            self._lanes_handle = None

    def _fwd_bwd(self, images, t, eps, y=None):
        W = ops._WinoWeights
        if self._wino_plan is not None and self._wino_plan.valid():
            self._wino_plan.launch()                   # every transformed-weight image of the step, one launch
            W.active_plan = self._wino_plan
        elif self._wino_requests is None:
            self._wino_requests = W.recording = {}     # first step: note which images the dispatch asks for
        try:
            x_t, noise = self.diffusion.noise_images(images, t, eps)
            pred = self.model(x_t, t) if y is None else self.model(x_t, t, y)
            ts, rows = self.t_sampler, None
            if ts is not None:
                # the loss through the sampler's tables; the rows' own losses (importance weight removed) feed the tick below
                d, rows = self.diffusion, ts.rows_buffer(images.shape[0])
                if self.learned:
                    scale = self.vlb_lambda * (d.noise_steps - 1)
                    loss, self.last_vlb = ops.lvar_loss(pred, images, noise, t, d.alpha, d.alpha_hat, d.beta, d._lv(), ts.wtab,
                                                        self.prediction, scale, vw=ts.vwtab)
                    ops.lvar_loss_rows(pred.detach(), images, noise, t, d.alpha, d.alpha_hat, d.beta, d._lv(), self.loss_weights,
                                       self.prediction, scale, out=rows)
                else:
                    loss = ops.objective_loss(pred, images, noise, t, d.alpha_hat, ts.wtab, self.prediction)
                    ops.loss_rows(pred.detach(), images, noise, t, d.alpha_hat, self.loss_weights, self.prediction, out=rows)
            elif self.learned:
                d = self.diffusion
                loss, self.last_vlb = ops.lvar_loss(pred, images, noise, t, d.alpha, d.alpha_hat, d.beta, d._lv(), self.loss_weights,
                                                    self.prediction, self.vlb_lambda * (d.noise_steps - 1))
            elif self.prediction == "eps" and self.loss_weights is None:
                loss = ops.mse_loss(noise, pred)
            else:
                loss = ops.objective_loss(pred, images, noise, t, self.diffusion.alpha_hat, self.loss_weights, self.prediction)
            self.opt.zero_grad()
            overlap = self.ddp is not None and self.ddp.world > 1 and not self.use_graph      # (a captured backward cannot hold the exchange)
            if overlap:
                self.ddp.begin_step()                  # bucket all-reduces start during backward, as their gradients complete
            with ops.inplace_param_grads(self.wgrad_stream, int(os.environ.get("AFD_WGRAD_BATCH", self.wgrad_batch)),   # weight gradients add straight into the flat .grad views
                                         on_write=self.ddp.wrote if overlap else None,
                                         fold_hint=self.ddp.would_complete if overlap else None):
                # backward on the calling thread instead of the autograd engine's device worker thread: no hand-over of the
                # interpreter lock per node (host time of a step 6.34 -> 5.6 ms, tools/step_median.py at B = 8; AFD_BWD_THREAD=1: the engine's thread)
                if os.environ.get("AFD_BWD_THREAD", "0") == "1":
                    loss.backward()
                else:
                    with torch.autograd.set_multithreading_enabled(False):
                        loss.backward()
                if overlap:
                    self.ddp.backward_done()
            if ts is not None:
                ts.update(t, rows)                     # on the main stream: behind the loss backward, which reads wtab
        finally:
            if W.recording is not None and W.recording is self._wino_requests:
                W.recording = None
                self._wino_plan = ops.WinoStepPlan(self._wino_requests)
            W.active_plan = None
        return loss.detach()

    def _update(self):
        scale = self.ddp.finish() if self.ddp is not None else 1.0
        self.opt.step(grad_scale=scale, ema=self._ema_home)

    def _body(self, images, t, eps, y=None):
        loss = self._fwd_bwd(images, t, eps, y)
        self._update()
        return loss

    def __call__(self, images, t=None, eps=None, y=None):
        loss = self._step(images, t, eps, y)
        if self.ema is not None:
            self.ema.step += 1                          # one EMA call per step (the capture warm-up's are undone)
        return loss

    def _step(self, images, t=None, eps=None, y=None):
        """images (B,C,S,S) on the device; t (B,) int64 [default: diffusion.sample_timesteps];
        eps: injected noise or None (device RNG); y (B,) int64 class labels (only with conditional=True; NULL_LABEL = no label
        for that sample).  Under graph=True / "lanes" the labels are a static captured input like images, t and eps: a step
        captured with labels must get them on every call, one captured without must never get them.
        Returns the loss as a 0-d device tensor."""
        if y is not None and not self.conditional:
            raise ValueError("TrainStep: class labels were passed but the step was built with conditional=False: label_emb sits "
                             "outside the optimised range (FlatParams) and would never be updated; build TrainStep(..., conditional=True)")
        drawn = False                               # t was drawn on the device, straight into the captured step's static buffer
        if t is None and self.t_sampler is not None:
            drawn = self._graph is not None
            t = self.t_sampler.draw(images.shape[0], out=self._static["t"] if drawn else None)
        elif t is None:
            t = self.diffusion.sample_timesteps(images.shape[0])
        t = t.to(images.device, non_blocking=True)
        if y is not None:
            y = torch.as_tensor(y)
            if self.p_uncond > 0:
                drop = label_dropout_mask(images.shape[0], self.p_uncond)
                y = y.masked_fill(drop.to(y.device), ops.NULL_LABEL)
            y = y.to(images.device, non_blocking=True)
            self.last_labels = y
        if self.lanes and eps is None:
            eps = torch.randn_like(images)          # drawn outside: the replayed list holds no generator state
        if not self.use_graph:
            if self._main_hi is not None:             # the dependent chain on the high-priority stream, joined with the caller's on both sides
                cur = torch.cuda.current_stream()
                self._main_hi.wait_stream(cur)
                with torch.cuda.stream(self._main_hi):
                    loss = self._body(images, t, eps, y)
                cur.wait_stream(self._main_hi)
                return loss
            return self._body(images, t, eps, y)
        whole = self.ddp is None                    # single GPU: AdamW is captured too
        if self._graph is None:
            self._static = {"images": images.clone(), "t": t.clone(), "eps": None if eps is None else eps.clone(),
                            "y": None if y is None else y.clone()}
            st = self._static
            # warm-up outside capture (allocator, lazy init, the Winograd plan's recording step).  These are real steps on
            # the first batch, so everything they change is put back afterwards -- parameters, AdamW moments and step
            # counter, the clip / schedule control buffer, the EMA buffer and its counter, the device generator -- and under data parallel they stop before the
            # exchange: the first graph call is then exactly one step, like the eager one (and like the reference's).
            bufs = self.opt.state_buffers()
            bufs += self._ema_home.state_buffers() if self._ema_home is not None else ()
            bufs += self.t_sampler.buffers() if self.t_sampler is not None else ()
            keep = [b.clone() for b in bufs]
            rng = torch.cuda.get_rng_state(images.device)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    (self._body if whole else self._fwd_bwd)(st["images"], st["t"], st["eps"], st["y"])
            torch.cuda.current_stream().wait_stream(s)
            for b, k in zip(bufs, keep):
                b.copy_(k)
            torch.cuda.set_rng_state(rng, images.device)
            ops.bump_param_epoch()
            self._graph = torch.cuda.CUDAGraph(keep_graph=True) if self.lanes else torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                st["loss"] = (self._body if whole else self._fwd_bwd)(st["images"], st["t"], st["eps"], st["y"])
            if self.lanes:
                import ctypes
                h, counts = ctypes.c_void_p(), (ctypes.c_int * 4)()
                lib().afd_replay_build(self._graph.raw_cuda_graph(), ctypes.byref(h), counts)
                self._lanes_handle, self.lanes_counts = h, tuple(counts)      # (work nodes, main lane, side lane, cross-lane waits)
        st = self._static
        if (eps is None) != (st["eps"] is None):
            raise ValueError("TrainStep(graph=True): the step was captured " + ("without" if st["eps"] is None else "with") +
                             " injected noise; `eps` must be passed (or omitted) on every call alike")
        if (y is None) != (st["y"] is None):
            raise ValueError("TrainStep(graph=True): the step was captured " + ("without" if st["y"] is None else "with") +
                             " class labels; `y` must be passed (or omitted) on every call alike")
        st["images"].copy_(images)
        if not drawn:
            st["t"].copy_(t)
        if y is not None:
            st["y"].copy_(y)
        if eps is not None:
            st["eps"].copy_(eps)
        if self.lanes:
            lib().afd_replay_run(self._lanes_handle, torch.cuda.current_stream().cuda_stream, self.wgrad_stream[0].cuda_stream)
        else:
            self._graph.replay()
        ops.bump_param_epoch()                          # the replayed AdamW moved the parameters
        if not whole:
            self.ddp.begin_step()                       # the replayed backward reported nothing: exchange everything now
            self._update()
        return st["loss"]


class DistillStep:
    """One training step of progressive distillation (Salimans & Ho 2022): the student learns to do in ONE DDIM step what the
    frozen teacher does in TWO.  Per call: draw a student step index k per row, gather the row timesteps (t, t_mid, t_prev) of
    `chain` on the device, `diffusion.distill_targets` (two eager teacher forwards under no_grad and three elementwise
    launches), then the inner TrainStep on (x_tilde, t, eps_tilde): it re-forms z_t = sqrt(a_t) x_tilde + sqrt(1 - a_t) eps_tilde
    and trains towards diffusion.training_target(x_tilde, eps_tilde, t), so every TrainStep feature (graph=False | True | "lanes",
    ema=, clipping, schedules, conditional=, data parallelism) works as it is -- the teacher's forwards run outside whatever the
    inner step captured.  The teacher's parameters are never touched.  `.step` is the inner TrainStep; the student's chain
    afterwards is `Diffusion.halve_chain(chain)`, sampled with `diffusion.sample(student, steps=that chain)`."""

    def __init__(self, student, teacher, diffusion, chain, lr, loss_weighting="truncated_snr", **train_step_kw):
        if student is teacher:
            raise ValueError("DistillStep: student is teacher: the teacher must stay frozen (student = copy.deepcopy(teacher))")
        if getattr(diffusion, "variance", "fixed") == "learned":
            raise ValueError("DistillStep: variance='learned' is not supported (the student's step is deterministic DDIM)")
        if train_step_kw.get("t_sampler") is not None:
            raise ValueError("DistillStep: t_sampler is not supported (the step draws positions of the chain, not timesteps)")
        levels = diffusion.distill_levels(chain)              # ValueError for an odd, unordered or out-of-range chain
        if diffusion.prediction == "eps":
            logging.warning("DistillStep: prediction='eps' is unstable at few sampling steps (Salimans & Ho 2022, section 4); "
                            "'v' or 'x0' is the parametrisation to distil with")
        self.student, self.teacher, self.diffusion = student, teacher, diffusion
        self.chain = [int(v) for v in chain]
        self.n_steps = levels[0].numel()
        dev = diffusion.alpha_hat.device
        self.levels = tuple(tab.to(dev).contiguous() for tab in levels)          # (t, t_mid, t_prev), (N,) int64 each
        self.step = TrainStep(student, diffusion, lr, loss_weighting=loss_weighting, **train_step_kw)

    def __call__(self, images, k=None, eps=None, y=None):
        """images (B, C, S, S) on the device; k (B,) student step indices in [0, N) [default: diffusion.sample_distill_steps];
        eps: injected noise or None (device RNG); y: class labels, handed to the teacher's forwards and the inner step.
        Returns the inner step's loss, a 0-d device tensor."""
        B = images.shape[0]
        if k is None:
            k = self.diffusion.sample_distill_steps(B, self.n_steps)
        k = torch.as_tensor(k)
        if k.dtype.is_floating_point or k.dtype == torch.bool or tuple(k.shape) != (B,):
            raise ValueError(f"DistillStep: k must hold {B} integer step indices, one per image")
        if not k.is_cuda and (int(k.min()) < 0 or int(k.max()) >= self.n_steps):
            raise ValueError(f"DistillStep: every step index must lie in [0, {self.n_steps})")
        k = k.to(images.device, non_blocking=True).long()
        rows = tuple(tab[k] for tab in self.levels)
        x_tilde, eps_tilde, t = self.diffusion.distill_targets(self.teacher, images, rows, self.chain, eps, y)
        return self.step(x_tilde, t, eps_tilde, y)


def progressive_distill(model, diffusion, dataloader, start_steps, end_steps, iters_per_round, lr, device, ema_beta=None,
                        on_round=None, **train_step_kw):
    """Progressive distillation: halve the DDIM chain of `model` round after round, from start_steps to end_steps sampling steps.
    start_steps = end_steps * 2^R with R >= 1 and start_steps <= T - 1 (ValueError otherwise, before any device work).  Round 0's
    teacher is `model` on chain = diffusion.ddim_timesteps(start_steps); each round makes student = copy.deepcopy(teacher), runs a
    DistillStep for iters_per_round steps over the loader (cycled; batches are (images, ...) tuples or tensors) with
    LRSchedule("linear", total=iters_per_round), the paper's per-round decay to zero, then teacher = student and
    chain = halve_chain(chain).  ema_beta: also keep EMA(ema_beta) of each round's student, fused into its AdamW launch from the
    first step; the next round's teacher is the student itself, the average is handed to on_round.  on_round(info, student,
    ema_model) is called after every round.  **train_step_kw go to every round's inner TrainStep (graph=, max_grad_norm=, ...).
    Single-process.  -> (the last student, [{"steps", "chain", "mean_loss"} per round]); `model` is left as it was."""
    import copy
    T = diffusion.noise_steps
    ok = all(isinstance(v, int) and not isinstance(v, bool) for v in (start_steps, end_steps, iters_per_round))
    if not ok or end_steps < 1 or iters_per_round < 1:
        raise ValueError(f"progressive_distill: start_steps, end_steps and iters_per_round must be integers >= 1 "
                         f"(got {start_steps!r}, {end_steps!r}, {iters_per_round!r})")
    ratio = start_steps // end_steps
    if start_steps % end_steps or ratio < 2 or ratio & (ratio - 1):
        raise ValueError(f"progressive_distill: start_steps must be end_steps * 2^R with R >= 1 (got {start_steps} and {end_steps})")
    if start_steps > T - 1:
        raise ValueError(f"progressive_distill: start_steps must lie in [2, {T - 1}] (got {start_steps})")
    for bad in ("lr_schedule", "ema", "ema_model", "ema_start"):
        if bad in train_step_kw:
            raise ValueError(f"progressive_distill: {bad} is set per round here (pass ema_beta for an average)")
    chain = diffusion.ddim_timesteps(start_steps)
    teacher, rounds, batches = model, [], None
    while len(chain) > end_steps:
        student = copy.deepcopy(teacher)
        kw = dict(train_step_kw)
        ema_model = None
        if ema_beta is not None:
            ema_model = copy.deepcopy(student)
            kw.update(ema=EMA(ema_beta), ema_model=ema_model, ema_start=0)
        step = DistillStep(student, teacher, diffusion, chain, lr, lr_schedule=LRSchedule("linear", total=iters_per_round), **kw)
        total = torch.zeros((), device=device)
        for _ in range(iters_per_round):
            batch = None if batches is None else next(batches, None)
            if batch is None:                                      # cycle the loader
                batches = iter(dataloader)
                batch = next(batches)
            images = batch[0] if isinstance(batch, (tuple, list)) else batch
            total += step(images.to(device))
        chain = Diffusion.halve_chain(chain)
        info = {"steps": len(chain), "chain": list(chain), "mean_loss": total.item() / iters_per_round}
        rounds.append(info)
        logging.info(f"progressive_distill: {2 * len(chain)} -> {len(chain)} steps, mean loss {info['mean_loss']:.6f}")
        if on_round is not None:
            on_round(info, student, ema_model)
        teacher = student
    return teacher, rounds


class ConsistencyStep:
    """One training step of consistency distillation (Song et al. 2023; Luo et al. 2023 for this discrete-time form over a DDIM
    chain with skipped steps): the student's consistency function f(z_t, t) = c_skip[t] z_t + c_out[t] x_hat(z_t, t) learns to
    equal the TARGET network's f at the point one teacher DDIM step further down the chain, f(z_prev, t_prev), so that in the end
    every point of a trajectory maps to its origin and the student samples in 1 to 4 forwards (`Diffusion.consistency_sample`).
    Per call: draw a position k of `chain` per row, gather (t, t_prev) on the device, `diffusion.consistency_targets` (one eager
    teacher forward and one of the target network, under no_grad, and three elementwise launches), then the inner TrainStep on
    (x_tilde, t, eps_tilde): it re-forms z_t and trains towards diffusion.training_target(x_tilde, eps_tilde, t), so every
    TrainStep launch mode (graph=False | True | "lanes"), clipping, schedules, conditional= and data parallelism work as they
    are.  The target network `.target` is a deep copy of the student, kept as the exponential moving average of its weights with
    rate target_beta by the EMA fused into the inner step's AdamW launch (ema_start = 0): no extra launch.  It is the network to
    sample from.  The loss weight is a choice of the paper's lambda(t_n): the "truncated_snr" table on the x0 error, on which the
    squared distance between the two f is c_out[t]^2 times the x0 error.  The teacher's parameters are never touched.  `.step` is
    the inner TrainStep."""

    def __init__(self, student, teacher, diffusion, chain, lr, target_beta=0.95, sigma_data=0.5, timestep_scaling=10.0,
                 loss_weighting="truncated_snr", **train_step_kw):
        import copy
        if student is teacher:
            raise ValueError("ConsistencyStep: student is teacher: the teacher must stay frozen (student = copy.deepcopy(teacher))")
        if getattr(diffusion, "variance", "fixed") == "learned":
            raise ValueError("ConsistencyStep: variance='learned' is not supported (the consistency function is deterministic)")
        for bad in ("ema", "ema_model", "ema_start", "t_sampler"):
            if bad in train_step_kw:
                raise ValueError(f"ConsistencyStep: {bad} is not supported (the step keeps its target network with the inner "
                                 f"step's EMA, see target_beta, and draws positions of the chain, not timesteps)")
        if isinstance(target_beta, bool) or not isinstance(target_beta, (int, float)) or not 0.0 <= target_beta < 1.0:
            raise ValueError(f"ConsistencyStep: target_beta must lie in [0, 1) (got {target_beta!r})")
        levels = diffusion.consistency_levels(chain)          # ValueError for an unordered or out-of-range chain
        coef = diffusion.consistency_coefficients(sigma_data, timestep_scaling)       # and for bad sigma_data / timestep_scaling
        if diffusion.prediction == "eps":
            logging.warning("DistillStep: prediction='eps' is unstable at few sampling steps (Salimans & Ho 2022, section 4); "
                            "'v' or 'x0' is the parametrisation to distil with")
        self.student, self.teacher, self.diffusion = student, teacher, diffusion
        self.chain = [int(v) for v in chain]
        self.n_steps = levels[0].numel()
        self.sigma_data, self.timestep_scaling = float(sigma_data), float(timestep_scaling)
        dev = diffusion.alpha_hat.device
        self.levels = tuple(tab.to(dev).contiguous() for tab in levels)          # (t, t_prev), (N,) int64 each
        self.coef = coef.to(dev).contiguous()                                      # (T, 2) fp64
        self.target = copy.deepcopy(student)
        self.step = TrainStep(student, diffusion, lr, loss_weighting=loss_weighting, ema=EMA(float(target_beta)),
                              ema_model=self.target, ema_start=0, **train_step_kw)

    def __call__(self, images, k=None, eps=None, y=None):
        """images (B, C, S, S) on the device; k (B,) positions of the chain in [0, N) [default: diffusion.sample_distill_steps];
        eps: injected noise or None (device RNG); y: class labels, handed to both forwards and the inner step.
        Returns the inner step's loss, a 0-d device tensor."""
        B = images.shape[0]
        if k is None:
            k = self.diffusion.sample_distill_steps(B, self.n_steps)
        k = torch.as_tensor(k)
        if k.dtype.is_floating_point or k.dtype == torch.bool or tuple(k.shape) != (B,):
            raise ValueError(f"ConsistencyStep: k must hold {B} integer positions, one per image")
        if not k.is_cuda and (int(k.min()) < 0 or int(k.max()) >= self.n_steps):
            raise ValueError(f"ConsistencyStep: every position must lie in [0, {self.n_steps})")
        k = k.to(images.device, non_blocking=True).long()
        rows = tuple(tab[k] for tab in self.levels)
        x_tilde, eps_tilde, t = self.diffusion.consistency_targets(self.teacher, self.target, images, rows, self.chain, self.coef,
                                                                   eps, y)
        return self.step(x_tilde, t, eps_tilde, y)


def consistency_distill(model, diffusion, dataloader, steps, iters, lr, device, target_beta=0.95, on_done=None, **train_step_kw):
    """Consistency distillation of `model` in ONE training run: the teacher is `model` on chain = diffusion.ddim_timesteps(steps),
    the student a deep copy of it, trained by a ConsistencyStep for `iters` steps over the loader (cycled; batches are (images, ...)
    tuples or tensors) with LRSchedule("linear", total=iters) unless the caller passes lr_schedule=.  steps in [1, T - 1] and
    iters >= 1 are integers (ValueError otherwise, before any device work).  on_done(info, student, target) is called at the end.
    **train_step_kw go to the ConsistencyStep (sigma_data=, timestep_scaling=, loss_weighting=) and its inner TrainStep (graph=,
    max_grad_norm=, ...).  Single-process.  -> (the target network, the one to sample with `diffusion.consistency_sample`,
    {"chain", "mean_loss"}); `model` is left as it was."""
    import copy
    T = diffusion.noise_steps
    ok = all(isinstance(v, int) and not isinstance(v, bool) for v in (steps, iters))
    if not ok or iters < 1:
        raise ValueError(f"consistency_distill: steps and iters must be integers >= 1 (got {steps!r}, {iters!r})")
    if not 1 <= steps <= T - 1:
        raise ValueError(f"consistency_distill: steps must lie in [1, {T - 1}] (got {steps})")
    for bad in ("ema", "ema_model", "ema_start", "t_sampler"):
        if bad in train_step_kw:
            raise ValueError(f"consistency_distill: {bad} is not supported (the target network is the step's average: target_beta)")
    if isinstance(target_beta, bool) or not isinstance(target_beta, (int, float)) or not 0.0 <= target_beta < 1.0:
        raise ValueError(f"consistency_distill: target_beta must lie in [0, 1) (got {target_beta!r})")
    if getattr(diffusion, "variance", "fixed") == "learned":
        raise ValueError("consistency_distill: variance='learned' is not supported (the consistency function is deterministic)")
    chain = diffusion.ddim_timesteps(steps)
    kw = dict(train_step_kw)
    kw.setdefault("lr_schedule", LRSchedule("linear", total=iters))
    student = copy.deepcopy(model)
    step = ConsistencyStep(student, model, diffusion, chain, lr, target_beta=target_beta, **kw)
    total, batches = torch.zeros((), device=device), None
    for _ in range(iters):
        batch = None if batches is None else next(batches, None)
        if batch is None:                                      # cycle the loader
            batches = iter(dataloader)
            batch = next(batches)
        images = batch[0] if isinstance(batch, (tuple, list)) else batch
        total += step(images.to(device))
    info = {"chain": list(chain), "mean_loss": total.item() / iters}
    logging.info(f"consistency_distill: {len(chain)} teacher steps, {iters} iterations, mean loss {info['mean_loss']:.6f}")
    if on_done is not None:
        on_done(info, student, step.target)
    return step.target, info


def train(args, model_path=None, dataloader=None, model=None, diffusion=None):
    """Drop-in for modules/ddpm_utils.py:483-518: returns the list of per-epoch mean losses; saves a
    preview grid and the state_dict every epoch."""
    from tqdm import tqdm
    setup_logging(args.run_name)
    device = args.device
    ema_beta = getattr(args, "ema_beta", None)
    ema = ema_model = None
    if ema_beta is not None:              # (the reference's conditional recipe: EMA(0.995), ema_model = deepcopy(model))
        import copy
        ema, ema_model = EMA(ema_beta), copy.deepcopy(model)
    n_batches = len(dataloader)
    kind, warmup = getattr(args, "lr_schedule", None), getattr(args, "lr_warmup", 0) or 0
    schedule = None
    if kind is not None or warmup:
        schedule = LRSchedule(kind or "constant", warmup=warmup, total=args.epochs * n_batches,
                              min_ratio=getattr(args, "lr_min_ratio", 0.0) or 0.0)
    t_sampler = getattr(args, "t_sampler", None)
    if isinstance(t_sampler, str) and t_sampler in T_SAMPLERS:
        hist, up = getattr(args, "t_sampler_history", None), getattr(args, "t_sampler_uniform_prob", None)
        t_sampler = LossSecondMomentSampler(diffusion, history_per_term=10 if hist is None else hist,
                                            uniform_prob=0.001 if up is None else up)
    step = TrainStep(model, diffusion, lr=args.lr, graph=False, ema=ema, ema_model=ema_model, t_sampler=t_sampler,
                     ema_start=getattr(args, "ema_start", 2000), max_grad_norm=getattr(args, "max_grad_norm", None),
                     lr_schedule=schedule, loss_weighting=getattr(args, "loss_weighting", None),
                     snr_gamma=5.0 if getattr(args, "snr_gamma", None) is None else args.snr_gamma,
                     vlb_lambda=0.001 if getattr(args, "vlb_lambda", None) is None else args.vlb_lambda)
    loss_all = []
    for epoch in range(args.epochs):
        logging.info(f"Starting epoch {epoch}:")
        pbar = tqdm(dataloader)
        epoch_loss = torch.zeros((), device=device)
        for i, (images, _) in enumerate(pbar):
            loss = step(images.to(device))
            epoch_loss += loss
            if i % 50 == 0:
                pbar.set_postfix(MSE=loss.item())
        loss_all.append(epoch_loss.item() / n_batches)
        previews = [(model, f"{epoch}.jpg")] + ([(ema_model, f"{epoch}_ema.jpg")] if ema is not None else [])
        for net, fname in previews:
            sampled, _ = diffusion.sample(net, n=args.image_gen_n, image_channels=args.image_channels)
            try:
                from .imageio_utils import save_images
                save_images(sampled, os.path.join("results", args.run_name, fname))
            except Exception as e:                                 # preview only; never fail a run on I/O
                logging.warning(f"preview not saved: {e}")
        if model_path:
            torch.save(model.state_dict(), model_path)
            if ema is not None:
                torch.save(ema_model.state_dict(), ema_path(model_path))
            if step.t_sampler is not None:
                torch.save(step.t_sampler.state_dict(), t_sampler_path(model_path))
    return loss_all


def ema_path(model_path):
    """Where `train` writes the EMA weights beside a checkpoint: ckpt_X.pt -> ckpt_X_ema.pt."""
    root, ext = os.path.splitext(model_path)
    return f"{root}_ema{ext}"


def t_sampler_path(model_path):
    """Where `train` writes the timestep sampler's state beside a checkpoint: ckpt_X.pt -> ckpt_X_tsampler.pt."""
    root, ext = os.path.splitext(model_path)
    return f"{root}_tsampler{ext}"
