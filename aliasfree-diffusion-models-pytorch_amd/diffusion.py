"""F12-F17: the DDPM process (modules/ddpm_models.py:301-436) over the HIP kernels.

Bit-exactness: the schedule tables are built on the host with the reference's own torch calls (fp32
linspace; torch.cumprod, which on the CPU accumulates fp32 inputs in double -- DESIGN.md section 4); `sample_timesteps` draws from torch's CPU generator exactly like
the reference; noise_images / the denoise update / the uint8 quantisation are bit-exact HIP
restatements (csrc/sampler.hip).  The sampling loop stays on the device: no per-step H2D copy of `t`
(the reference does one per step, :362) and no per-step host sync.
"""
import contextlib
import logging
import math

import numpy as np
import torch
import torch.distributed as dist

from . import ops, unipc
from .analytic import AnalyticVariance
from .filters import circularLowpassKernel


def shard_range(n, rank, world):
    """Contiguous shard [lo, hi) of n items for `rank` of `world` (sizes differ by at most one; empty when n < world)."""
    return n * rank // world, n * (rank + 1) // world


def gather_u8(t, counts, group=None, dst=0):
    """Collect every rank's (k_r, ...) uint8 tensor on rank `dst`, concatenated in rank order; `counts[r]` = k_r (known to
    every rank: shard sizes are a function of n and the world size).  Shards are padded to the largest so one all_gather
    does it; with 'gloo' the bytes are staged through host memory.  Returns the tensor on `dst`, None elsewhere."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    via_host = dist.get_backend(group) == "gloo"
    kmax = max(max(counts), 1)
    pad = torch.zeros((kmax,) + tuple(t.shape[1:]), dtype=torch.uint8, device="cpu" if via_host else t.device)
    if t.shape[0]:
        pad[:t.shape[0]].copy_(t)
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad, group=group)
    if rank != dst:
        return None
    return torch.cat([parts[r][:counts[r]] for r in range(world)]).to(t.device)


class Diffusion:
    SCHEDULES = ("linear", "cosine")
    PREDICTIONS = ("eps", "v", "x0")
    LOSS_WEIGHTINGS = ("min_snr", "truncated_snr")
    VARIANCES = ("fixed", "learned")

    def __init__(self, noise_steps=1000, beta_start=1e-4, beta_end=0.02, img_size=256, device="cuda", schedule="linear",
                 cosine_s=0.008, prediction="eps", variance="fixed"):
        """schedule: "linear" (the reference's beta schedule) or "cosine" (Nichol & Dhariwal 2021, offset cosine_s).
        prediction: what the network's output means -- "eps", "v" = sqrt(a_t) eps - sqrt(1 - a_t) x0 (Salimans & Ho 2022) or "x0".
        Every sampler and evaluation turns the output into eps with `predict_eps`; `TrainStep` trains towards `training_target`.
        variance: "fixed" (beta_t, the reference's) or "learned" (Nichol & Dhariwal 2021): the network is UNet(c_in=C, c_out=2 C),
        its first C output channels are the prediction and the next C the coefficient v of
        log sigma^2 = ((v + 1) / 2) log beta_t + (1 - (v + 1) / 2) log beta~_t per pixel (`lvar_coefficients`).  The DDPM chain
        (`sample`, `revert`, `sample_sharded`, `ilvr`, guided or not, eager or graph=True) then draws with that variance,
        `calc_bpd(sigma="learned")` scores it and `TrainStep` trains it with the hybrid loss.  Everything that goes through
        `predict_eps` -- DDIM (also under `ilvr`), DPM-Solver++(2M), `inpaint`, `invert`, `decode`, `sdedit`, `interpolate`,
        `equivariance`, the sweeps, `sample_shift` and `sample_concurrent` --
        reads the prediction half alone and keeps its own variance."""
        if not isinstance(variance, str) or variance not in self.VARIANCES:
            raise ValueError(f"Diffusion: unknown variance {variance!r} ('fixed' or 'learned')")
        if not isinstance(schedule, str) or schedule not in self.SCHEDULES:
            raise ValueError(f"Diffusion: unknown schedule {schedule!r} ('linear' or 'cosine')")
        if not isinstance(prediction, str) or prediction not in self.PREDICTIONS:
            raise ValueError(f"Diffusion: unknown prediction {prediction!r} ('eps', 'v' or 'x0')")
        if schedule == "cosine" and not (isinstance(cosine_s, (int, float)) and not isinstance(cosine_s, bool)
                                         and math.isfinite(cosine_s) and cosine_s >= 0):
            raise ValueError(f"Diffusion: cosine_s must be a finite number >= 0 (got {cosine_s!r})")
        self.noise_steps, self.beta_start, self.beta_end = noise_steps, beta_start, beta_end
        self.img_size, self.device = img_size, device
        self.schedule, self.cosine_s, self.prediction = schedule, float(cosine_s), prediction
        self.variance = variance
        self._lv_dev = None
        beta = self.prepare_noise_schedule()                    # host fp32
        alpha = 1.0 - beta
        alpha_hat = torch.cumprod(alpha, dim=0)                 # host ATen cumprod, as the reference (:309): accumulates in double, rounds to fp32
        self.beta, self.alpha, self.alpha_hat = beta.to(device), alpha.to(device), alpha_hat.to(device)
        self.filter = None
        self._t_cache = {}

    def prepare_noise_schedule(self):
        if self.schedule == "cosine":
            # f(u) = cos^2(((u / T + s) / (1 + s)) pi / 2) in fp64; beta_t = min(1 - f(t + 1) / f(t), 0.999), rounded once to fp32
            T, s = self.noise_steps, self.cosine_s
            f = [math.cos(((u / T + s) / (1.0 + s)) * (math.pi / 2.0)) ** 2 for u in range(T + 1)]       # (libm's cos)
            return torch.tensor([min(1.0 - f[t + 1] / f[t], 0.999) for t in range(T)], dtype=torch.float64).float()
        return torch.linspace(self.beta_start, self.beta_end, self.noise_steps)

    # Parametrisations and loss weights -----------------------------------------------------------------------------------
    def _sqrt_tables(self, t, like):
        """sqrt(a_t), sqrt(1 - a_t) of the rows t, shaped to broadcast over `like` (B, ...), in like's dtype on like's device:
        from the fp32 alpha_hat widened first, so in fp64 they are the exact table's roots."""
        ah = self.alpha_hat.to(device=like.device, dtype=like.dtype)[t.to(like.device)]
        ah = ah.reshape((-1,) + (1,) * (like.dim() - 1))
        return torch.sqrt(ah), torch.sqrt(1.0 - ah)

    def training_target(self, x0, eps, t):
        """What the network is trained towards for `self.prediction`, in plain torch ops on the inputs' device and in their
        dtype: eps, sqrt(a_t) eps - sqrt(1 - a_t) x0 ("v") or x0.  t: (B,) integer timesteps."""
        if self.prediction == "eps":
            return eps
        if self.prediction == "x0":
            return x0
        sa, sb = self._sqrt_tables(t, x0)
        return sa * eps - sb * x0

    # Learned reverse-process variances (Nichol & Dhariwal 2021) ------------------------------------------------------------------
    def lvar_coefficients(self):
        """(T, 3) fp64 host table [lb_t, lbt_t, k_t] of the learned variance, from the fp32 schedule tables widened to fp64; row 0
        is zeros.  For 1 <= t < T: lb_t = log(beta[t]); lbt_t = log(beta~_t), beta~_t = (1 - ah[t-1]) / (1 - ah[t]) * beta[t]
        (positive for every t >= 1 under this indexing, so nothing is clipped; lbt_t < lb_t); k_t = beta[t]^2 / (alpha[t] (1 - ah[t])),
        the KL term's weight of (eps_hat - eps)^2 exp(-logvar)."""
        T = self.noise_steps
        if T < 2:
            raise ValueError(f"Diffusion.lvar_coefficients: needs noise_steps >= 2 (got {T})")
        b = self.beta.detach().cpu().double().numpy()
        a = self.alpha.detach().cpu().double().numpy()
        om = 1.0 - self.alpha_hat.detach().cpu().double().numpy()
        tab = np.zeros((T, 3), dtype=np.float64)
        for t in range(1, T):
            tab[t, 0] = math.log(b[t])
            tab[t, 1] = math.log(om[t - 1] / om[t] * b[t])
            tab[t, 2] = b[t] * b[t] / (a[t] * om[t])
        return torch.from_numpy(tab)

    def _lv(self):
        """`lvar_coefficients` on the device, built once."""
        if self._lv_dev is None:
            self._lv_dev = self.lvar_coefficients().to(self.device).contiguous()
        return self._lv_dev

    def output_channels(self, image_channels):
        """The channels the network must emit for C = image_channels: C, or 2 C with variance="learned"."""
        return 2 * image_channels if self.variance == "learned" else image_channels

    def check_model(self, model, image_channels=None, where="Diffusion"):
        """ValueError when the model's output layer (`model.outc`) does not emit `output_channels` channels.  image_channels
        defaults to the model's input channels; a model without `outc` / `inc` is checked on its first output instead."""
        co = getattr(getattr(model, "outc", None), "out_channels", None)
        C = image_channels
        if C is None and hasattr(model, "inc"):
            C = next((p.shape[1] for p in model.inc.parameters() if p.dim() == 4), None)
        if co is None or C is None:
            return
        self._check_out_channels(co, C, where)

    def _check_out_channels(self, got, C, where):
        want = self.output_channels(C)
        if got != want:
            raise ValueError(f"{where}: the model emits {got} channels but variance={self.variance!r} on {C}-channel images needs "
                             f"{want}" + (f" (build UNet(c_in={C}, c_out={2 * C}): the prediction and the variance coefficient)"
                                          if self.variance == "learned" else f" (build UNet(c_in={C}, c_out={C}), or "
                                          f"Diffusion(variance='learned') for a {2 * C}-channel output)"))

    def _raw_output(self, model, x_t, t, y=None):
        """The network's contiguous output at x_t, its channel count checked against `output_channels`."""
        out = model(x_t, t) if y is None else model(x_t, t, y)
        self._check_out_channels(out.shape[1], x_t.shape[1], "Diffusion")
        return out.contiguous()

    def predict_eps(self, model, x_t, t, y=None):
        """Run the model and return eps.  prediction="eps": exactly model(x_t, t[, y]), the same tensor, no launch.  "v" / "x0":
        one fused conversion launch (ops.pred_to_eps), in place on the model's output; t is the per-row int64 device tensor
        the model got, so the conversion captures into the sampling graphs with no host value in it.
        variance="learned": the contiguous eps of the output's prediction half, one launch (ops.split_pred); the coefficient
        half is not read, so whatever calls this keeps its own, fixed variance."""
        if self.variance == "learned":
            return ops.split_pred(self._raw_output(model, x_t, t, y), x_t.contiguous(), t, self.alpha_hat, self.prediction)
        out = model(x_t, t) if y is None else model(x_t, t, y)
        if out.shape[1] != x_t.shape[1]:
            self._check_out_channels(out.shape[1], x_t.shape[1], "Diffusion")
        if self.prediction == "eps":
            return out
        out = out.contiguous()
        return ops.pred_to_eps(out, x_t.contiguous(), t, self.alpha_hat, self.prediction, eps_out=out)

    def snr_weights(self, kind="min_snr", gamma=5.0):
        """(T,) fp64 host table of the loss weight of each timestep for `self.prediction`, with snr_t = a_t / (1 - a_t) from the fp32
        alpha_hat widened to fp64 and c_t the clipped snr:
          "min_snr" (Min-SNR-gamma, Hang et al. 2023): c = min(snr, gamma);
          "truncated_snr" (Salimans & Ho 2022, the weight progressive distillation trains with): c = max(snr, 1); gamma is ignored.
        The weight is c / snr for "eps", c for "x0" and c / (snr + 1) for "v": c on the x0 error in every parametrisation."""
        if not isinstance(kind, str) or kind not in self.LOSS_WEIGHTINGS:
            raise ValueError(f"Diffusion.snr_weights: unknown kind {kind!r} ('min_snr' or 'truncated_snr')")
        a = self.alpha_hat.detach().cpu().double()
        snr = a / (1.0 - a)
        if kind == "truncated_snr":
            clipped = torch.clamp(snr, min=1.0)
        else:
            if isinstance(gamma, bool) or not isinstance(gamma, (int, float, np.integer, np.floating)) or not gamma > 0 \
                    or not math.isfinite(gamma):
                raise ValueError(f"Diffusion.snr_weights: gamma must be a finite number > 0 (got {gamma!r})")
            clipped = torch.clamp(snr, max=float(gamma))
        if self.prediction == "eps":
            return clipped / snr
        if self.prediction == "x0":
            return clipped
        return clipped / (snr + 1.0)

    # Progressive distillation (Salimans & Ho 2022) ---------------------------------------------------------------------------------
    def distill_levels(self, chain):
        """The per-step timestep tables of one distillation round.  chain: the teacher's DDIM timesteps, an explicit strictly
        decreasing sequence of ints in [1, T - 1] of EVEN length 2N (validated as `sample(steps=chain)` validates it).  With the
        levels L = chain + [0], student step k goes L[2k] -> L[2k + 2] and the teacher covers it through L[2k + 1]:
        -> (t, t_mid, t_prev), three (N,) int64 host tensors.  ValueError also when alpha_hat does not strictly decrease along the
        levels (the target's denominator sqrt(a'') - (sigma'' / sigma) sqrt(a) would not be positive)."""
        if isinstance(chain, (int, np.integer)):
            raise ValueError("Diffusion.distill_levels: chain must be an explicit sequence of timesteps (e.g. ddim_timesteps(S))")
        levels = [t for t, _ in self._ddim_pairs(chain, 0.0)] + [0]
        if len(levels) % 2 != 1:
            raise ValueError(f"Diffusion.distill_levels: the teacher's chain must have an even number of steps, two per student "
                             f"step (got {len(levels) - 1})")
        a = self.alpha_hat.detach().cpu().double()[levels].tolist()      # (level 0 is alpha_hat[0], as the DDIM step reads it)
        if any(lo >= hi for lo, hi in zip(a, a[1:])):
            raise ValueError("Diffusion.distill_levels: alpha_hat must strictly decrease with t along the chain's levels")
        as_t = lambda v: torch.tensor(v, dtype=torch.long)
        return as_t(levels[0:-1:2]), as_t(levels[1::2]), as_t(levels[2::2])

    @staticmethod
    def halve_chain(chain):
        """The student's chain of a teacher's: every second timestep, chain[0::2] (it keeps the first, T - 1 for `ddim_timesteps`)."""
        return list(chain)[0::2]

    @staticmethod
    def sample_distill_steps(n, N):
        """(n,) student step indices in [0, N), from the CPU global generator like `sample_timesteps`."""
        return torch.randint(0, N, (n,))

    def distill_targets(self, teacher, x0, k, chain, eps=None, y=None):
        """-> (x_tilde, eps_tilde, t): the distillation target of each row of x0 (B, C, H, W on the device) at student step k[b]
        of the teacher's `chain` (`distill_levels`).  z_t = noise_images(x0, t, eps), then two deterministic DDIM steps of the
        frozen teacher at the row's own timesteps, t -> t_mid -> t_prev, folded into the pair (x_tilde, eps_tilde) whose single
        DDIM step from z_t lands on the teacher's z_prev (ops.distill_mid, ops.distill_target: afd.h has the expressions).  Two
        forwards and three elementwise launches, under no_grad, the teacher hinted and in eval mode; its mode is put back also
        after an exception.  TrainStep(x_tilde, t, eps_tilde) re-forms z_t and trains towards training_target(x_tilde, eps_tilde, t).
        k: (B,) integer tensor (host or device) or a (t, t_mid, t_prev) tuple of (B,) int64 device tensors already gathered
        (DistillStep).  eps: injected noise, default the device generator's; y: class labels handed to both forwards."""
        if self.variance == "learned":
            raise ValueError("Diffusion.distill_targets: variance='learned' is not supported (the student's step is deterministic "
                             "DDIM; distilling a learned variance is out of scope)")
        if isinstance(k, tuple):
            t, t_mid, t_prev = k
        else:
            tabs = self.distill_levels(chain)
            k = torch.as_tensor(k)
            if k.dtype.is_floating_point or k.dtype == torch.bool or tuple(k.shape) != (x0.shape[0],):
                raise ValueError(f"Diffusion.distill_targets: k must hold {x0.shape[0]} integer step indices, one per row")
            kh = k.cpu().long()
            if int(kh.min()) < 0 or int(kh.max()) >= tabs[0].numel():
                raise ValueError(f"Diffusion.distill_targets: every step index must lie in [0, {tabs[0].numel()}) (got {kh.tolist()})")
            t, t_mid, t_prev = (tab[kh].to(x0.device).contiguous() for tab in tabs)
        with self._model_scope(teacher, leave_training=False):
            x0 = x0.contiguous()
            z_t, _ = self.noise_images(x0, t, eps)
            out1 = self._raw_output(teacher, z_t, t, y)
            z_mid = ops.distill_mid(out1, z_t, t, t_mid, self.alpha_hat, self.prediction)
            out2 = self._raw_output(teacher, z_mid, t_mid, y)
            x_tilde, eps_tilde = ops.distill_target(out2, z_mid, z_t, t, t_mid, t_prev, self.alpha_hat, self.prediction)
        return x_tilde, eps_tilde, t

    # Consistency distillation (Song et al. 2023; Luo et al. 2023) --------------------------------------------------------------------
    def consistency_coefficients(self, sigma_data=0.5, timestep_scaling=10.0):
        """(T, 2) fp64 host table [c_skip, c_out] of the consistency parametrisation (LCM's form), with sd = sigma_data and
        s = timestep_scaling:  c_skip[t] = sd^2 / ((s t)^2 + sd^2),  c_out[t] = s t / sqrt((s t)^2 + sd^2).  Row 0 is exactly
        (1, 0), the boundary condition: the consistency function f(z, t) = c_skip[t] z + c_out[t] x_hat(z, t) is the identity at
        t = 0, whatever the model.  c_skip strictly decreases and c_out strictly increases with t."""
        for name, v in (("sigma_data", sigma_data), ("timestep_scaling", timestep_scaling)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not v > 0:
                raise ValueError(f"Diffusion.consistency_coefficients: {name} must be a finite number > 0 (got {v!r})")
        sd2 = float(sigma_data) ** 2
        st = float(timestep_scaling) * torch.arange(self.noise_steps, dtype=torch.float64)
        d = st * st + sd2
        return torch.stack([sd2 / d, st / torch.sqrt(d)], dim=1).contiguous()

    def _cm(self, sigma_data=0.5, timestep_scaling=10.0):
        """`consistency_coefficients` on the device, built once per (sigma_data, timestep_scaling)."""
        cache = self.__dict__.setdefault("_cm_dev", {})
        key = (float(sigma_data), float(timestep_scaling))
        if key not in cache:
            cache[key] = self.consistency_coefficients(sigma_data, timestep_scaling).to(self.device).contiguous()
        return cache[key]

    def consistency_levels(self, chain):
        """The per-position timestep tables of a consistency distillation over the teacher's DDIM `chain` (an explicit strictly
        decreasing sequence of ints in [1, T - 1], any length N >= 1, validated as `sample(steps=chain)` validates it).  With the
        levels L = chain + [0], position k is the teacher's step L[k] -> L[k + 1]: -> (t, t_prev), two (N,) int64 host tensors.
        ValueError also when alpha_hat does not strictly decrease along the levels."""
        if isinstance(chain, (int, np.integer)):
            raise ValueError("Diffusion.consistency_levels: chain must be an explicit sequence of timesteps (e.g. ddim_timesteps(S))")
        levels = [t for t, _ in self._ddim_pairs(chain, 0.0)] + [0]
        a = self.alpha_hat.detach().cpu().double()[levels].tolist()      # (level 0 is alpha_hat[0], as the DDIM step reads it)
        if any(lo >= hi for lo, hi in zip(a, a[1:])):
            raise ValueError("Diffusion.consistency_levels: alpha_hat must strictly decrease with t along the chain's levels")
        as_t = lambda v: torch.tensor(v, dtype=torch.long)
        return as_t(levels[:-1]), as_t(levels[1:])

    def consistency_targets(self, teacher, target_model, x0, k, chain, coef, eps=None, y=None):
        """-> (x_tilde, eps_tilde, t): the consistency-distillation target of each row of x0 (B, C, H, W on the device) at position
        k[b] of the teacher's `chain` (`consistency_levels`).  z_t = noise_images(x0, t, eps); one deterministic DDIM step of the
        frozen teacher, t -> t_prev (ops.distill_mid); one forward of the target network at (z_prev, t_prev); then
        ops.consistency_target: the x0 (and the eps re-forming z_t with it) that a student must predict at (z_t, t) for its
        consistency function to equal the target network's at (z_prev, t_prev) (afd.h has the expressions).  Two forwards and three
        elementwise launches, under no_grad, both models hinted and in eval mode; their modes are put back also after an exception.
        TrainStep(x_tilde, t, eps_tilde) re-forms z_t and trains towards training_target(x_tilde, eps_tilde, t).
        k: (B,) integer tensor (host or device) or a (t, t_prev) tuple of (B,) int64 device tensors already gathered
        (ConsistencyStep).  coef: the (T, 2) fp64 device table (`consistency_coefficients` on the device).  eps: injected noise,
        default the device generator's; y: class labels handed to both forwards."""
        if self.variance == "learned":
            raise ValueError("Diffusion.consistency_targets: variance='learned' is not supported (the consistency function is "
                             "deterministic; distilling a learned variance is out of scope)")
        if isinstance(k, tuple):
            t, t_prev = k
        else:
            tabs = self.consistency_levels(chain)
            k = torch.as_tensor(k)
            if k.dtype.is_floating_point or k.dtype == torch.bool or tuple(k.shape) != (x0.shape[0],):
                raise ValueError(f"Diffusion.consistency_targets: k must hold {x0.shape[0]} integer positions, one per row")
            kh = k.cpu().long()
            if int(kh.min()) < 0 or int(kh.max()) >= tabs[0].numel():
                raise ValueError(f"Diffusion.consistency_targets: every position must lie in [0, {tabs[0].numel()}) (got {kh.tolist()})")
            t, t_prev = (tab[kh].to(x0.device).contiguous() for tab in tabs)
        with self._model_scope(teacher, leave_training=False), self._model_scope(target_model, leave_training=False):
            x0 = x0.contiguous()
            z_t, _ = self.noise_images(x0, t, eps)
            out = self._raw_output(teacher, z_t, t, y)
            z_prev = ops.distill_mid(out, z_t, t, t_prev, self.alpha_hat, self.prediction)
            out_tgt = self._raw_output(target_model, z_prev, t_prev, y)
            x_tilde, eps_tilde = ops.consistency_target(out_tgt, z_prev, z_t, t, t_prev, self.alpha_hat, coef, self.prediction)
        return x_tilde, eps_tilde, t

    def consistency_sample(self, model, n, image_channels, steps, noise_source="reference", graph=None, labels=None,
                           return_float=False, sigma_data=0.5, timestep_scaling=10.0):
        """Few-step sampling of a consistency model (`ConsistencyStep`, `consistency_distill`): multistep consistency sampling.
        steps: an int S (the timesteps `ddim_timesteps(S)`) or an explicit strictly decreasing sequence of timesteps in
        [1, T - 1]; [T - 1] alone is one-step generation.  x starts as the initial noise at steps[0]; every step runs ONE forward
        at (x, t) and one fused launch (ops.consistency_step): x <- f(x, t) noised again to the next timestep with fresh noise
        (`_step_noise`), and x <- f(x, t) itself at the last step.  More steps trade time for quality with no retraining.
        sigma_data / timestep_scaling: those the model was distilled with (`consistency_coefficients`).  noise_source, labels,
        return_float and the snapshots are `sample`'s for DDIM; graph=True captures one step (forward, device noise, the update
        with t and the next timestep read on the device) and replays it for every step but the last, as the DDIM loop does.
        Guidance is not offered."""
        logging.info(f"Sampling {n} new images....")
        if self.variance == "learned":
            raise ValueError("Diffusion.consistency_sample: variance='learned' is not supported")
        pairs = self._ddim_pairs(steps, 0.0)
        self.consistency_coefficients(sigma_data, timestep_scaling)                      # (argument errors before device work)
        if labels is not None:
            labels = self._check_labels(model, n, None, labels, "consistency_sample")
        coef = self._cm(sigma_data, timestep_scaling)
        self.check_model(model, image_channels, "Diffusion.consistency_sample")
        kind, ah = self.prediction, self.alpha_hat
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, noise_source)

            def step(t_rows, t, tn, draw):
                out = self._raw_output(model, x, t_rows, labels)
                if isinstance(t, torch.Tensor):
                    ops.consistency_step_dev(out, x, draw(), ah, coef, kind, t, tn, x)
                else:
                    ops.consistency_step(out, x, draw() if draw else None, ah, coef, kind, t, tn, x_out=x)

            replay = None
            if graph and noise_source != "cpu" and len(pairs) > 1:
                t_dev = torch.full((n,), pairs[0][0], device=x.device, dtype=torch.long)
                tn_dev = torch.full((1,), pairs[0][1], device=x.device, dtype=torch.long)
                g = self._capture(lambda: step(t_dev, t_dev, tn_dev, lambda: torch.randn_like(x)), x)

                def replay(t, tn):
                    t_dev.fill_(t)
                    tn_dev.fill_(tn)
                    g.replay()
            for t, tn in pairs:
                if replay is not None and tn > 0:
                    replay(t, tn)
                else:
                    step(self._t_full(n, t, x.device), t, tn, (lambda: self._step_noise(x, noise_source)) if tn > 0 else None)
                if self.ddim_snapshot(t, tn):
                    snaps.append(x.clone())
            x = x.clone()
        snaps.append(x)
        return self._finish(x, snaps, return_float)

    # F14 ---------------------------------------------------------------------------------
    def noise_images(self, x, t, eps=None):
        """-> (x_t, eps).  `eps` may be injected (parity mode); default = device RNG like the reference."""
        if eps is None:
            eps = torch.randn_like(x)
        return ops.noise_images(x, eps, t.to(x.device), self.alpha_hat), eps

    # F13 ---------------------------------------------------------------------------------
    def sample_timesteps(self, n):
        return torch.randint(low=1, high=self.noise_steps, size=(n,))     # CPU global generator, t in [1, T-1]

    # F16 ---------------------------------------------------------------------------------
    def _t_full(self, n, i, device):
        """Device tensor full((n,), i): built once per (n, stream) as arange and sliced -- no per-step H2D.
        Keyed by the current HIP stream as well: the table is filled by kernels on the stream that first asks, so a
        trajectory of `sample_concurrent` on another stream builds (and later frees) its own copy instead of reading one
        whose fill it is not ordered behind."""
        key = (n, str(device), ops._stream())
        tab = self._t_cache.get(key)
        if tab is None:
            tab = torch.arange(self.noise_steps, device=device, dtype=torch.long)[:, None].repeat(1, n).contiguous()
            if len(self._t_cache) >= 16:
                self._t_cache.pop(next(iter(self._t_cache)))
            self._t_cache[key] = tab
        return tab[i]

    def _initial_noise(self, n, c, noise_source, shard=None):
        """shard = (lo, hi): draw the noise of all n images (every rank consumes the identical generator stream) and keep
        rows lo:hi -- a sharded run then produces exactly the images of the one-rank run."""
        shape = (n, c, self.img_size, self.img_size)
        if noise_source == "device":
            x = torch.randn(shape, device=self.device)
        else:
            x = torch.randn(shape).to(self.device)                         # reference: CPU draw, then copy (:360)
        return x if shard is None else x[shard[0]:shard[1]].contiguous()

    def _step_noise(self, x, noise_source, shard=None, n=None):
        shape = x.shape if shard is None else (n,) + tuple(x.shape[1:])
        if noise_source == "cpu":      # parity mode: replay the reference's CPU-path stream
            z = torch.randn(shape).to(x.device)
        else:
            z = torch.randn(shape, device=x.device)
        return z if shard is None else z[shard[0]:shard[1]].contiguous()

    def _chunk_noise(self, shape, noise_source, noise_fn=None):
        """The fp32 noise of one chunk of rows of `calc_bpd` / `equivariance`, on the device: noise_fn(shape) when given, else
        drawn from the device generator (noise_source "device") or from the CPU generator and copied ("cpu")."""
        if noise_fn is not None:
            eps = noise_fn(shape)
        elif noise_source == "device":
            eps = torch.randn(shape, device=self.device)
        else:
            eps = torch.randn(shape).to(self.device)
        return eps.to(device=self.device, dtype=torch.float32).contiguous()

    def _loop(self, model, n, image_channels, theta=None, noise_source="reference", graph=None, shard=None, labels=None,
              cfg_scale=0.0):
        """Shared body of sample / revert.  noise_source: 'reference' (x_T from the CPU generator,
        per-step noise from the device generator -- what the reference does on a GPU), 'cpu'
        (everything from the CPU generator: reproduces the reference's CPU run), 'device'.
        graph: capture ONE denoise step (UNet forward + device noise + update) into a hipGraph and replay
        it for i = T-1 .. 2 (the step index lives in device memory).  Off by default: measured on MI355X the
        loop is bound by the ~330 dependent kernel boundaries per step on the device (2.18 ms/step at n=6
        with or without replay), not by host launches.
        labels: (n,) int64 device tensor (checked by `sample`) or None.  With labels and cfg_scale > 0 (classifier-free
        guidance) every step runs ONE forward over 2n rows [x ; x] with labels [labels ; NULL_LABEL] and the fused guided
        update writes both halves of that 2n-row state in place; the noise drawn is that of n images, as without labels.
        The state lives in xs (n rows, or those 2n) and one local `step` serves the eager iterations and the capture."""
        theta_step = None if theta is None else theta / self.noise_steps
        self.check_model(model, image_channels, "Diffusion.sample")
        learned = self.variance == "learned"
        forward = self._raw_output if learned else self.predict_eps      # learned: the raw 2C output goes to the update
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, noise_source, shard)
            n_all, n = n, x.shape[0]
            y, s = self._guided(labels, cfg_scale)
            xs = torch.cat([x, x]) if s > 0 else x
            rows = xs.shape[0]

            def step(t_rows, t, draw):
                out = forward(model, xs, t_rows, y)
                self._update(xs, n, out, draw() if draw else None, t, learned=learned, cfg_scale=s)

            replay = None
            if graph and theta is None and noise_source != "cpu" and shard is None:
                t_dev = torch.full((rows,), self.noise_steps - 1, device=x.device, dtype=torch.long)
                g = self._capture(lambda: step(t_dev, t_dev, lambda: torch.randn_like(xs[:n])), xs)

                def replay(i):
                    t_dev.fill_(i)
                    g.replay()
            for i in reversed(range(1, self.noise_steps)):
                if n == 0:                                   # an empty shard still consumes the shared noise stream
                    if i > 1:
                        self._step_noise(x, noise_source, shard, n_all)
                elif replay is not None and i > 1:           # the last step draws no noise: it runs eagerly
                    replay(i)
                else:
                    step(self._t_full(rows, i, x.device), i,
                         (lambda: self._step_noise(xs[:n], noise_source, shard, n_all)) if i > 1 else None)
                    if theta_step is not None:
                        xs = self.rotate_2d_matrix(xs, theta_step, self.filter)
                if i % 100 == 0:
                    snaps.append(xs[:n].clone())
            x = xs[:n].clone()
        snaps.append(x)
        return x, snaps

    # DDIM (Song et al. 2021) over a strided subsequence of the timesteps -------------------------------------------------
    def ddim_timesteps(self, steps):
        """The S = `steps` timesteps of a DDIM chain, strictly decreasing: tau_k = 1 + (k (T - 2)) // (S - 1) for k = 0 .. S-1,
        in descending order (S = 1: [T - 1]).  S = T - 1 gives T-1 .. 1, the DDPM chain's own indices; the last tau is 1."""
        T = self.noise_steps
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
            raise ValueError(f"Diffusion.ddim_timesteps: steps must be an int (got {type(steps).__name__})")
        S = int(steps)
        if not 1 <= S <= T - 1:
            raise ValueError(f"Diffusion.ddim_timesteps: steps must lie in [1, {T - 1}] (got {S})")
        if S == 1:
            return [T - 1]
        return [1 + (k * (T - 2)) // (S - 1) for k in reversed(range(S))]

    def _ddim_pairs(self, steps, eta, timesteps=None):
        """steps (an int S or an explicit strictly decreasing sequence of ints in [1, T-1]) -> [(t, t_prev)], the last
        t_prev 0.  Raises ValueError for anything else, and for eta < 0.  timesteps: the rule for an int S (default
        `ddim_timesteps`)."""
        eta = float(eta)
        if not eta >= 0:
            raise ValueError(f"Diffusion: DDIM needs eta >= 0 (got {eta})")
        if isinstance(steps, (int, np.integer)) and not isinstance(steps, bool):
            taus = (timesteps or self.ddim_timesteps)(steps)
        else:
            try:
                taus = list(steps)
            except TypeError:
                raise ValueError(f"Diffusion: steps must be an int or a sequence of ints (got {type(steps).__name__})") from None
            T = self.noise_steps
            if not taus or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in taus):
                raise ValueError("Diffusion: an explicit steps sequence must be a non-empty sequence of ints")
            taus = [int(v) for v in taus]
            if any(not 1 <= v <= T - 1 for v in taus):
                raise ValueError(f"Diffusion: every step of an explicit steps sequence must lie in [1, {T - 1}] (got {taus})")
            if any(a <= b for a, b in zip(taus, taus[1:])):
                raise ValueError(f"Diffusion: an explicit steps sequence must be strictly decreasing (got {taus})")
        return list(zip(taus, taus[1:] + [0]))

    @staticmethod
    def ddim_snapshot(t, t_prev):
        """Whether x is kept as a snapshot after the step t -> t_prev: when the step crosses a multiple of 100.  On the
        full chain (t_prev = t - 1) this is the DDPM sampler's i % 100 == 0."""
        return t_prev // 100 < t // 100

    def _ddim_loop(self, model, n, image_channels, pairs, eta, noise_source="reference", graph=None, labels=None, cfg_scale=0.0,
                   analytic=None, start=None):
        """`_loop` over the DDIM steps `pairs` (see `sample`).  x_T is drawn as in `_loop`; with eta > 0 every step but the
        last draws the noise of n images (`_step_noise`), with eta == 0 none is drawn.  graph: capture one step (forward,
        noise, the update with t and t_prev read on the device) and replay it for every step but the last, which runs eagerly.
        start: the (n, C, S, S) state at level pairs[0][0] to start from instead of drawn noise (`decode`); it is not written.
        analytic: an `AnalyticVariance`; the steps then draw with its sigmas (ops.ddim_step_var), whose table is built here, once,
        and stays on the device, and the noise is drawn as for eta > 0 whatever eta is."""
        snaps = []
        sig = None if analytic is None else analytic.sigma_table(self, pairs, eta).to(self.device).contiguous()
        noisy = eta > 0 or sig is not None
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, noise_source) if start is None else start.to(self.device).contiguous().clone()
            y, s = self._guided(labels, cfg_scale)
            xs = torch.cat([x, x]) if s > 0 else x
            rows = xs.shape[0]

            def step(t_rows, t, tp, draw):
                eps = self.predict_eps(model, xs, t_rows, y)
                self._update(xs, n, eps, draw() if draw else None, t, tp, eta=eta, cfg_scale=s, sig=sig)

            replay = None
            if graph and noise_source != "cpu" and len(pairs) > 1:
                t_dev = torch.full((rows,), pairs[0][0], device=x.device, dtype=torch.long)
                tp_dev = torch.full((1,), pairs[0][1], device=x.device, dtype=torch.long)
                g = self._capture(lambda: step(t_dev, t_dev, tp_dev, (lambda: torch.randn_like(xs[:n])) if noisy else None), xs)

                def replay(t, tp):
                    t_dev.fill_(t)
                    tp_dev.fill_(tp)
                    g.replay()
            for t, tp in pairs:
                if replay is not None and tp > 0:
                    replay(t, tp)
                else:
                    step(self._t_full(rows, t, x.device), t, tp,
                         (lambda: self._step_noise(xs[:n], noise_source)) if noisy and tp > 0 else None)
                if self.ddim_snapshot(t, tp):
                    snaps.append(xs[:n].clone())
            x = xs[:n].clone()
        snaps.append(x)
        return x, snaps

    # DPM-Solver++(2M) (Lu et al. 2022): a second-order multistep solver of the probability-flow ODE ------------------------
    def _logsnr(self):
        """lam(t) = log(sqrt(a_t)) - log(sqrt(1 - a_t)) in fp64 for every t, a_t the fp32 alpha_hat[t] (decreasing in t)."""
        a = self.alpha_hat.detach().cpu().double().numpy()
        return np.log(np.sqrt(a)) - np.log(np.sqrt(1.0 - a))

    def logsnr_timesteps(self, steps):
        """The S = `steps` timesteps of a DPM-Solver++ chain, uniform in log-SNR and strictly decreasing from T - 1 to 1.
        r_0 = T - 1, r_{S-1} = 1; for 0 < k < S - 1, r_k is the t in [1, T - 1] whose lam(t) is nearest to
        lam(T-1) + (k / (S-1)) (lam(1) - lam(T-1)), ties to the smaller t.  Then r_k = max(r_k, r_{k+1} + 1) for k = S-2 .. 0,
        and r_k = min(r_k, T - 1 - k).  S = 1: [T - 1]; S = T - 1: T-1 .. 1.  Argument errors as `ddim_timesteps`."""
        T = self.noise_steps
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)):
            raise ValueError(f"Diffusion.logsnr_timesteps: steps must be an int (got {type(steps).__name__})")
        S = int(steps)
        if not 1 <= S <= T - 1:
            raise ValueError(f"Diffusion.logsnr_timesteps: steps must lie in [1, {T - 1}] (got {S})")
        if S == 1:
            return [T - 1]
        lam = self._logsnr()
        k = np.arange(1, S - 1)
        target = lam[T - 1] + (k / (S - 1)) * (lam[1] - lam[T - 1])
        up = -lam[1:T]                                   # increasing; position j is t = j + 1
        hi = np.clip(np.searchsorted(up, -target), 0, T - 2)
        lo = np.clip(hi - 1, 0, T - 2)
        pick = np.where(np.abs(up[hi] + target) < np.abs(up[lo] + target), hi, lo)     # ties: lo, the smaller t
        r = np.concatenate([[T - 1], pick + 1, [1]]).astype(np.int64)
        for i in range(S - 2, -1, -1):
            r[i] = max(r[i], r[i + 1] + 1)
        r = np.minimum(r, T - 1 - np.arange(S))
        return [int(v) for v in r]

    def dpmpp_pairs(self, steps):
        """steps (an int S, spaced by `logsnr_timesteps`, or an explicit strictly decreasing sequence validated as for DDIM)
        -> [(t, t_prev)], the last t_prev 0."""
        return self._ddim_pairs(steps, 0.0, self.logsnr_timesteps)

    @staticmethod
    def dpmpp_order(k, S):
        """The order of step k of an S-step DPM-Solver++(2M) chain: 1 at k = 0 (no previous x0) and, when S < 15, at the last
        step (diffusers' lower_order_final); 2 otherwise."""
        return 1 if k == 0 or (k == S - 1 and S < 15) else 2

    def dpmpp_coefficients(self, pairs):
        """(S, 5) fp32 host table of the DPM-Solver++(2M) chain `pairs`: row k = [alpha(t), sigma(t), A, B0, B1] of the step
        t -> tp, computed in fp64 and rounded once.  alpha(t) = sqrt(a_t), sigma(t) = sqrt(1 - a_t), h_k = lam(tp) - lam(t),
        A = sigma(tp) / sigma(t), B = -alpha(tp) expm1(-h_k).  First order (B0 = B, B1 = 0) at k = 0 and, when S < 15, at
        k = S - 1; otherwise second order with r = h_{k-1} / h_k: B0 = B (1 + 1 / (2 r)), B1 = -B / (2 r)."""
        ah = self.alpha_hat.detach().cpu().tolist()                      # one copy; Python floats hold the fp32 values exactly
        alpha = lambda t: math.sqrt(ah[t])
        sigma = lambda t: math.sqrt(1.0 - ah[t])
        lam = lambda t: math.log(alpha(t)) - math.log(sigma(t))
        S = len(pairs)
        rows, h_prev = [], None
        for k, (t, tp) in enumerate(pairs):
            h = lam(tp) - lam(t)
            A = sigma(tp) / sigma(t)
            B = -alpha(tp) * math.expm1(-h)
            if self.dpmpp_order(k, S) == 1:
                B0, B1 = B, 0.0
            else:
                r = h_prev / h
                B0, B1 = B * (1.0 + 1.0 / (2.0 * r)), -B / (2.0 * r)
            rows.append([alpha(t), sigma(t), A, B0, B1])
            h_prev = h
        return torch.tensor(np.array(rows, dtype=np.float64).astype(np.float32))

    def _dpmpp_loop(self, model, n, image_channels, pairs, noise_source="reference", graph=None, labels=None, cfg_scale=0.0):
        """`_loop` over the DPM-Solver++(2M) steps `pairs`: x_T drawn as in `_loop`, no noise after it, one forward per step
        (2n rows when guided).  The x0 of the previous step is the solver's state, updated in place by the kernel.  graph:
        capture one step (forward and update, reading the step's coefficients from a static device buffer) and replay it for
        every step but the last, which runs eagerly."""
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, noise_source)
            table = self.dpmpp_coefficients(pairs).to(x.device)          # once per trajectory
            y, s = self._guided(labels, cfg_scale)
            xs = torch.cat([x, x]) if s > 0 else x
            rows = xs.shape[0]
            x0 = torch.zeros_like(x)                                      # the solver state: the previous step's x0

            def step(t_rows, coef, prev):
                eps = self.predict_eps(model, xs, t_rows, y)
                if s > 0:
                    ops.dpmpp_step_cfg(xs[:n], eps, prev, coef, s, xs[:n], xs[n:], x0)
                else:
                    ops.dpmpp_step(xs, eps, prev, coef, xs, x0)           # in place (elementwise)

            replay = None
            if graph and len(pairs) > 1:
                t_dev = torch.full((rows,), pairs[0][0], device=x.device, dtype=torch.long)
                coef = table[0].clone()
                # the captured step always reads x0: it starts at zero, so the first-order first step (B1 = 0) adds B1 * 0 = +0
                g = self._capture(lambda: step(t_dev, coef, x0), xs)
                x0.zero_()                                                # undo the warm-up's state as well

                def replay(k):
                    t_dev.fill_(pairs[k][0])
                    coef.copy_(table[k])
                    g.replay()
            for k, (t, tp) in enumerate(pairs):
                if replay is not None and tp > 0:
                    replay(k)
                else:
                    step(self._t_full(rows, t, x.device), table[k], x0 if self.dpmpp_order(k, len(pairs)) == 2 else None)
                if self.ddim_snapshot(t, tp):
                    snaps.append(xs[:n].clone())
            x = xs[:n].clone()
        snaps.append(x)
        return x, snaps

    # UniPC (Zhao et al. 2023): a multistep predictor-corrector of order up to 3, one forward per step (unipc.py) -------------
    UNIPC_SAMPLERS = {"unipc": 2, "unipc_1": 1, "unipc_2": 2, "unipc_3": 3}

    @staticmethod
    def unipc_order(k, S, P):
        """The order of step k of an S-step UniPC chain of order P: min(P, k + 1) and, when S < 15, also min(., S - k)
        (`dpmpp_order`'s convention; P = 2 gives `dpmpp_order`)."""
        return unipc.unipc_order(k, S, P)

    def unipc_coefficients(self, pairs, order, dtype=torch.float32):
        """(S, 12) host table of the UniPC chain `pairs` at order P = `order` (1 .. 3), computed in fp64 and rounded once to
        `dtype` (torch.float64: the unrounded table).  Row k = [alpha, sigma, Ac, c0, c1, c2, c3, Ap, p0, p1, p2, slot] of
        evaluation k at level lev[k] (lev = taus + [0]; alpha, sigma, lam as in `dpmpp_coefficients`): with
        m_k = (x~_k - sigma e) / alpha,
            x_k      = Ac x_{k-1} + c0 m_k + c1 m_{k-1} + c2 m_{k-2} + c3 m_{k-3}     (the corrector, order[k-1])
            x~_{k+1} = Ap x_k     + p0 m_k + p1 m_{k-1} + p2 m_{k-2}                  (the predictor, order[k])
        the rho / D_i form of unipc.py folded per evaluation: for a move s -> u of width h with B = expm1(-h), A = sigma_u / sigma_s,
        the earlier evaluation i weighs -alpha_u B rho_i / r_i, the corrector's new one -alpha_u B rho_p, and the base takes
        -alpha_u B minus all of those, so each move's weights sum to -alpha_u B.  Row 0: Ac = 1 and c* = 0 (no corrector: the
        corrected state starts as x_T); unused history weights are 0.  slot = k mod 3, the ring position that receives m_k."""
        P = int(order)
        if not 1 <= P <= unipc.MAX_ORDER:
            raise ValueError(f"Diffusion.unipc_coefficients: order must be 1, 2 or 3 (got {order!r})")
        _, alpha, sigma, lam = unipc.schedule_levels(self.alpha_hat, pairs)
        S = len(pairs)

        def weights(s, u, earlier, corrector):
            """-> (A, w_new, w_base, [w_1 ..]) of the move s -> u with the earlier evaluations at the positions `earlier`; w_new
            (the corrector's weight of the new evaluation) is 0 for a predictor."""
            h = lam[u] - lam[s]
            aB = alpha[u] * math.expm1(-h)
            rs = [(lam[q] - lam[s]) / h for q in earlier]
            rho = unipc.unipc_rho(rs, h, corrector)
            w = [-aB * w_i / r for w_i, r in zip(rho, rs)]
            w_new = -aB * rho[-1] if corrector else 0.0
            return sigma[u] / sigma[s], w_new, -aB - sum(w) - w_new, w

        rows = []
        for k in range(S):
            c = [1.0, 0.0, 0.0, 0.0, 0.0]
            if k >= 1:
                p = self.unipc_order(k - 1, S, P)
                A, w_new, w_base, w = weights(k - 1, k, [k - 1 - i for i in range(1, p)], True)
                c = [A, w_new, w_base] + w + [0.0] * (3 - p)
            p = self.unipc_order(k, S, P)
            A, _, w_base, w = weights(k, k + 1, [k - i for i in range(1, p)], False)
            rows.append([alpha[k], sigma[k]] + c + [A, w_base] + w + [0.0] * (3 - p) + [float(k % 3)])
        table = np.array(rows, dtype=np.float64)
        return torch.tensor(table if dtype == torch.float64 else table.astype(np.float32))

    def _unipc_loop(self, model, n, image_channels, pairs, order, noise_source="reference", graph=None, labels=None, cfg_scale=0.0):
        """`_dpmpp_loop` for UniPC of order `order`: x_T drawn as in `_loop`, no noise after it, one forward per step (2n rows
        when guided) and one update launch that corrects the last state with the new evaluation and predicts the next.  The
        solver's state is xc (n rows: the corrected state, starts as x_T) and hist (a ring of the last three m), both updated in
        place by the kernel; xs holds the predicted state the network sees.  graph: capture one step (forward and update,
        reading the step's row from a static device buffer) and replay it for every step but the last, which runs eagerly."""
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, noise_source)
            table = self.unipc_coefficients(pairs, order).to(x.device)   # once per trajectory
            y, s = self._guided(labels, cfg_scale)
            xs = torch.cat([x, x]) if s > 0 else x
            rows = xs.shape[0]
            xc = x.clone()
            hist = torch.zeros((3,) + tuple(x.shape), device=x.device, dtype=x.dtype)

            def step(t_rows, coef):
                eps = self.predict_eps(model, xs, t_rows, y)
                if s > 0:
                    ops.unipc_step_cfg(xs[:n], eps, xc, hist, coef, s, xs[:n], xs[n:])
                else:
                    ops.unipc_step(xs, eps, xc, hist, coef, xs)           # in place (elementwise)

            replay = None
            if graph and len(pairs) > 1:
                t_dev = torch.full((rows,), pairs[0][0], device=x.device, dtype=torch.long)
                coef = table[0].clone()
                g = self._capture(lambda: step(t_dev, coef), xs)
                xc.copy_(xs[:n])                                          # undo the warm-up's state as well (xs is x_T again)
                hist.zero_()

                def replay(k):
                    t_dev.fill_(pairs[k][0])
                    coef.copy_(table[k])
                    g.replay()
            for k, (t, tp) in enumerate(pairs):
                if replay is not None and tp > 0:
                    replay(k)
                else:
                    step(self._t_full(rows, t, x.device), table[k])
                if self.ddim_snapshot(t, tp):
                    snaps.append(xs[:n].clone())
            x = xs[:n].clone()
        snaps.append(x)
        return x, snaps

    def _hint(self, model):
        """Tell the model the range of the timesteps this process will pass (all of them in [0, noise_steps)): lets the
        UNet tabulate its time embeddings once per trajectory (unet.UNet._timestep_tables); cleared again when the loop
        ends (_unhint), so a direct call of the model may pass any t."""
        if hasattr(model, "_t_range"):
            model._t_range = self.noise_steps

    @staticmethod
    def _unhint(model):
        """The loop is over: a later direct call of the model may pass any t again."""
        if hasattr(model, "_t_range"):
            model._t_range = None

    @contextlib.contextmanager
    def _model_scope(self, model, leave_training=True):
        """What every loop over the model runs in: the model hinted (`_hint`) and in eval mode, under no_grad.  On the way out,
        also after an exception: leave_training (the samplers) puts the model in train mode, as the reference leaves it (:379),
        and clears the hint; otherwise (the evaluations) the mode and the hint come back as they were found."""
        found = None if leave_training else (model.training, getattr(model, "_t_range", None))
        self._hint(model)
        try:
            model.eval()
            with torch.no_grad():
                yield
        finally:
            if leave_training:
                model.train()
                self._unhint(model)
            else:
                model.train(found[0])
                if hasattr(model, "_t_range"):
                    model._t_range = found[1]

    @staticmethod
    def _guided(labels, cfg_scale):
        """-> (y, s), built once per trajectory.  Classifier-free guidance (labels and cfg_scale > 0): y = [labels ; NULL_LABEL],
        the labels of the 2n rows [x ; x] of the one forward per step, and s = cfg_scale.  Otherwise y = labels and s = 0."""
        if labels is not None and cfg_scale > 0:
            return torch.cat([labels, torch.full_like(labels, ops.NULL_LABEL)]), cfg_scale
        return labels, 0.0

    def _check_labels(self, model, n, theta, labels, where="sample"):
        if theta is not None:
            raise NotImplementedError(f"Diffusion.{where}: class labels together with a rotation (theta) are not supported")
        if getattr(model, "label_emb", None) is None:
            raise ValueError(f"Diffusion.{where}: labels were passed but the model has no label embedding (build UNet(num_classes=K))")
        y = torch.as_tensor(labels)
        if y.dtype.is_floating_point or y.dtype.is_complex or y.dtype == torch.bool:
            raise ValueError(f"Diffusion.{where}: labels must be integers (got {y.dtype})")
        if tuple(y.shape) != (n,):
            raise ValueError(f"Diffusion.{where}: expected {n} labels, one per image (got shape {tuple(y.shape)})")
        return y.to(device=self.device, dtype=torch.long).contiguous()

    def _check_ddim(self, where, steps, eta, theta=None):
        """-> the DDIM (t, t_prev) pairs, or None for the DDPM chain (steps=None)."""
        if steps is None:
            if eta:
                raise ValueError(f"Diffusion.{where}: eta applies to the DDIM sampler only (pass steps=)")
            return None
        if theta is not None:
            raise NotImplementedError(f"Diffusion.{where}: steps (DDIM) together with a rotation (theta) is not supported")
        return self._ddim_pairs(steps, eta)

    def _check_sampler(self, where, sampler, steps, eta, theta=None):
        """-> (solver, pairs): ("ddim", the `_check_ddim` pairs or None) for sampler None / "ddim", ("dpmpp_2m", the DPM++
        pairs) for "dpmpp_2m", (the name, the same pairs) for a key of `UNIPC_SAMPLERS`."""
        if sampler is None or (isinstance(sampler, str) and sampler == "ddim"):
            return "ddim", self._check_ddim(where, steps, eta, theta)
        if not (isinstance(sampler, str) and (sampler == "dpmpp_2m" or sampler in self.UNIPC_SAMPLERS)):
            raise ValueError(f"Diffusion.{where}: unknown sampler {sampler!r} (None, 'ddim', 'dpmpp_2m', 'unipc', 'unipc_1', "
                             f"'unipc_2' or 'unipc_3')")
        if theta is not None:
            raise NotImplementedError(f"Diffusion.{where}: sampler={sampler!r} together with a rotation (theta) is not supported")
        if steps is None:
            raise ValueError(f"Diffusion.{where}: sampler={sampler!r} needs steps (an int or an explicit sequence of timesteps)")
        if eta != 0:
            raise ValueError(f"Diffusion.{where}: sampler={sampler!r} is deterministic: eta must be 0 (got {eta})")
        return sampler, self.dpmpp_pairs(steps)

    def sample(self, model, n, image_channels, theta=None, noise_source="reference", return_float=False, graph=None,
               labels=None, cfg_scale=0.0, steps=None, eta=0.0, sampler=None):
        """labels: (n,) integer class labels (NULL_LABEL for an unconditional image) for a UNet(num_classes=K); None = the
        unconditional sampler.  cfg_scale > 0: classifier-free guidance, eps = torch.lerp(eps_uncond, eps_cond, cfg_scale),
        both predictions from ONE forward over 2n rows per step; cfg_scale <= 0: the conditional prediction alone.  The noise
        drawn (x_T and every step's) is that of the unconditional sampler for the same seed and noise_source.
        steps: None = the full DDPM chain (T - 1 forwards).  An int S (1 <= S <= T - 1) or an explicit strictly decreasing
        sequence of timesteps in [1, T - 1] selects DDIM over those timesteps (`ddim_timesteps`), S forwards, with
        eta = 0 deterministic (no noise drawn after x_T) and eta = 1 ancestral.  Snapshots are taken after each step that
        crosses a multiple of 100 (`ddim_snapshot`), plus the final x.  Not supported together with theta.
        sampler: None or "ddim" (the samplers above); "dpmpp_2m" runs DPM-Solver++(2M) over `steps` (an int S, spaced
        uniformly in log-SNR by `logsnr_timesteps`, or an explicit sequence), S forwards, deterministic (eta must be 0; no
        noise is drawn after x_T).  Guidance, graph= and the snapshots work as for DDIM.  "unipc_1" / "unipc_2" / "unipc_3"
        ("unipc" = "unipc_2") run UniPC of that order under the same rules: a predictor-corrector that still costs one forward
        per step.  Order 3 pays from about S = 16 on; below that its extrapolation over log-SNR steps near 1 is worse than
        "unipc_2" or "dpmpp_2m" (DESIGN.md section 6z).
        `sample_analytic` is this sampler's DDIM chain drawing with the optimal variances of Analytic-DPM."""
        logging.info(f"Sampling {n} new images....")
        if theta is not None:
            logging.info(f"Theta {theta} provided. Rotation will be applied.")
        solver, pairs = self._check_sampler("sample", sampler, steps, eta, theta)
        if labels is not None:
            labels = self._check_labels(model, n, theta, labels)
        elif cfg_scale:
            raise ValueError("Diffusion.sample: cfg_scale needs class labels")
        if solver == "dpmpp_2m":
            x, snaps = self._dpmpp_loop(model, n, image_channels, pairs, noise_source, graph, labels, float(cfg_scale))
        elif solver in self.UNIPC_SAMPLERS:
            x, snaps = self._unipc_loop(model, n, image_channels, pairs, self.UNIPC_SAMPLERS[solver], noise_source, graph, labels,
                                        float(cfg_scale))
        elif pairs is None:
            x, snaps = self._loop(model, n, image_channels, theta, noise_source, graph, labels=labels, cfg_scale=float(cfg_scale))
        else:
            x, snaps = self._ddim_loop(model, n, image_channels, pairs, float(eta), noise_source, graph, labels, float(cfg_scale))
        return self._finish(x, snaps, return_float)

    def sample_analytic(self, model, n, image_channels, analytic, theta=None, noise_source="reference", return_float=False, graph=None,
                        labels=None, cfg_scale=0.0, steps=None, eta=0.0, sampler=None):
        """`sample` over the DDIM chain `steps` with the optimal reverse variances of Analytic-DPM (Bao et al. 2022): `sample`'s
        arguments with `analytic`, an `AnalyticVariance` (`estimate_analytic_variance`) that holds an estimate at every
        timestep of the chain.  The chain keeps DDIM's mean at that eta (eta = 1: Analytic-DDPM, eta = 0: Analytic-DDIM) and
        draws with sigma* in place of eta^2 beta~, which is far too small on a short chain: every step but the last draws the
        noise of n images, also at eta = 0.  x_T, the generator path, labels, guidance (the table should then be the guided
        eps's: estimate it with the same cfg_scale), graph=, return_float and the snapshots are `sample`'s.  Refused with
        ValueError before any device work: steps=None (pass steps=T-1 for the full chain), a sampler other than None / "ddim",
        theta, a process with variance="learned", a table of another process or one that misses a timestep of the chain.
        (A method of its own because `sample`'s parameter list is pinned.)  Returns what `sample` returns."""
        logging.info(f"Sampling {n} new images....")
        self._check_analytic("sample_analytic", analytic, steps, sampler, theta)
        pairs = self._check_ddim("sample_analytic", steps, eta)
        analytic.sigma2(self, pairs, eta)                      # refuses a foreign table or a missing timestep before any device work
        if labels is not None:
            labels = self._check_labels(model, n, None, labels, "sample_analytic")
        elif cfg_scale:
            raise ValueError("Diffusion.sample_analytic: cfg_scale needs class labels")
        x, snaps = self._ddim_loop(model, n, image_channels, pairs, float(eta), noise_source, graph, labels, float(cfg_scale),
                                   analytic=analytic)
        return self._finish(x, snaps, return_float)

    def _check_analytic(self, where, analytic, steps, sampler=None, theta=None):
        """ValueError for a request the analytic variance cannot serve; nothing touches a device."""
        if not isinstance(analytic, AnalyticVariance):
            raise ValueError(f"Diffusion.{where}: analytic must be an AnalyticVariance (got {type(analytic).__name__})")
        if steps is None:
            raise ValueError(f"Diffusion.{where}: analytic needs steps (the analytic variance belongs to the DDIM chain: pass "
                             f"steps={self.noise_steps - 1}, T - 1, for the full chain)")
        if not (sampler is None or (isinstance(sampler, str) and sampler == "ddim")):
            raise ValueError(f"Diffusion.{where}: analytic goes with sampler None or 'ddim' (got {sampler!r}: that solver draws no noise)")
        if theta is not None:
            raise ValueError(f"Diffusion.{where}: analytic together with a rotation (theta) is not supported")
        if self.variance == "learned":
            raise ValueError(f"Diffusion.{where}: analytic is for a process with variance='fixed' (this one draws with the variance "
                             "its network emits)")

    def _finish(self, x, snaps, return_float):
        """What `sample` and `inpaint` return: the final x and the snapshots, quantised; with return_float also x itself."""
        self.last_float_snapshots = snaps          # pre-quantisation x at i % 100 == 0 and the final x (parity tests)
        xq = ops.quantize_u8(x)
        rq = ops.quantize_u8(torch.cat(snaps))
        if return_float:
            return xq, rq, x
        return xq, rq

    # Inpainting (RePaint, Lugmayr et al. 2022) -----------------------------------------------------------------------------
    @staticmethod
    def repaint_moves(chain, jump_length, jump_n_sample):
        """RePaint's resampling schedule (its get_schedule_jump, re-indexed onto chain positions) as a list of moves
        (t_from, t_to).  chain: the strictly decreasing model timesteps (T-1 .. 1 for DDPM, the DDIM taus); levels = chain + [0].
        A down-move (t > t_to) is one forward and a masked update; an up-move (t < t_to) renoises the whole image.  Every
        position p (0 < p < S, (S - 1 - p) % j == 0, p >= j) is left jump_n_sample - 1 times by an up-move of jump_length
        positions.  jump_n_sample = 1 gives the plain chain."""
        for name, v in (("jump_length", jump_length), ("jump_n_sample", jump_n_sample)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"Diffusion.repaint_moves: {name} must be an int >= 1 (got {v!r})")
        chain = [int(v) for v in chain]
        if not chain or chain[-1] < 1 or any(a <= b for a, b in zip(chain, chain[1:])):
            raise ValueError(f"Diffusion.repaint_moves: chain must be a non-empty, strictly decreasing list of timesteps >= 1")
        j, r = int(jump_length), int(jump_n_sample)
        levels, S = chain + [0], len(chain)
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

    def _inpaint_inputs(self, images, mask):
        """-> (images, mask) on the device: fp32 (n, C, img_size, img_size) and a contiguous uint8 mask of the same shape."""
        self._check_images("inpaint", images)
        m = torch.as_tensor(mask)
        if m.dtype.is_complex:
            raise ValueError("Diffusion.inpaint: mask must hold 0 or 1")
        try:
            shape = torch.broadcast_shapes(tuple(m.shape), tuple(images.shape))
        except RuntimeError:
            shape = None
        if shape != tuple(images.shape):
            raise ValueError(f"Diffusion.inpaint: mask of shape {tuple(m.shape)} does not broadcast to images {tuple(images.shape)}")
        if not bool(((m == 0) | (m == 1)).all()):
            raise ValueError("Diffusion.inpaint: every mask value must be 0 or 1 (1 = known: keep the pixel of images)")
        x0 = images.to(self.device).contiguous()
        m = m.to(self.device).to(torch.uint8).expand(x0.shape).contiguous()
        return x0, m

    def inpaint(self, model, images, mask, steps=None, eta=0.0, labels=None, cfg_scale=0.0, jump_length=10, jump_n_sample=1,
                noise_source="reference", graph=None, return_float=False):
        """Fill the region of `images` where `mask` is 0 and keep the rest (RePaint, Lugmayr et al. 2022): no retraining.
        images: (n, C, img_size, img_size) fp32 in [-1, 1]; mask: broadcasts to images.shape, every value 0 or 1, 1 = known.
        steps / eta / labels / cfg_scale / noise_source / graph: as for `sample`.  x_T is drawn as `sample` draws it.  Each
        down-move t -> t_prev draws the noise of n images where `sample` draws it (after the forward), and whenever t_prev > 0
        (also for DDIM with eta = 0): a generated pixel uses it as the sampler's step noise, a known pixel to noise images to
        t_prev (at t_prev = 0 the known pixels are images itself).  With an all-zero mask the output is `sample`'s, bit for bit.
        jump_n_sample (RePaint's r) and jump_length (j): resampling (`repaint_moves`); every up-move draws the noise of n
        images and renoises the whole image.  graph=True captures one down-move and replays it; up-moves and the last step run
        eagerly in between.  Snapshots: after every down-move that crosses a multiple of 100 (`ddim_snapshot`), so a
        re-descended segment adds its snapshots again, plus the final x.  Returns what `sample` returns."""
        logging.info(f"Inpainting {images.shape[0] if isinstance(images, torch.Tensor) else '?'} images....")
        pairs = self._check_ddim("inpaint", steps, eta)
        chain = list(range(self.noise_steps - 1, 0, -1)) if pairs is None else [t for t, _ in pairs]
        moves = self.repaint_moves(chain, jump_length, jump_n_sample)
        x0, m = self._inpaint_inputs(images, mask)
        n = x0.shape[0]
        if labels is not None:
            labels = self._check_labels(model, n, None, labels)
        elif cfg_scale:
            raise ValueError("Diffusion.inpaint: cfg_scale needs class labels")
        x, snaps = self._inpaint_loop(model, x0, m, moves, None if pairs is None else float(eta), noise_source, graph, labels,
                                      float(cfg_scale))
        return self._finish(x, snaps, return_float)

    def _update(self, xs, n, out, z, t, tp=None, eta=None, learned=False, cfg_scale=0.0, x0=None, mask=None, sig=None):
        """One update of the state xs, in place: its n rows, or both halves of the 2n rows [x ; x] of a guided forward
        (cfg_scale > 0).  out: that forward's output (eps; with `learned` the raw 2C output); z: the step's noise of n images, or
        None.  eta None: the DDPM step t -> t - 1, with the fixed or (`learned`) the network's variance; otherwise the DDIM step
        t -> tp.  x0 and mask: the masked form of `inpaint`.  t and tp: host ints, or int64 device tensors (the graph-replayable
        _dev form).  sig: the (T,) fp32 device table of the analytic sigmas; the DDIM step then scales z by sig[t].  One launch:
        the wrapper these facts name, ops.{denoise,ddim}_step[_var][_lvar][_masked][_cfg][_dev]."""
        ddim, masked, guided, dev = eta is not None, mask is not None, cfg_scale > 0, isinstance(t, torch.Tensor)
        var = sig is not None
        if learned and (ddim or masked):
            raise NotImplementedError("Diffusion: the learned variance is drawn by the unmasked DDPM step alone")
        if var and (masked or not ddim):
            raise NotImplementedError("Diffusion: the analytic variance is drawn by the unmasked DDIM step alone")
        step = getattr(ops, ("ddim_step" if ddim else "denoise_step") + "_var" * var + "_lvar" * learned + "_masked" * masked
                       + "_cfg" * guided + "_dev" * dev)
        x = xs[:n] if guided else xs
        args = [x, out, z] + ([x0, mask] if masked else [])
        if ddim:
            args += [self.alpha_hat] + ([sig] if var else []) + [t, tp, eta]
        else:
            args += [self.alpha, self.alpha_hat, self.beta] + ([self._lv(), self.prediction] if learned else []) + [t]
        step(*args, *([cfg_scale, x, xs[n:]] if guided else [x]))

    def _inpaint_loop(self, model, x0, mask, moves, eta, noise_source, graph, labels, cfg_scale):
        """`inpaint`'s trajectory over `moves`.  The state lives in xs: n rows, or the 2n rows [x ; x] of the guided forward,
        which every update writes in place (both halves).  eta None: DDPM updates."""
        n, c = x0.shape[0], x0.shape[1]
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, c, noise_source)
            y, s = self._guided(labels, cfg_scale)
            xs = torch.cat([x, x]) if s > 0 else x
            rows = xs.shape[0]

            def step(t_rows, t, tp, draw):
                eps = self.predict_eps(model, xs, t_rows, y)
                self._update(xs, n, eps, draw() if draw else None, t, tp, eta=eta, cfg_scale=s, x0=x0, mask=mask)

            replay = None
            first = next(((t, tp) for t, tp in moves if t > tp > 0), None)
            if graph and noise_source != "cpu" and first is not None:
                t_dev = torch.full((rows,), first[0], device=x.device, dtype=torch.long)
                tp_dev = torch.full((1,), first[1], device=x.device, dtype=torch.long)
                g = self._capture(lambda: step(t_dev, t_dev, tp_dev, lambda: torch.randn_like(xs[:n])), xs)

                def replay(t, tp):
                    t_dev.fill_(t)
                    tp_dev.fill_(tp)
                    g.replay()
            for t, tp in moves:
                if tp > t:                                   # up-move: renoise the whole image from level t to tp
                    z = self._step_noise(xs[:n], noise_source)
                    ops.renoise(xs[:n], z, self.alpha_hat, t, tp, out=xs[:n])
                    if s > 0:
                        xs[n:].copy_(xs[:n])
                    continue
                if replay is not None and tp > 0:
                    replay(t, tp)
                else:
                    step(self._t_full(rows, t, x.device), t, tp, (lambda: self._step_noise(xs[:n], noise_source)) if tp > 0 else None)
                if self.ddim_snapshot(t, tp):
                    snaps.append(xs[:n].clone())
            x = xs[:n].clone()
        snaps.append(x)
        return x, snaps

    # Reference-guided sampling (ILVR, Choi et al. 2021) ------------------------------------------------------------------------------
    def _ilvr_operator(self, where, factor, taps):
        """-> (ops.Taps, levels) of phi = 4^levels up2^levels(down2^levels(.)): factor = 2^levels; taps None = the default filter."""
        if self.img_size not in ops.REFINE_SIDES:
            raise NotImplementedError(f"Diffusion.{where}: img_size must be a power of two in [4, 64] (got {self.img_size})")
        if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or factor < 2 or factor & (factor - 1) \
                or 2 * factor > self.img_size:
            raise ValueError(f"Diffusion.{where}: factor must be a power of two in [2, {self.img_size // 2}] (got {factor!r})")
        if taps is None:
            taps = circularLowpassKernel(math.pi / 2, 9, beta=8)
        k = taps.detach().cpu().numpy() if isinstance(taps, torch.Tensor) else np.asarray(taps)
        if k.ndim != 2 or k.shape[0] != k.shape[1] or k.shape[0] % 2 == 0 or k.shape[0] > 15 or k.dtype.kind not in "fiu":
            raise ValueError(f"Diffusion.{where}: taps must be an (N, N) array of numbers with N odd and at most 15 "
                             f"(got shape {tuple(k.shape)}): an even N shifts the image by half a pixel per pass")
        return ops.Taps(k), int(factor).bit_length() - 1

    def _ilvr_reference(self, reference):
        self._check_images("ilvr", reference, "reference")
        return reference.to(self.device).contiguous()

    def reference_from_lowres(self, low, factor, taps=None):
        """A full-size reference for `ilvr` from low-resolution images: 4^L up2^L(low) with factor = 2^L, through the filtered
        upsampler (ops.FiltUp2).  low: fp32 (n, C, img_size / factor, img_size / factor); taps as for `ilvr`.  For low =
        down2^L(v) this is ops.lowpass_project(v): `ilvr` on it super-resolves.  Returns the reference on the device."""
        k, levels = self._ilvr_operator("reference_from_lowres", factor, taps)
        side = self.img_size >> levels
        if not isinstance(low, torch.Tensor) or low.dtype != torch.float32:
            raise ValueError("Diffusion.reference_from_lowres: low must be an fp32 tensor")
        if low.dim() != 4 or low.shape[0] < 1 or tuple(low.shape[2:]) != (side, side):
            raise ValueError(f"Diffusion.reference_from_lowres: low must have shape (n, C, {side}, {side}) (got {tuple(low.shape)})")
        x = low.to(self.device).contiguous()
        with torch.no_grad():
            for _ in range(levels):
                x = ops.FiltUp2.apply(x, k)
            return x.mul_(float(4 ** levels))

    def ilvr(self, model, reference, factor=4, t_stop=0, taps=None, steps=None, eta=0.0, labels=None, cfg_scale=0.0,
             noise_source="reference", graph=None, return_float=False):
        """Draw samples that share the coarse content of `reference` (ILVR, Choi et al. 2021): no retraining.  After the update of
        a move t -> t_prev the state's low frequencies are replaced by those of the reference noised to t_prev,
            x <- x + phi(y - x),   y ~ q(x_t_prev | reference)   (y = reference at t_prev = 0),
        with phi = 4^L up2^L(down2^L(.)) (factor = 2^L) built from the filtered resamplers: one fused launch per move
        (ops.lowpass_refine).
        reference: fp32 (n, C, img_size, img_size) in [-1, 1]; img_size must be a power of two in [4, 64].
        factor: a power of two, 2 <= factor <= img_size / 2; the larger, the less of the reference is kept.
        t_stop: an int in [0, T]; a move is refined when t_prev >= t_stop (0: every move, the last included; >= T - 1: none, and
        the result, the snapshots and the generators' positions are `sample`'s, bit for bit).
        taps: None = circularLowpassKernel(pi / 2, 9, beta=8); otherwise an (N, N) array or tensor, N odd and at most 15.  Symmetric
        taps (taps == taps.T, and the same read backwards) are what makes up2 the transpose of down2, hence phi symmetric positive
        semi-definite with eigenvalues at most about 1: the refinement then never expands.  Asymmetric taps are accepted and
        carry no such promise.
        steps / eta / labels / cfg_scale / noise_source / graph: as for `sample` (DDPM with steps=None, the learned variance
        included, or DDIM; there is no DPM-Solver++ form: its multistep history would be stale after a refinement).  Each move
        draws the step's noise exactly where `sample` draws it; a refined move with t_prev > 0 then draws the noise of n images
        for the reference.  graph=True captures one refined move (forward, both draws, update, refinement with t_prev read on the
        device) and, when t_stop > 0, one unrefined move, and replays them; the last move runs eagerly.  Snapshots as `sample`
        (`ddim_snapshot`).  Returns what `sample` returns."""
        logging.info(f"Sampling {reference.shape[0] if isinstance(reference, torch.Tensor) else '?'} images guided by a reference....")
        k, levels = self._ilvr_operator("ilvr", factor, taps)
        ref = self._ilvr_reference(reference)
        T = self.noise_steps
        if isinstance(t_stop, bool) or not isinstance(t_stop, (int, np.integer)) or not 0 <= t_stop <= T:
            raise ValueError(f"Diffusion.ilvr: t_stop must be an int in [0, {T}] (got {t_stop!r})")
        pairs = self._check_ddim("ilvr", steps, eta)
        n = ref.shape[0]
        if labels is not None:
            labels = self._check_labels(model, n, None, labels, "ilvr")
        elif cfg_scale:
            raise ValueError("Diffusion.ilvr: cfg_scale needs class labels")
        moves = [(t, t - 1) for t in range(T - 1, 0, -1)] if pairs is None else pairs
        x, snaps = self._ilvr_loop(model, ref, k, levels, int(t_stop), moves, None if pairs is None else float(eta), noise_source,
                                   graph, labels, float(cfg_scale))
        return self._finish(x, snaps, return_float)

    def _ilvr_loop(self, model, ref, taps, levels, t_stop, moves, eta, noise_source, graph, labels, cfg_scale):
        """`ilvr`'s trajectory over `moves`, [(t, t_prev)] descending to 0.  eta None: DDPM updates (with the network's variance
        when it is learned), otherwise DDIM.  The state lives in xs as in `_inpaint_loop`; a refined move adds one launch that
        writes both halves of a guided state."""
        n, c = ref.shape[0], ref.shape[1]
        self.check_model(model, c, "Diffusion.ilvr")
        learned = eta is None and self.variance == "learned"
        forward = self._raw_output if learned else self.predict_eps      # learned: the raw 2C output goes to the update
        takes_noise = eta is None or eta > 0
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, c, noise_source)
            y, s = self._guided(labels, cfg_scale)
            xs = torch.cat([x, x]) if s > 0 else x
            rows = xs.shape[0]

            def step(t_rows, t, tp, draw, draw_ref, refined):
                out = forward(model, xs, t_rows, y)
                self._update(xs, n, out, draw() if draw else None, t, tp, eta=eta, learned=learned, cfg_scale=s)
                if refined:
                    refine = ops.lowpass_refine_dev if isinstance(tp, torch.Tensor) else ops.lowpass_refine
                    refine(xs[:n], ref, draw_ref() if draw_ref else None, self.alpha_hat, tp, taps, levels, out=xs[:n],
                           out2=xs[n:] if s > 0 else None)

            replay = None
            first = next(((t, tp) for t, tp in moves if tp > 0), None)
            if graph and noise_source != "cpu" and first is not None:
                t_dev = torch.full((rows,), first[0], device=x.device, dtype=torch.long)
                tp_dev = torch.full((1,), first[1], device=x.device, dtype=torch.long)
                dev_draw = lambda: torch.randn_like(xs[:n])
                graphs = {}                                  # one capture per kind of move (refined or not), made when first needed

                def replay(t, tp, refined):
                    if refined not in graphs:
                        graphs[refined] = self._capture(
                            lambda: step(t_dev, t_dev, tp_dev, dev_draw if takes_noise else None, dev_draw, refined), xs)
                    t_dev.fill_(t)
                    tp_dev.fill_(tp)
                    graphs[refined].replay()
            host_draw = lambda: self._step_noise(xs[:n], noise_source)
            for t, tp in moves:
                refined = tp >= t_stop
                if replay is not None and tp > 0:            # the last move draws no noise: it runs eagerly
                    replay(t, tp, refined)
                else:
                    step(self._t_full(rows, t, x.device), t, tp, host_draw if takes_noise and tp > 0 else None,
                         host_draw if tp > 0 else None, refined)
                if self.ddim_snapshot(t, tp):
                    snaps.append(xs[:n].clone())
            x = xs[:n].clone()
        snaps.append(x)
        return x, snaps

    # Diffusion posterior sampling (DPS, Chung et al. 2023) for noisy linear measurements ---------------------
    def x0_coefficients(self, t):
        """(a, b), two (B,) fp64 host tensors with x0_hat = a x_t + b out for `self.prediction` at the timesteps t: (1 / sqrt(ah),
        -sqrt(1 - ah) / sqrt(ah)) for "eps", (sqrt(ah), -sqrt(1 - ah)) for "v" and (0, 1) for "x0", ah the fp32 alpha_hat[t]
        widened to fp64.  The kernels round each once to fp32 (afd.h: afd_dps_residual)."""
        ah = self.alpha_hat.detach().cpu().double()[torch.as_tensor(t).cpu().long()]
        sa, sb = torch.sqrt(ah), torch.sqrt(1.0 - ah)
        if self.prediction == "v":
            return sa, -sb
        if self.prediction == "x0":
            return torch.zeros_like(ah), torch.ones_like(ah)
        return 1.0 / sa, -sb / sa

    def _output_and_vjp(self, model, x_t, t, y, seed_fn):
        """-> (out, v): the network's output at x_t, detached, and its vector-Jacobian product v = (d out / d x_t)^T g with the seed
        g = seed_fn(out).  One forward and one backward under enable_grad (the samplers' scope runs under no_grad), x_t a fresh
        leaf.  While it runs every parameter of the model is frozen (requires_grad False), so the ops that look at
        needs_input_grad compute no weight gradient, and no parameter's .grad is written; the flags come back as they were found,
        also after an exception.  Works for any differentiable nn.Module."""
        frozen = [p for p in model.parameters() if p.requires_grad]
        for p in frozen:
            p.requires_grad_(False)
        try:
            with torch.enable_grad():
                x = x_t.detach().requires_grad_(True)
                out = self._raw_output(model, x, t, y)
                found = out.detach()
                with torch.autograd.set_multithreading_enabled(False):          # backward on the calling thread, as TrainStep runs it
                    (v,) = torch.autograd.grad(out, x, seed_fn(found))
        finally:
            for p in frozen:
                p.requires_grad_(True)
        return found, v.contiguous()

    def posterior_sample(self, model, measurement, operator, zeta=1.0, steps=None, eta=0.0, labels=None, noise_source="reference",
                         return_float=False):
        """Restore images from a noisy linear measurement y = A x + sigma n without retraining (diffusion posterior sampling,
        Chung et al. 2023): after every step of the chain the state moves down the gradient, with respect to x_t, of
        |y - A x0_hat(x_t)|, with the step zeta / |y - A x0_hat| per row,
            x <- update(x, out) - zeta grad_{x_t} |y - A x0_hat(x_t)|,     x0_hat = a_t x_t + b_t out(x_t)   (`x0_coefficients`).
        measurement: fp32 (n, C, h, w); operator: a `posterior.LinearOperator`, whose stride gives the image size
        (h s, w s) = (img_size, img_size).  zeta: a finite number >= 0, the guidance's weight (0: the plain sampler's images,
        at the same cost).
        steps=None runs the DDPM chain, an int or an explicit sequence DDIM with `eta`, as `sample` does; x_T, the steps' noise,
        the snapshots and the result are drawn, taken and returned as `sample` draws, takes and returns them.
        Per step: one forward and one backward of the network (`_output_and_vjp`; the parameters are frozen meanwhile), the fused
        residual kernel as the backward's seed (ops.dps_residual), the sampler's own update, and one elementwise correction
        (ops.dps_correct), on the last step too; nothing is read back from the device.
        labels: class labels for a conditional model.  Classifier-free guidance is not offered (it would need the
        vector-Jacobian product of a 2n-row combination), nor variance="learned", graph capture or a rotation."""
        where = "posterior_sample"
        from .posterior import LinearOperator
        if not isinstance(operator, LinearOperator):
            raise ValueError(f"Diffusion.{where}: operator must be a posterior.LinearOperator (got {type(operator).__name__})")
        if isinstance(zeta, bool) or not isinstance(zeta, (int, float, np.integer, np.floating)) or not (zeta >= 0 and math.isfinite(zeta)):
            raise ValueError(f"Diffusion.{where}: zeta must be a finite number >= 0 (got {zeta!r})")
        if self.variance == "learned":
            raise ValueError(f"Diffusion.{where}: variance='learned' is not supported (the guidance differentiates the prediction "
                             f"alone and the chain keeps the fixed variance)")
        if not isinstance(measurement, torch.Tensor) or measurement.dtype != torch.float32 or measurement.dim() != 4 \
                or measurement.shape[0] < 1:
            raise ValueError(f"Diffusion.{where}: measurement must be an fp32 (n, C, h, w) tensor with n >= 1")
        s, S = operator.stride, self.img_size
        if not 1 <= S <= 64 or S % s or tuple(measurement.shape[2:]) != (S // s, S // s):
            raise ValueError(f"Diffusion.{where}: at stride {s} and img_size {S} (at most 64, a multiple of the stride) the measurement "
                             f"must have shape (n, C, {S // s}, {S // s}) (got {tuple(measurement.shape)})")
        n, C = int(measurement.shape[0]), int(measurement.shape[1])
        try:
            operator._mask_for(C, S // s, S // s)
        except ValueError as e:
            raise ValueError(f"Diffusion.{where}: {e}") from None
        logging.info(f"Restoring {n} images from their measurements....")
        pairs = self._check_ddim(where, steps, eta)
        if labels is not None:
            labels = self._check_labels(model, n, None, labels, where)
        self.check_model(model, C, f"Diffusion.{where}")
        moves = [(t, t - 1) for t in range(self.noise_steps - 1, 0, -1)] if pairs is None else pairs
        ddim_eta = None if pairs is None else float(eta)
        takes_noise = ddim_eta is None or ddim_eta > 0
        zeta = float(zeta)
        snaps = []
        with self._model_scope(model):
            x = self._initial_noise(n, C, noise_source)
            y = measurement.to(self.device).contiguous()
            taps, mask = operator._taps, operator._device_mask(x.device)
            g = torch.empty_like(x)
            sums = torch.empty(n, C, device=x.device, dtype=torch.float64)
            for t, tp in moves:
                t_rows = self._t_full(n, t, x.device)
                seed = lambda out: ops.dps_residual(x, out, t_rows, self.alpha_hat, self.prediction, y, taps, s, mask, g, sums)[0]
                out, v = self._output_and_vjp(model, x, t_rows, labels, seed)
                eps = out if self.prediction == "eps" else ops.pred_to_eps(out, x, t_rows, self.alpha_hat, self.prediction, eps_out=out)
                z = self._step_noise(x, noise_source) if takes_noise and tp > 0 else None
                self._update(x, n, eps, z, t, tp if ddim_eta is not None else None, eta=ddim_eta)
                ops.dps_correct(x, g, v, sums, t_rows, self.alpha_hat, self.prediction, zeta)
                if self.ddim_snapshot(t, tp):
                    snaps.append(x.clone())
            x = x.clone()
        snaps.append(x)
        return self._finish(x, snaps, return_float)

    # Real images: DDIM inversion with fixed-point refinement, decoding, SDEdit, interpolation ----------------
    def ddim_timesteps_from(self, t0, steps):
        """The S = `steps` timesteps of a DDIM chain that starts at t0 instead of T - 1, strictly decreasing:
        tau_k = 1 + (k (t0 - 1)) // (S - 1) for k = 0 .. S-1, in descending order (S = 1: [t0]); needs 1 <= S <= t0 <= T - 1.
        ddim_timesteps_from(T - 1, S) == ddim_timesteps(S)."""
        T = self.noise_steps
        for name, v in (("t0", t0), ("steps", steps)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Diffusion.ddim_timesteps_from: {name} must be an int (got {type(v).__name__})")
        t0, S = int(t0), int(steps)
        if not 1 <= S <= t0 <= T - 1:
            raise ValueError(f"Diffusion.ddim_timesteps_from: needs 1 <= steps <= t0 <= {T - 1} (got steps = {S}, t0 = {t0})")
        if S == 1:
            return [t0]
        return [1 + (k * (t0 - 1)) // (S - 1) for k in reversed(range(S))]

    def _invert_moves(self, steps):
        """The moves (s, u) of `invert` over `steps` (what `sample(steps=)` accepts): the sampler's pairs (t, t_prev) reversed and
        swapped, so the chain climbs the levels [0] + reversed(taus) and ends at taus[0]."""
        return [(tp, t) for t, tp in reversed(self._ddim_pairs(steps, 0.0))]

    def _check_images(self, where, images, name="images"):
        """ValueError unless `images` is an fp32 (n, C, img_size, img_size) tensor with n >= 1; nothing is moved."""
        if not isinstance(images, torch.Tensor) or images.dtype != torch.float32:
            raise ValueError(f"Diffusion.{where}: {name} must be an fp32 tensor")
        if images.dim() != 4 or images.shape[0] < 1 or tuple(images.shape[2:]) != (self.img_size, self.img_size):
            raise ValueError(f"Diffusion.{where}: {name} must have shape (n, C, {self.img_size}, {self.img_size}) "
                             f"(got {tuple(images.shape)})")

    def _check_guidance(self, where, model, n, labels, cfg_scale):
        """-> the labels on the device (or None), as `sample` checks them; cfg_scale without labels is refused."""
        if labels is not None:
            return self._check_labels(model, n, None, labels, where)
        if cfg_scale:
            raise ValueError(f"Diffusion.{where}: cfg_scale needs class labels")
        return None

    def invert(self, model, images, steps, refine=0, labels=None, cfg_scale=0.0, graph=None):
        """DDIM inversion: the latents at level taus[0] whose deterministic DDIM chain (`decode` with eta = 0 over the same
        `steps`, labels and cfg_scale) regenerates `images`.  images: fp32 (n, C, img_size, img_size) in [-1, 1]; steps: what
        `sample(steps=)` accepts, an int S (`ddim_timesteps`) or an explicit strictly decreasing sequence.  The chain is walked
        upwards over the levels [0] + reversed(taus) (`_invert_moves`).  A move s -> u evaluates the model at timestep u (always
        >= 1: `sample_timesteps` never draws 0, so the network is untrained there) and iterates
            z_0 = x_s,   z_{k+1} = step(x_s, eps_theta(z_k, u), s, u)  for k = 0 .. refine,   x_u = z_{refine + 1}
        with step = ops.ddim_invert_step: each iteration is one iteration of the fixed-point equation whose solution is the exact
        inverse of the sampler's step u -> s.  refine = 0 is plain DDIM inversion, one forward per level; each further iteration
        costs one more forward, (refine + 1) S in all.  With guidance the 2n rows [z ; z] go through one forward and the guided
        step writes both halves.  Nothing is drawn: no generator's state changes.  graph=True captures one iteration (forward
        and the step with s and u read on the device) and replays it.  Returns fp32 (n, C, img_size, img_size) on the device."""
        logging.info(f"Inverting {images.shape[0] if isinstance(images, torch.Tensor) else '?'} images....")
        self._check_images("invert", images)
        moves = self._invert_moves(steps)
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
            raise ValueError(f"Diffusion.invert: refine must be an int >= 0 (got {refine!r})")
        n = images.shape[0]
        labels = self._check_guidance("invert", model, n, labels, cfg_scale)
        self.check_model(model, images.shape[1], "Diffusion.invert")
        return self._invert_loop(model, images, moves, int(refine), graph, labels, float(cfg_scale))

    def _invert_loop(self, model, images, moves, refine, graph, labels, cfg_scale):
        """`invert`'s trajectory over `moves`, [(s, u)] ascending from 0.  base holds x_s and is only read within a level; the
        iterate lives in zs, n rows or the 2n rows [z ; z] of the guided forward, which every step writes (both halves)."""
        with self._model_scope(model):
            base = images.to(self.device).contiguous().clone()
            n = base.shape[0]
            y, s = self._guided(labels, cfg_scale)
            zs = torch.cat([base, base]) if s > 0 else base.clone()
            rows = zs.shape[0]

            def iterate(t_rows, lo, hi):
                eps = self.predict_eps(model, zs, t_rows, y)
                dev = "_dev" if isinstance(lo, torch.Tensor) else ""
                if s > 0:
                    getattr(ops, "ddim_invert_step_cfg" + dev)(base, eps, self.alpha_hat, lo, hi, s, zs[:n], zs[n:])
                else:
                    getattr(ops, "ddim_invert_step" + dev)(base, eps, self.alpha_hat, lo, hi, zs)

            replay = None
            if graph and len(moves) * (refine + 1) > 1:
                t_dev = torch.full((rows,), moves[0][1], device=base.device, dtype=torch.long)
                lo_dev = torch.full((1,), moves[0][0], device=base.device, dtype=torch.long)
                g = self._capture(lambda: iterate(t_dev, lo_dev, t_dev), zs)

                def replay(lo, hi):
                    lo_dev.fill_(lo)
                    t_dev.fill_(hi)
                    g.replay()
            for lo, hi in moves:
                for _ in range(refine + 1):
                    if replay is not None:
                        replay(lo, hi)
                    else:
                        iterate(self._t_full(rows, hi, base.device), lo, hi)
                base.copy_(zs[:n])
        return base

    def decode(self, model, latents, steps, eta=0.0, labels=None, cfg_scale=0.0, noise_source="reference", graph=None,
               return_float=False):
        """The DDIM chain of `sample` started from `latents`, the state at level taus[0], instead of drawn noise.  latents: fp32
        (n, C, img_size, img_size), e.g. what `invert` returns for the same `steps`; it is not written.  steps / eta / labels /
        cfg_scale / noise_source / graph / return_float and the snapshots: as for `sample` with steps= (DDIM only: there is no
        sampler argument).  With eta > 0 the step noise comes from the generator path `sample` uses; with eta = 0 nothing is
        drawn.  For latents drawn as `sample` draws x_T the result is `sample`'s, bit for bit.  Returns what `sample` returns."""
        logging.info(f"Decoding {latents.shape[0] if isinstance(latents, torch.Tensor) else '?'} latents....")
        self._check_images("decode", latents, "latents")
        if steps is None:
            raise ValueError("Diffusion.decode: steps is required (an int or an explicit sequence of timesteps: DDIM only)")
        pairs = self._check_ddim("decode", steps, eta)
        n, c = latents.shape[0], latents.shape[1]
        labels = self._check_guidance("decode", model, n, labels, cfg_scale)
        x, snaps = self._ddim_loop(model, n, c, pairs, float(eta), noise_source, graph, labels, float(cfg_scale), start=latents)
        return self._finish(x, snaps, return_float)

    def sdedit(self, model, images, t0, steps, eta=0.0, labels=None, cfg_scale=0.0, noise_source="reference", graph=None,
               return_float=False):
        """SDEdit (Meng et al. 2022): noise `images` to level t0 and denoise them from there, so the coarse content survives and
        the detail is drawn anew; the larger t0, the freer the edit.  images: fp32 (n, C, img_size, img_size) in [-1, 1], e.g. a
        stroke painting or a composite; t0: an int in [1, T - 1].  z is drawn as `sample` draws x_T (`_initial_noise`),
        x = ops.noise_images(images, z, t0, alpha_hat), then `decode` over ddim_timesteps_from(t0, S) for an int `steps` = S, or
        over an explicit sequence whose first element must be t0.  Everything else as `decode`.  Returns what `sample` returns."""
        logging.info(f"Editing {images.shape[0] if isinstance(images, torch.Tensor) else '?'} images....")
        self._check_images("sdedit", images)
        T = self.noise_steps
        if isinstance(t0, bool) or not isinstance(t0, (int, np.integer)) or not 1 <= t0 <= T - 1:
            raise ValueError(f"Diffusion.sdedit: t0 must be an int in [1, {T - 1}] (got {t0!r})")
        if steps is None:
            raise ValueError("Diffusion.sdedit: steps is required (an int or an explicit sequence of timesteps starting at t0)")
        if isinstance(steps, (int, np.integer)) and not isinstance(steps, bool):
            steps = self.ddim_timesteps_from(int(t0), steps)
        pairs = self._check_ddim("sdedit", steps, eta)
        if pairs[0][0] != t0:
            raise ValueError(f"Diffusion.sdedit: an explicit steps sequence must start at t0 = {t0} (got {list(steps)!r})")
        n, c = images.shape[0], images.shape[1]
        self._check_guidance("sdedit", model, n, labels, cfg_scale)
        z = self._initial_noise(n, c, noise_source)
        x = ops.noise_images(images.to(self.device), z, self._t_full(n, int(t0), z.device), self.alpha_hat)
        return self.decode(model, x, [t for t, _ in pairs], eta, labels, cfg_scale, noise_source, graph, return_float)

    def interpolate(self, model, a, b, weights, steps, refine=0, labels=None, cfg_scale=0.0, graph=None, return_float=False):
        """Interpolate between the images a and b through their latents: `invert` torch.cat([a, b]) as one batch of 2n rows (labels
        repeated), ops.slerp(lat[:n], lat[n:], weights) -> (n, W, ...), and `decode` the n W rows as one batch with eta = 0 (the
        labels repeated per weight).  Rows are ordered (pair, weight): row i W + k is pair i at weights[k]; weight 0 reconstructs
        a, weight 1 b.  The batching is part of the contract: the result equals those three public calls made by hand, bit for
        bit.  a, b: fp32 (n, C, img_size, img_size) in [-1, 1]; weights: a non-empty 1-D sequence of finite numbers; steps /
        refine / labels / cfg_scale / graph: as for `invert` and `decode`.  Returns what `sample` returns."""
        self._check_images("interpolate", a, "a")
        self._check_images("interpolate", b, "b")
        if a.shape != b.shape:
            raise ValueError(f"Diffusion.interpolate: a and b must have one shape (got {tuple(a.shape)} and {tuple(b.shape)})")
        try:
            w = np.asarray(weights.detach().cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
        except (TypeError, ValueError):
            w = None
        if w is None or w.ndim != 1 or w.size < 1 or not np.isfinite(w).all():
            raise ValueError("Diffusion.interpolate: weights must be a non-empty 1-D sequence of finite numbers")
        self._invert_moves(steps)
        if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
            raise ValueError(f"Diffusion.interpolate: refine must be an int >= 0 (got {refine!r})")
        n = a.shape[0]
        y = self._check_guidance("interpolate", model, n, labels, cfg_scale)
        lat = self.invert(model, torch.cat([a.to(self.device), b.to(self.device)]), steps, refine,
                          None if y is None else torch.cat([y, y]), cfg_scale, graph)
        mid = ops.slerp(lat[:n], lat[n:], weights)
        return self.decode(model, mid.reshape((n * w.size,) + tuple(lat.shape[1:])), steps, 0.0,
                           None if y is None else y.repeat_interleave(w.size), cfg_scale, graph=graph, return_float=return_float)

    # The model's own log-density: the probability-flow ODE with a Hutchinson trace (Song et al. 2021) ---------
    def eps_jacobian_coefficients(self, t):
        """(c1, c2), two fp64 host tensors of t's shape with eps = c1 x_t + c2 out, and so J_eps = d eps / d x_t = c1 I + c2 J_out,
        for `self.prediction` at the timesteps t: (0, 1) for "eps", (sqrt(1 - ah), sqrt(ah)) for "v" and (1 / sqrt(1 - ah),
        -sqrt(ah) / sqrt(1 - ah)) for "x0", ah the fp32 alpha_hat[t] widened to fp64.  The sibling of `x0_coefficients`."""
        ah = self.alpha_hat.detach().cpu().double()[torch.as_tensor(t).cpu().long()]
        sa, sb = torch.sqrt(ah), torch.sqrt(1.0 - ah)
        if self.prediction == "v":
            return sb, sa
        if self.prediction == "x0":
            return 1.0 / sb, -sa / sb
        return torch.zeros_like(ah), torch.ones_like(ah)

    def dequantize(self, images, noise_source="device"):
        """Uniform dequantisation of 8-bit images: `snap_8bit(images)` plus u / 127.5 with u uniform in [-0.5, 0.5), ONE
        torch.rand of the images' shape from the device generator (noise_source "device") or the CPU generator ("cpu", then
        copied); fp32 arithmetic.  Every value stays within half a level (1 / 255) of the snapped image.  Returns fp32 on the
        device."""
        snapped = self.snap_8bit(images).to(self.device)
        u = torch.rand(snapped.shape, device=self.device) if noise_source == "device" else torch.rand(snapped.shape).to(self.device)
        return (snapped + (u - 0.5) / 127.5).contiguous()

    def ode_likelihood(self, model, images, steps=100, method="heun", probes=1, probe="rademacher", labels=None, dequantize=False,
                       noise_source="device", return_latents=False):
        """The model's own log-density of `images` (Song et al. 2021, section 4.3: "NLL" from the probability-flow ODE), the
        counterpart of `calc_bpd`'s variational bound.  With a_t = alpha_hat[t] (level 0, the image, read as alpha_hat[0], as
        `invert` reads it), sig = sqrt((1 - a) / a) and y = x / sqrt(a) the ODE is dy / dsig = eps(x, t), DDIM is its Euler
        rule, and with d = C H W and U = taus[0] the top level
            log p_0(x_0) = log N(x_U; 0, I) + (d / 2) (log a_U - log a_0) + Integral_{sig_0}^{sig_U} sqrt(a) tr J_eps(x, t) dsig.
        tr J_eps is estimated by Hutchinson's v^T J_eps v = c1 |v|^2 + c2 v.w with w = J_out^T v, the network's input
        vector-Jacobian product (`_output_and_vjp`: one forward and one backward with the parameters frozen, no .grad written)
        and (c1, c2) of `eps_jacobian_coefficients`.
        images: fp32 (n, C, img_size, img_size) in [-1, 1].  steps: what `sample(steps=)` accepts, an int S (`ddim_timesteps`) or
        an explicit strictly decreasing sequence; the chain climbs [0] + reversed(taus) (`_invert_moves`).  With h = sig_u - sig_s:
          method="euler": `invert`'s move with refine = 0: evaluate at (x_s, u), x_u = ops.ddim_invert_step(x_s, eps, s, u),
            trace += h sqrt(a_u) tr J_eps(x_s, u).  One forward + backward per move and probe; the latents are `invert`'s.  It is a
            BASELINE, first order: on Gaussian data (d = 192, T = 1000) its log p is off by -0.62 / -0.32 / -0.160 / -0.080 nats per
            dimension at S = 25 / 50 / 100 / 200.  Do not quote a likelihood from it.
          method="heun" (the default), second order: the first move, out of level 0, is the Euler move (the network is never
            evaluated at t = 0); every later move evaluates eps_s, tr_s at (x_s, s), the predictor x~ = ddim_invert_step(x_s,
            eps_s, s, u), eps_u, tr_u at (x~, u), then x_u = sqrt(a_u) (x_s / sqrt(a_s) + h (eps_s + eps_u) / 2)
            (ops.ode_heun_step) and trace += h (sqrt(a_s) tr_s + sqrt(a_u) tr_u) / 2: two forward + backward pairs per move and
            probe.  On the same data: +0.088 / +0.021 / +0.0052 / +0.0013 nats per dimension at S = 25 / 50 / 100 / 200.
        probe: "rademacher" (+-1: |v|^2 = d exactly, and the estimate is exact whenever J is diagonal), "gaussian", or "basis": the
        d unit vectors, the exact trace at d backward passes per evaluation (`probes` is ignored) -- for small images and tests.
        probes: P >= 1, the probes per image, drawn once as (P, n, C, H, W) and fixed along the trajectory; each is one
        `_output_and_vjp` call per evaluation (no retain_graph), the state moves with the output of the first.  Each probe's
        integral is kept apart in an fp64 (P, n) accumulator on the device (ops.ode_trace_rows); nothing is read back before
        the end and the loop never synchronises.
        Draws, in this order, each ONE call from the device generator (noise_source "device") or the CPU generator ("cpu", then
        copied): with dequantize=True torch.rand((n, C, H, W)) (`dequantize`: the image is `snap_8bit`-ed and u / 127.5 added, u in
        [-0.5, 0.5)); then the probes, torch.randint(0, 2, (P, n, C, H, W)) * 2 - 1 for "rademacher", torch.randn of that shape for
        "gaussian", nothing for "basis".
        labels: class labels for a conditional model (log p(x | y)).  The model's mode, hint and requires_grad flags come back
        as they were found, also after an exception.
        Returns a dict of CPU fp64 (n,) tensors: logp (nats; the density of the float image at level 0), bpd = -logp / (d ln 2) +
        log2(127.5), prior_logp = log N(x_U; 0, I), trace (the integral; the mean over probes, their sum for "basis"), trace_sem
        (the standard error over probes; 0 for P = 1 and for "basis"); beside them trace_probes, fp64 (P, n), each probe's own integral,
        and with return_latents also latents, the fp32 x_U on the device.
        Not offered: classifier-free guidance (it would need the vector-Jacobian product of a 2n-row combination, as for
        `posterior_sample`), graph capture (autograd runs inside the step), adaptive step control, variance="learned"."""
        where = "ode_likelihood"
        from . import likelihood as lk
        if not (isinstance(method, str) and method in lk.METHODS):
            raise ValueError(f"Diffusion.{where}: unknown method {method!r} ('heun' or 'euler')")
        if not (isinstance(probe, str) and probe in lk.PROBES):
            raise ValueError(f"Diffusion.{where}: unknown probe {probe!r} ('rademacher', 'gaussian' or 'basis')")
        if isinstance(probes, bool) or not isinstance(probes, (int, np.integer)) or probes < 1:
            raise ValueError(f"Diffusion.{where}: probes must be an int >= 1 (got {probes!r})")
        if not (isinstance(noise_source, str) and noise_source in ("device", "cpu")):
            raise ValueError(f"Diffusion.{where}: noise_source must be 'device' or 'cpu' (got {noise_source!r})")
        if self.variance == "learned":
            raise ValueError(f"Diffusion.{where}: variance='learned' is not supported (the ODE's drift is the prediction alone)")
        self._check_images(where, images)
        try:
            moves = self._invert_moves(steps)
        except ValueError as e:
            raise ValueError(f"Diffusion.{where}: {str(e).removeprefix('Diffusion: ')}") from None
        n, C = int(images.shape[0]), int(images.shape[1])
        shape = tuple(images.shape[1:])
        d = int(np.prod(shape))
        if labels is not None:
            labels = self._check_labels(model, n, None, labels, where)
        self.check_model(model, C, f"Diffusion.{where}")
        logging.info(f"Integrating the probability-flow ODE of {n} images....")

        levels = [0] + [u for _, u in moves]
        a, sig = lk.sigma_levels(self.alpha_hat, levels)
        c1s, c2s = (c.tolist() for c in self.eps_jacobian_coefficients(levels))
        dev = self.device
        x = self.dequantize(images, noise_source) if dequantize else images.to(dev).contiguous().clone()
        v = lk.draw_probes(probe, probes, n, shape, dev if noise_source == "device" else None).to(dev).contiguous()
        P = int(v.shape[0])
        acc = torch.zeros(P, n, device=dev, dtype=torch.float64)
        prior = torch.zeros(n, device=dev, dtype=torch.float64)

        def evaluate(xs, k, weight):
            """eps at (xs, levels[k]) from the first probe's forward; weight * (c1 |v|^2 + c2 v.w) of every probe goes into acc."""
            t_rows = self._t_full(n, levels[k], dev)
            first = None
            for p in range(P):
                out, w = self._output_and_vjp(model, xs, t_rows, labels, lambda o, p=p: v[p])
                ops.ode_trace_rows(v[p], w, weight * c1s[k], weight * c2s[k], acc[p])
                first = out if first is None else first
            if self.prediction == "eps":
                return first
            return ops.pred_to_eps(first, xs, t_rows, self.alpha_hat, self.prediction, eps_out=first)

        with self._model_scope(model, leave_training=False):
            pred = torch.empty_like(x)
            for k, (s, u) in enumerate(moves):
                h = sig[k + 1] - sig[k]
                if method == "euler" or s == 0:
                    eps = evaluate(x, k + 1, h * math.sqrt(a[k + 1]))
                    ops.ddim_invert_step(x, eps, self.alpha_hat, s, u, x)
                    continue
                eps_s = evaluate(x, k, 0.5 * h * math.sqrt(a[k]))
                ops.ddim_invert_step(x, eps_s, self.alpha_hat, s, u, pred)
                eps_u = evaluate(pred, k + 1, 0.5 * h * math.sqrt(a[k + 1]))
                ops.ode_heun_step(x, eps_s, eps_u, self.alpha_hat, s, u, x)
            ops.ode_trace_rows(x, None, -0.5, 0.0, prior)

        tr = acc.cpu()
        prior_logp = prior.cpu() - 0.5 * d * math.log(2.0 * math.pi)
        if probe == "basis":
            trace, sem = tr.sum(0), torch.zeros(n, dtype=torch.float64)
        else:
            trace = tr.mean(0)
            sem = tr.std(0, unbiased=True) / math.sqrt(P) if P > 1 else torch.zeros(n, dtype=torch.float64)
        logp = prior_logp + 0.5 * d * (math.log(a[-1]) - math.log(a[0])) + trace
        res = {"logp": logp, "bpd": lk.bpd_from_logp(logp, d), "prior_logp": prior_logp, "trace": trace, "trace_sem": sem,
               "trace_probes": tr}
        if return_latents:
            res["latents"] = x
        return res

    @staticmethod
    def _capture(one_step, xs):
        """Capture one_step (which updates xs in place) into a hipGraph, after a warm-up on a side stream whose effect on xs
        and on the device generator is undone: the replays consume the noise stream the eager loop would."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        keep = xs.clone()
        rng = torch.cuda.get_rng_state(xs.device)
        with torch.cuda.stream(side):
            one_step()
        torch.cuda.current_stream().wait_stream(side)
        xs.copy_(keep)
        torch.cuda.set_rng_state(rng, xs.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one_step()
        return g

    # Likelihood: the variational bound in bits per dimension (Ho et al. 2020, section 3.3) -----------------------------------
    VLB_SIGMAS = ("beta", "posterior")           # (calc_bpd also takes "learned" on a learned-variance process)

    def vlb_coefficients(self, sigma="beta"):
        """(T, 4) fp64 host table of the bound's coefficients, from the fp32 schedule tables widened to fp64.  Row t (1 <= t < T)
        = [w_t, c_t, log_scale_t, prior], row 0 is zeros except the prior column:
          beta~_t = (1 - ah[t-1]) / (1 - ah[t]) * beta[t];  s2 = beta[t] (sigma="beta") or beta~_t (sigma="posterior")
          w_t = beta[t]^2 / (2 s2 alpha[t] (1 - ah[t]))       (the KL term per unit of sum (eps_hat - eps)^2)
          c_t = (-1 + log(s2 / beta~_t) + beta~_t / s2) / 2   (per element; exactly 0 for "posterior", computed without
                                                                cancellation for "beta": (u - log1p(u)) / 2, u = beta~_t / s2 - 1)
          log_scale_t = log(s2) / 2                            (the decoder's at t = 1)
          prior = (-1 - log(1 - ah[T-1]) + (1 - ah[T-1])) / 2  (per element, the same in every row).
        sigma may also be an `AnalyticVariance` with an estimate at every t in 1 .. T - 1: s2 = its sigma*2(t, t - 1) at eta = 1
        (Analytic-DDPM, whose mean is the posterior's), and w_t, c_t, log_scale_t by the same formulas, c_t as (u - log1p(u)) / 2."""
        analytic = isinstance(sigma, AnalyticVariance)
        if not analytic and (not isinstance(sigma, str) or sigma not in self.VLB_SIGMAS):
            raise ValueError(f"Diffusion.vlb_coefficients: unknown sigma {sigma!r} ('beta' or 'posterior')")
        T = self.noise_steps
        if T < 2:
            raise ValueError(f"Diffusion.vlb_coefficients: needs noise_steps >= 2 (got {T})")
        s2_av = sigma.sigma2(self, [(t, t - 1) for t in range(1, T)], 1.0) if analytic else None
        b = self.beta.detach().cpu().double().numpy()
        a = self.alpha.detach().cpu().double().numpy()
        ah = self.alpha_hat.detach().cpu().double().numpy()
        om = 1.0 - ah                                            # exact: 1 - an fp32 value in [0, 1] fits an fp64
        tab = np.zeros((T, 4), dtype=np.float64)
        for t in range(1, T):
            bt = om[t - 1] / om[t] * b[t]
            s2 = s2_av[t - 1] if analytic else (b[t] if sigma == "beta" else bt)
            tab[t, 0] = b[t] * b[t] / (2.0 * s2 * a[t] * om[t])
            if analytic or sigma == "beta":                     # beta~ / beta - 1 = (ah[t] - ah[t-1]) / (1 - ah[t])
                u = (bt - s2) / s2 if analytic else (ah[t] - ah[t - 1]) / om[t]
                if abs(u) < 0.1:
                    tab[t, 1] = 0.5 * sum((-u) ** k / k for k in range(2, 40))     # u - log1p(u), summed from its series
                else:
                    tab[t, 1] = 0.5 * (u - math.log1p(u))
            tab[t, 2] = 0.5 * math.log(s2)
        tab[:, 3] = 0.5 * (-1.0 - math.log(om[T - 1]) + om[T - 1])
        return torch.from_numpy(tab)

    @staticmethod
    def snap_8bit(images):
        """The 8-bit image the bound is evaluated on, as fp32 on the host: uint8 k -> k / 127.5 - 1; float x ->
        k = round((x + 1) * 127.5) (half to even) clamped to 0 .. 255, then k / 127.5 - 1 (fp32 arithmetic throughout)."""
        x = images.detach().cpu()
        if x.dtype == torch.uint8:
            k = x.float()
        else:
            k = torch.round((x.float() + 1.0) * 127.5).clamp_(0.0, 255.0)
        return k / 127.5 - 1.0

    def bpd_timesteps(self, n, t_samples=None, noise_source="device"):
        """The timesteps of each of n images, each list descending: T-1 .. 1 for the full bound (t_samples None or T - 1);
        otherwise K = t_samples distinct values drawn per image, uniformly without replacement from [1, T-1], by one
        torch.randperm(T - 1) per image from the device generator (noise_source "device") or the CPU generator ("cpu")."""
        T = self.noise_steps
        K = T - 1 if t_samples is None else t_samples
        if K == T - 1:
            return [list(range(T - 1, 0, -1)) for _ in range(n)]
        out = []
        for _ in range(n):
            p = torch.randperm(T - 1, device=self.device) if noise_source == "device" else torch.randperm(T - 1)
            out.append(sorted((int(v) + 1 for v in p[:K].cpu()), reverse=True))
        return out

    @staticmethod
    def bpd_rows(timesteps):
        """The rows of the bound loop, image-major in the order of each image's timesteps -> (img, t), two int64 arrays."""
        img = np.concatenate([np.full(len(ts), i, dtype=np.int64) for i, ts in enumerate(timesteps)])
        t = np.concatenate([np.asarray(ts, dtype=np.int64) for ts in timesteps])
        return img, t

    @staticmethod
    def bpd_chunks(rows, batch):
        """The [lo, hi) row ranges of the forwards: consecutive chunks of `batch` rows, the last one shorter."""
        return [(lo, min(rows, lo + batch)) for lo in range(0, rows, batch)]

    def bpd_combine(self, n, per, img, t, term, sq, prior, K, return_terms=False):
        """Per-image parts from the rows' terms (fp64 host arrays, nats) -> the dict `calc_bpd` returns.  prior: (n,) nats.
        The terms of the K evaluated timesteps of an image are scaled by (T - 1) / K (1 for the full bound)."""
        T = self.noise_steps
        scale = (T - 1) / K
        norm = per * math.log(2.0)
        dec = t == 1
        vb = np.bincount(img[~dec], weights=term[~dec], minlength=n) * scale
        dd = np.bincount(img[dec], weights=term[dec], minlength=n) * scale
        prior = np.asarray(prior, dtype=np.float64)
        out = {"bpd": (prior + vb + dd) / norm, "prior_bpd": prior / norm, "vb_bpd": vb / norm, "decoder_bpd": dd / norm}
        if return_terms:
            terms = np.zeros((n, T))
            mse = np.zeros((n, T))
            terms[img, t] = term
            mse[img, t] = sq / per
            out["terms"], out["mse"] = terms, mse
        return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)) for k, v in out.items()}

    def _bpd_images(self, model, images):
        """Validated, snapped images -> fp32 (n, C, img_size, img_size) host tensor."""
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] < 1:
            raise ValueError("Diffusion.calc_bpd: images must be an (n, C, H, W) tensor with n >= 1")
        C = next((p.shape[1] for p in model.inc.parameters() if p.dim() == 4), None) if hasattr(model, "inc") else None
        size = getattr(model, "image_size", self.img_size)
        if tuple(images.shape[2:]) != (self.img_size, self.img_size) or size != self.img_size or (C is not None and images.shape[1] != C):
            raise ValueError(f"Diffusion.calc_bpd: images of shape {tuple(images.shape)} do not match the model "
                             f"({C if C is not None else 'C'} channels, {size} x {size}) and img_size {self.img_size}")
        if images.dtype != torch.uint8:
            if not images.dtype.is_floating_point:
                raise ValueError(f"Diffusion.calc_bpd: images must be float in [-1, 1] or uint8 (got {images.dtype})")
            x = images.detach()
            if not bool(((x >= -1.0 - 1e-5) & (x <= 1.0 + 1e-5)).all()):
                raise ValueError("Diffusion.calc_bpd: float images must lie in [-1, 1]")
        return self.snap_8bit(images)

    def calc_bpd(self, model, images, labels=None, sigma="beta", t_samples=None, batch=256, noise_source="device", noise_fn=None,
                 return_terms=False):
        """Negative log-likelihood bound of `images` under `model`, in bits per dimension (Ho et al. 2020, section 3.3;
        Nichol & Dhariwal's calc_bpd_loop): prior + sum_{t=2}^{T-1} L_t + L_1, over D ln 2 with D = C * H * W.
        images: (n, C, img_size, img_size), float in [-1, 1] or uint8.  Float values are snapped once to the nearest of the
        256 levels (`snap_8bit`): the result is the likelihood of that 8-bit image, not of the float one.
        prior = KL(q(x_{T-1} | x0) || N(0, I)); L_t = KL(q(x_{t-1} | x_t, x0) || p(x_{t-1} | x_t)) with variance s2 from
        sigma ("beta": beta_t, what the sampler draws; "posterior": beta~_t; an `AnalyticVariance` with an estimate at every t:
        the optimal sigma*2(t, t - 1) of Analytic-DPM, which tightens the bound); L_1 = -log p(x0 | x_1), the discretised
        Gaussian around the image the sampler returns.  Coefficients: `vlb_coefficients`.
        Rows (image, t) are image-major, t descending within an image (`bpd_rows`), and go to the model in chunks of `batch`
        (`bpd_chunks`), one forward per chunk with per-row t.  Each chunk draws its noise, (rows, C, H, W), from the device
        generator (noise_source "device"), the CPU generator ("cpu", then copied), or noise_fn(shape) when given.
        t_samples = K < T - 1: K timesteps per image (`bpd_timesteps`, drawn before any noise) and the unbiased estimate
        prior + (T - 1) / K * sum_k L_{t_k}; None (or T - 1): the full bound, T - 1 rows per image.
        labels: (n,) int64 class labels for a UNet(num_classes=K): the bound of log p(x | y); NULL_LABEL rows give the
        unconditional bound.  Returns a dict of CPU fp64 (n,) tensors bpd, prior_bpd, vb_bpd (the KL terms), decoder_bpd
        (bpd is their sum); with return_terms also terms (n, T), nats per t (0 where not evaluated; unscaled), and mse (n, T),
        the per-element mean of (eps_hat - eps)^2.
        sigma="learned" (needs variance="learned"): the per-pixel variance the network emits, in L_t and in the decoder
        (`ops.vlb_terms_lvar`, the terms the hybrid loss trains on).  "beta" / "posterior" on a learned-variance process score its
        prediction half with those fixed variances."""
        T = self.noise_steps
        if T < 3:
            raise ValueError(f"Diffusion.calc_bpd: needs noise_steps >= 3 (got {T})")
        learned = isinstance(sigma, str) and sigma == "learned"
        if learned and self.variance != "learned":
            raise ValueError(f"Diffusion.calc_bpd: unknown sigma 'learned' for a process with variance={self.variance!r} ('beta' or "
                             "'posterior'; 'learned' needs Diffusion(variance='learned'))")
        coef = self.vlb_coefficients("beta" if learned else sigma)           # (the prior column does not depend on sigma; an
        #                                                                      AnalyticVariance is checked there, before any launch)
        if t_samples is not None and (isinstance(t_samples, bool) or not isinstance(t_samples, (int, np.integer))
                                      or not 1 <= t_samples <= T - 1):
            raise ValueError(f"Diffusion.calc_bpd: t_samples must be an int in [1, {T - 1}] or None (got {t_samples!r})")
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"Diffusion.calc_bpd: batch must be a positive int (got {batch!r})")
        if noise_source not in ("device", "cpu"):
            raise ValueError(f"Diffusion.calc_bpd: noise_source must be 'device' or 'cpu' (got {noise_source!r})")
        x0 = self._bpd_images(model, images)
        self.check_model(model, images.shape[1], "Diffusion.calc_bpd")
        n, shape = x0.shape[0], tuple(x0.shape[1:])
        per = int(np.prod(shape))
        y = None if labels is None else self._check_labels(model, n, None, labels, "calc_bpd")
        K = T - 1 if t_samples is None else int(t_samples)

        timesteps = self.bpd_timesteps(n, K, noise_source)
        img, t = self.bpd_rows(timesteps)
        assert img.min() >= 0 and img.max() < n and t.min() >= 1 and t.max() < T     # the kernels read them unchecked
        dev = self.device
        x0 = x0.to(dev).contiguous()
        img_d, t_d = torch.from_numpy(img).to(dev), torch.from_numpy(t).to(dev)
        y_rows = None if y is None else y[img_d]
        coef_d = coef.to(dev)
        term = torch.empty(len(t), device=dev, dtype=torch.float64)
        sq = torch.empty_like(term)
        prior = ops.vlb_prior(x0, 0.5 * float(self.alpha_hat[T - 1]))
        with self._model_scope(model, leave_training=False):
            for lo, hi in self.bpd_chunks(len(t), batch):
                eps = self._chunk_noise((hi - lo,) + shape, noise_source, noise_fn)
                rows_i, rows_t = img_d[lo:hi], t_d[lo:hi]
                xt = ops.noise_images_gather(x0, rows_i, eps, rows_t, self.alpha_hat, check_range=False)
                if learned:
                    out2 = self._raw_output(model, xt, rows_t, None if y_rows is None else y_rows[lo:hi])
                    ops.vlb_terms_lvar(x0, rows_i, xt, eps, out2, rows_t, self._lv(), self.alpha, self.alpha_hat, self.beta,
                                       self.prediction, term[lo:hi], sq[lo:hi], check_range=False)
                    continue
                eh = self.predict_eps(model, xt, rows_t, None if y_rows is None else y_rows[lo:hi])
                ops.vlb_terms(x0, rows_i, xt, eps, eh.contiguous(), rows_t, coef_d, self.alpha, self.alpha_hat, self.beta,
                              term[lo:hi], sq[lo:hi], check_range=False)
        prior_nats = prior.cpu().numpy() + per * float(coef[0, 3])
        return self.bpd_combine(n, per, img, t, term.cpu().numpy(), sq.cpu().numpy(), prior_nats, K, return_terms)

    # Analytic-DPM (Bao et al. 2022): the statistic of the optimal reverse variance ------------------------------------------------
    def estimate_analytic_variance(self, model, images, timesteps=None, rows_per_step=64, batch=256, labels=None, cfg_scale=0.0,
                                   noise_source="device", noise_fn=None):
        """Monte-Carlo estimate of G_t = E|eps_theta(x_t, t)|^2 / d over `images` -> an `AnalyticVariance` (analytic.py) with an
        estimate at every timestep of `timesteps`: None = 1 .. T - 1, an int S = `ddim_timesteps(S)`, or a sequence of ints in
        [1, T - 1] taken as given.  images: (N, C, img_size, img_size), uint8 pixels (k -> k / 127.5 - 1) or float values, used
        as they are (nothing is snapped or clipped), or a `DeviceDataset`.
        Rows are timestep-major: timestep k takes the rows [k rows_per_step, (k + 1) rows_per_step), and row r reads image
        r mod N, so the images are cycled through.  The rows go to the model in chunks of `batch` with per-row t, as in `calc_bpd`:
        each chunk draws its noise (`_chunk_noise`: the device generator, the CPU generator, or noise_fn(shape)), is noised by one
        gather launch and goes through `predict_eps` (a v- or x0-model's output is converted; of a learned-variance model the
        prediction half is read); one ops.eps_sqnorm_rows launch per chunk leaves the rows' fp64 sums on the device, read back
        once at the end and folded into per-timestep means with np.bincount in fp64.
        labels: (N,) int64 class labels, one per image, for a UNet(num_classes=K): the table of the conditional eps; with
        cfg_scale > 0 each chunk is one forward over 2B rows [x_t ; x_t] with labels [y ; NULL_LABEL] and the table is that of
        the guided eps = lerp(eps_uncond, eps_cond, cfg_scale), what `sample(labels=, cfg_scale=)` steps with.
        The model's mode and timestep hint come back as they were found."""
        T = self.noise_steps
        where = "Diffusion.estimate_analytic_variance"
        if timesteps is None:
            ts = list(range(1, T))
        elif isinstance(timesteps, (int, np.integer)) and not isinstance(timesteps, bool):
            ts = self.ddim_timesteps(timesteps)
        else:
            try:
                ts = list(timesteps)
            except TypeError:
                raise ValueError(f"{where}: timesteps must be None, an int or a sequence of ints") from None
            if not ts or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= T - 1 for v in ts):
                raise ValueError(f"{where}: timesteps must be a non-empty sequence of ints in [1, {T - 1}]")
            ts = [int(v) for v in ts]
        for name, v in (("rows_per_step", rows_per_step), ("batch", batch)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"{where}: {name} must be a positive int (got {v!r})")
        if noise_source not in ("device", "cpu"):
            raise ValueError(f"{where}: noise_source must be 'device' or 'cpu' (got {noise_source!r})")
        rows = len(ts) * int(rows_per_step)
        from .data import DeviceDataset
        if isinstance(images, DeviceDataset):
            N = len(images)
            x0 = images.batch(torch.arange(min(N, rows), device=images.device))[0]
        else:
            if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] < 1 or \
                    not (images.dtype == torch.uint8 or images.dtype.is_floating_point):
                raise ValueError(f"{where}: images must be an (N, C, H, W) uint8 or float tensor with N >= 1, or a DeviceDataset")
            N = images.shape[0]
            x0 = images[:min(N, rows)].detach()
            x0 = x0.float() / 127.5 - 1.0 if x0.dtype == torch.uint8 else x0.float()
        if tuple(x0.shape[2:]) != (self.img_size, self.img_size):
            raise ValueError(f"{where}: images of shape {tuple(x0.shape)} do not match img_size {self.img_size}")
        y = None if labels is None else self._check_labels(model, N, None, labels, "estimate_analytic_variance")
        if y is None and cfg_scale:
            raise ValueError(f"{where}: cfg_scale needs class labels")
        self.check_model(model, x0.shape[1], where)
        shape = tuple(x0.shape[1:])
        per = int(np.prod(shape))
        t = np.repeat(np.asarray(ts, dtype=np.int64), int(rows_per_step))
        img = np.arange(rows, dtype=np.int64) % N
        dev = self.device
        x0 = x0.to(dev).contiguous()
        img_d, t_d = torch.from_numpy(img).to(dev), torch.from_numpy(t).to(dev)
        y_rows = None if y is None else y[img_d]
        guided = y is not None and cfg_scale > 0
        sums = torch.empty(rows, device=dev, dtype=torch.float64)
        with self._model_scope(model, leave_training=False):
            for lo, hi in self.bpd_chunks(rows, int(batch)):
                eps = self._chunk_noise((hi - lo,) + shape, noise_source, noise_fn)
                rows_t = t_d[lo:hi]
                xt = ops.noise_images_gather(x0, img_d[lo:hi], eps, rows_t, self.alpha_hat, check_range=False)
                if guided:
                    yc = y_rows[lo:hi]
                    eh = self.predict_eps(model, torch.cat([xt, xt]), torch.cat([rows_t, rows_t]),
                                          torch.cat([yc, torch.full_like(yc, ops.NULL_LABEL)]))
                    ops.eps_sqnorm_rows(eh, float(cfg_scale), out=sums[lo:hi])
                else:
                    eh = self.predict_eps(model, xt, rows_t, None if y_rows is None else y_rows[lo:hi])
                    ops.eps_sqnorm_rows(eh, out=sums[lo:hi])
        sums = sums.cpu().numpy()
        count = np.bincount(t, minlength=T).astype(np.int64)
        total = np.bincount(t, weights=sums, minlength=T)
        gamma = np.full(T, np.nan, dtype=np.float64)
        hit = count > 0
        gamma[hit] = total[hit] / (count[hit].astype(np.float64) * per)
        return AnalyticVariance(gamma, count, T, self.schedule, self.prediction, self.alpha_hat)

    # Equivariance scores: EQ-T / EQ-R of Karras et al. 2021 (StyleGAN3, section 2 and appendix E) for eps_theta -------------
    EQ_KINDS = ("translate", "rotate")

    def equivariance_transforms(self, specs):
        """(K, 6) fp64 host table of affine maps in scipy's convention, out[o] = spline3(in)(M o + off) per (img_size, img_size)
        plane with periodic wrap, row k = [m00, m01, m10, m11, off0, off1] in (row, col) order, from a list of specs:
          ("translate", dy, dx): M = I, off = (-dy, -dx): the content moves down by dy and right by dx, as ndimage.shift does
                                 (whole or fractional pixels);
          ("rotate", degrees):   the M and off `ops.rotate_spline3_wrap` builds (ndimage.rotate, reshape=False)."""
        if isinstance(specs, (str, bytes)) or not hasattr(specs, "__len__") or len(specs) == 0:
            raise ValueError("Diffusion.equivariance_transforms: needs a non-empty list of ('translate', dy, dx) / ('rotate', degrees)")
        S = self.img_size
        tab = np.zeros((len(specs), 6), dtype=np.float64)
        for i, sp in enumerate(specs):
            if isinstance(sp, (str, bytes)) or not hasattr(sp, "__len__") or len(sp) == 0 or not isinstance(sp[0], str) \
                    or sp[0] not in self.EQ_KINDS:
                raise ValueError(f"Diffusion.equivariance_transforms: unknown transform {sp!r} ('translate' or 'rotate')")
            want = 2 if sp[0] == "translate" else 1
            try:
                v = [float(a) for a in sp[1:]]
            except (TypeError, ValueError):
                v = None
            if v is None or len(v) != want or any(isinstance(a, bool) for a in sp[1:]) or not all(math.isfinite(a) for a in v):
                raise ValueError(f"Diffusion.equivariance_transforms: {sp!r} needs {want} finite number(s) after the kind")
            if sp[0] == "translate":
                tab[i] = [1.0, 0.0, 0.0, 1.0, -v[0], -v[1]]
            else:
                m, off = ops.rotate_affine(v[0], S, S)
                tab[i] = [m[0, 0], m[0, 1], m[1, 0], m[1, 1], off[0], off[1]]
        return torch.from_numpy(tab)

    @staticmethod
    def equivariance_mask(affine_row, H, W, margin):
        """The validity mask of one transform, a bool (H, W) numpy array: output pixel o = (oy, ox) counts iff o and its source
        c = M o + off, taken before any wrapping, both lie in [margin, H-1-margin] x [margin, W-1-margin].  It drops what the
        wrap would bring in from the other side and a border band (the UNet's zero-padded convolutions are not equivariant
        there).  c is evaluated in fp64 as (m_0 oy + m_1 ox) + off, every operation rounded, as `afd_eq_terms` does."""
        a = np.asarray(affine_row, dtype=np.float64).reshape(6)
        m = float(margin)
        oy, ox = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        cy = (a[0] * oy + a[1] * ox) + a[4]
        cx = (a[2] * oy + a[3] * ox) + a[5]
        hy, hx = float(H - 1) - m, float(W - 1) - m
        return (oy >= m) & (oy <= hy) & (ox >= m) & (ox <= hx) & (cy >= m) & (cy <= hy) & (cx >= m) & (cx <= hx)

    @staticmethod
    def equivariance_rows(n, J, K):
        """The rows of the transformed pass, image-major, then timestep, then transform -> (img, j, k), three int64 arrays of
        n * J * K values.  Row r compares source field img[r] * J + j[r] (one per image and timestep) under transform k[r]."""
        r = np.arange(n * J * K, dtype=np.int64)
        return r // (J * K), (r // K) % J, r % K

    @staticmethod
    def equivariance_combine(n, J, K, C, sums, peak=2.0):
        """The rows' sums [sum d^2, sum ref^2, masked pixels * C] ((n * J * K, 3) fp64, `equivariance_rows` order) -> the dict
        `equivariance` returns: mse, power (n, J, K): the sums over C * count; count (K,): masked pixels per transform;
        eq_db (J, K) = 10 log10(peak^2 / mean_i mse); snr_db (J, K) = 10 log10(mean_i power / mean_i mse); +inf where the mean
        mse is 0."""
        s = np.asarray(sums, dtype=np.float64).reshape(n, J, K, 3)
        elems = s[..., 2]
        if not (elems > 0).all() or not (elems == elems[:1, :1]).all():
            raise ValueError("Diffusion.equivariance_combine: every row of a transform must count the same, non-zero number of elements")
        mse, power = s[..., 0] / elems, s[..., 1] / elems
        m, pw = mse.mean(axis=0), power.mean(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            eq = np.where(m == 0, np.inf, 10.0 * np.log10(float(peak) ** 2 / m))
            snr = np.where(m == 0, np.inf, 10.0 * np.log10(pw / m))
        out = {"mse": mse, "power": power, "eq_db": eq, "snr_db": snr, "count": elems[0, 0] / C}
        return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)) for k, v in out.items()}

    def _equivariance_images(self, model, images):
        if not isinstance(images, torch.Tensor) or images.dtype != torch.float32:
            raise ValueError("Diffusion.equivariance: images must be an fp32 tensor")
        if images.dim() != 4 or images.shape[0] < 1 or tuple(images.shape[2:]) != (self.img_size, self.img_size):
            raise ValueError(f"Diffusion.equivariance: images must have shape (n, C, {self.img_size}, {self.img_size}) "
                             f"(got {tuple(images.shape)})")
        C = next((p.shape[1] for p in model.inc.parameters() if p.dim() == 4), None) if hasattr(model, "inc") else None
        size = getattr(model, "image_size", self.img_size)
        if size != self.img_size or (C is not None and images.shape[1] != C):
            raise ValueError(f"Diffusion.equivariance: images of shape {tuple(images.shape)} do not match the model "
                             f"({C if C is not None else 'C'} channels, {size} x {size})")
        return images.detach()

    def equivariance(self, model, images, t, transforms, margin=4.0, peak=2.0, labels=None, batch=256, noise_source="device",
                     noise_fn=None):
        """How equivariant eps_theta is, in dB (EQ-T / EQ-R of Karras et al. 2021): the PSNR between "transform the input, then
        run the model" and "run the model, then transform the output".  images: (n, C, img_size, img_size) fp32; t: an int or a
        sequence of J ints in [1, T-1]; transforms: a list of K specs (`equivariance_transforms`).  For image i, timestep t_j and
        transform S_k, with one noise eps_ij shared by every k:
          x = noise_images(x0_i, t_j, eps_ij);  g = model(S_k x, t_j), S_k x rounded once to fp32;  r = S_k model(x, t_j) in fp64
          mse[i, j, k] = sum_mask (g - r)^2 / (C count_k),  power[i, j, k] = sum_mask r^2 / (C count_k)
        over the transform's validity mask for `margin` pixels (`equivariance_mask`; an empty mask is a ValueError).
        First pass: the n * J base rows (image-major), in chunks of `batch` (`bpd_chunks`), one forward per chunk with per-row
        t; each chunk draws its noise, (rows, C, H, W), from the device generator (noise_source "device"), the CPU generator
        ("cpu") or noise_fn(shape); x and the model's output are prefiltered once into fp64 spline coefficients.  Second pass:
        the n * J * K rows (`equivariance_rows`) in chunks of `batch`: one row-wise resampling of x, one forward, one fused
        comparison (`ops.eq_terms`).  labels: (n,) int64 for a UNet(num_classes=).  Returns a dict of CPU fp64 tensors: mse,
        power (n, J, K), eq_db = 10 log10(peak^2 / mean_i mse) and snr_db = 10 log10(mean_i power / mean_i mse) (J, K), and
        count (K,).  peak = 2 is StyleGAN3's I_max, the range of x0 in [-1, 1]; snr_db assumes no range.  Fractional shifts and
        rotations resample with a cubic spline, a mild low-pass: compare scores under the same transforms only.
        The score is of the network's raw output, whatever `prediction` says it means (eps, v or x0): it does not go through
        `predict_eps`, whose x_t term would add a trivially equivariant part.  With variance="learned" it is the score of the
        output's prediction half."""
        T = self.noise_steps
        ts = [t] if isinstance(t, (int, np.integer)) and not isinstance(t, bool) else t
        if isinstance(ts, (str, bytes, bool)) or not hasattr(ts, "__len__") or len(ts) == 0 or \
                any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= T - 1 for v in ts):
            raise ValueError(f"Diffusion.equivariance: t must be an int or a non-empty sequence of ints in [1, {T - 1}] (got {t!r})")
        ts = [int(v) for v in ts]
        aff = self.equivariance_transforms(transforms)
        for name, v, ok in (("margin", margin, lambda a: a >= 0), ("peak", peak, lambda a: a > 0)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not ok(v):
                raise ValueError(f"Diffusion.equivariance: {name} must be a finite number {'>= 0' if name == 'margin' else '> 0'} (got {v!r})")
        if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
            raise ValueError(f"Diffusion.equivariance: batch must be a positive int (got {batch!r})")
        if noise_source not in ("device", "cpu"):
            raise ValueError(f"Diffusion.equivariance: noise_source must be 'device' or 'cpu' (got {noise_source!r})")
        x0 = self._equivariance_images(model, images)
        n, shape = x0.shape[0], tuple(x0.shape[1:])
        C, S = shape[0], self.img_size
        for k_, row in enumerate(aff.numpy()):
            if not self.equivariance_mask(row, S, S, margin).any():
                raise ValueError(f"Diffusion.equivariance: transform {k_} ({transforms[k_]!r}) leaves no pixel inside the margin "
                                 f"of {margin} on {S} x {S}")
        y = None if labels is None else self._check_labels(model, n, None, labels, "equivariance")
        J, K = len(ts), aff.shape[0]

        img, j, k = self.equivariance_rows(n, J, K)
        src = img * J + j                                                  # the source field of each transformed row
        src0 = np.arange(n * J, dtype=np.int64)                            # base rows: (image, t_j), image-major
        assert src.min() >= 0 and src.max() < n * J and k.min() >= 0 and k.max() < K       # the kernels read them unchecked
        dev = self.device
        x0 = x0.to(dev).contiguous()
        t_host = np.asarray(ts, dtype=np.int64)
        img0_d, t0_d = torch.from_numpy(src0 // J).to(dev), torch.from_numpy(t_host[src0 % J]).to(dev)
        src_d, k_d, t_d = torch.from_numpy(src).to(dev), torch.from_numpy(k).to(dev), torch.from_numpy(t_host[j]).to(dev)
        aff_d = aff.to(dev)
        coef_x = torch.empty((n * J,) + shape, device=dev, dtype=torch.float64)
        coef_f = torch.empty_like(coef_x)
        sums = torch.empty((len(k), 3), device=dev, dtype=torch.float64)
        with self._model_scope(model, leave_training=False):
            for lo, hi in self.bpd_chunks(n * J, batch):
                eps = self._chunk_noise((hi - lo,) + shape, noise_source, noise_fn)
                rows_t = t0_d[lo:hi]
                xt = ops.noise_images_gather(x0, img0_d[lo:hi], eps, rows_t, self.alpha_hat, check_range=False)
                f = model(xt, rows_t) if y is None else model(xt, rows_t, y[img0_d[lo:hi]])
                f = f[:, :C] if self.variance == "learned" else f             # the prediction half
                ops.spline3_prefilter_wrap(xt, coef_x[lo:hi])
                ops.spline3_prefilter_wrap(f.contiguous(), coef_f[lo:hi])
            for lo, hi in self.bpd_chunks(len(k), batch):
                rows_s, rows_k, rows_t = src_d[lo:hi], k_d[lo:hi], t_d[lo:hi]
                sx = ops.affine_spline3_wrap_rows(coef_x, rows_s, aff_d, rows_k, check_range=False)
                g = model(sx, rows_t) if y is None else model(sx, rows_t, y[rows_s // J])
                g = g[:, :C] if self.variance == "learned" else g
                ops.eq_terms(coef_f, rows_s, aff_d, rows_k, g.contiguous(), margin, sums[lo:hi], check_range=False)
        return self.equivariance_combine(n, J, K, C, sums.cpu().numpy(), peak)

    def sample_sharded(self, model, n, image_channels, theta=None, noise_source="reference", group=None, dst=0, steps=None):
        """`sample` with the n images partitioned over the ranks of `group` (sampling is embarrassingly parallel per
        image: replicas only, no collective in the loop) and the uint8 results gathered on rank `dst`.
        Every rank must have been seeded alike (as the reference's scripts do with set_seed): each rank draws the noise
        of ALL n images from the same generator stream and keeps its rows, so the gathered (x, result) equal what one rank
        computes for the same seed -- whatever the world size.  Returns (x_u8, result_u8) on `dst`, (None, None) elsewhere;
        without an initialised process group it is `sample`.  DDIM (steps=) is not supported here: use `sample`."""
        if steps is not None:
            raise NotImplementedError("Diffusion.sample_sharded: DDIM (steps=) is not supported; use sample or sample_concurrent")
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            return self.sample(model, n, image_channels, theta=theta, noise_source=noise_source)
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        lo, hi = shard_range(n, rank, world)
        x, snaps = self._loop(model, n, image_channels, theta, noise_source, None, shard=(lo, hi))
        counts = [shard_range(n, r, world)[1] - shard_range(n, r, world)[0] for r in range(world)]
        xq = gather_u8(ops.quantize_u8(x) if hi > lo else torch.empty((0,) + tuple(x.shape[1:]), dtype=torch.uint8, device=x.device),
                       counts, group, dst)
        # result = cat(snapshots): (S * n_r, ...) on each rank -> (S, n, ...) snapshot-major like `sample`
        S = len(snaps)
        rq_local = ops.quantize_u8(torch.cat(snaps)) if hi > lo else torch.empty((0,) + tuple(x.shape[1:]), dtype=torch.uint8, device=x.device)
        rq = gather_u8(rq_local, [S * c for c in counts], group, dst)
        if rank != dst:
            return None, None
        offs = np.cumsum([0] + [S * c for c in counts])
        per_rank = [rq[offs[r]:offs[r + 1]].reshape(S, counts[r], *rq.shape[1:]) for r in range(world)]
        return xq, torch.cat(per_rank, dim=1).reshape(S * n, *rq.shape[1:])

    def sample_rotation_sweep_sharded(self, model, n, image_channels, thetas, group=None, dst=0, steps=None):
        """Config E sweep (ddpm_tasks.py:346-369) with the ANGLES partitioned over the ranks (BASELINE config 5): each rank
        runs `sample_rotation_sweep` on its contiguous share of `thetas`; since that draws the n-image noise of every step
        once and shares it between its angles, all ranks (seeded alike, ddpm_tasks.py:365) consume the identical noise
        stream however many angles they hold -- "same seed per theta" holds across the shards.  Gathers on `dst`:
        ([x_u8 per angle], [result_u8 per angle]) in the order of `thetas`; (None, None) elsewhere.  A rotation by theta / T
        per step has no meaning on a strided chain: DDIM (steps=) is not supported."""
        if steps is not None:
            raise NotImplementedError("Diffusion.sample_rotation_sweep_sharded: DDIM (steps=) is not supported with rotations")
        thetas = list(thetas)
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            return self.sample_rotation_sweep(model, n, image_channels, thetas)
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        K = len(thetas)
        lo, hi = shard_range(K, rank, world)
        xs, rs = self.sample_rotation_sweep(model, n, image_channels, thetas[lo:hi])
        S = (self.noise_steps - 1) // 100 + 1                       # snapshots at i % 100 == 0 (0 < i < T) + the final x
        shape = (image_channels, self.img_size, self.img_size)
        empty = torch.empty((0,) + shape, dtype=torch.uint8, device=self.device)
        counts = [shard_range(K, r, world)[1] - shard_range(K, r, world)[0] for r in range(world)]
        xa = gather_u8(torch.cat(xs) if xs else empty, [c * n for c in counts], group, dst)
        ra = gather_u8(torch.cat(rs) if rs else empty, [c * n * S for c in counts], group, dst)
        if rank != dst:
            return None, None
        return list(xa.reshape(K, n, *shape)), list(ra.reshape(K, S * n, *shape))

    def sample_rotation_sweep(self, model, n, image_channels, thetas, steps=None):
        """Config E sweep (ddpm_tasks.py:346-369) as ONE batched trajectory.  The reference re-seeds before every angle,
        so every angle consumes the identical noise stream and only the per-step rotation differs: here the
        len(thetas) * n images ride one batch, every noise draw (x_T from the CPU generator, the per-step noise from the
        device generator, n images each: the same draws in the same order as one `sample(n, theta)` call after the same
        seeding) is shared by all angles, and each angle's slice is rotated by its own theta / T after every step.
        One UNet forward per step instead of len(thetas): at n = 4 the sweep is launch-bound, so this is ~9x faster for
        the reference's 9 angles.  Returns ([x_u8 per angle], [result_u8 per angle]) like `rotation_results`.  A rotation by
        theta / T per step has no meaning on a strided chain: DDIM (steps=) is not supported."""
        if steps is not None:
            raise NotImplementedError("Diffusion.sample_rotation_sweep: DDIM (steps=) is not supported with rotations")
        K = len(thetas)
        if K == 0:                                       # (a rank of the sharded sweep that holds no angle)
            return [], []
        snaps = [[] for _ in range(K)]
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, "reference").repeat(K, 1, 1, 1)
            for i in reversed(range(1, self.noise_steps)):
                eps = self.predict_eps(model, x, self._t_full(K * n, i, x.device))
                noise = torch.randn(n, *x.shape[1:], device=x.device).repeat(K, 1, 1, 1) if i > 1 else None
                x = ops.denoise_step(x, eps, noise, self.alpha, self.alpha_hat, self.beta, i)
                for k, th in enumerate(thetas):
                    if th:                                   # the reference rotates only for a truthy theta (:375)
                        x[k * n:(k + 1) * n] = self.rotate_2d_matrix(x[k * n:(k + 1) * n], th / self.noise_steps, self.filter)
                if i % 100 == 0:
                    for k in range(K):
                        snaps[k].append(x[k * n:(k + 1) * n].clone())
        xs, results = [], []
        for k in range(K):
            xk = x[k * n:(k + 1) * n]
            xs.append(ops.quantize_u8(xk))
            results.append(ops.quantize_u8(torch.cat(snaps[k] + [xk])))
        return xs, results

    def sample_concurrent(self, model, n, image_channels, batch=256, streams=4, noise_fn=None, graph=False, steps=None, eta=0.0):
        """Throughput form of `sample` for many images: the n images are cut into batches of `batch` and `streams`
        of those trajectories run CONCURRENTLY, each on its own HIP stream (the trajectories are independent: sampling
        is embarrassingly parallel per image).  One 256-image forward leaves CUs idle in its small layers; a second
        trajectory in flight fills them: measured on MI355X (tools/sample_streams.py) 77 / 96 / 103 / 107 images/s with
        1 / 2 / 3 / 4 trajectories of 256 images in flight (a single 512-image batch: 91).  Returns (x_u8, result_u8) like `sample`, batches
        concatenated.  Noise comes from the device generator (or noise_fn(batch_index, i, x) for tests).
        graph=True: every trajectory's denoise step (UNet forward + update; the noise is drawn into a static buffer just
        before) is captured once into its own hipGraph and replayed on its stream, which takes the host's ~170 launches
        per forward out of the loop.
        steps / eta: DDIM over a strided chain, as for `sample`; noise_fn is then called with i = the step's t (and not at
        all after x_T when eta == 0)."""
        pairs = self._check_ddim("sample_concurrent", steps, eta)
        eta = None if pairs is None else float(eta)          # None: DDPM updates over the full chain
        if pairs is None:
            pairs = [(i, i - 1) for i in reversed(range(1, self.noise_steps))]
        noisy = eta is None or eta > 0
        shape = (image_channels, self.img_size, self.img_size)
        sizes = [min(batch, n - o) for o in range(0, n, batch)]
        pool = [torch.cuda.Stream() for _ in range(max(1, min(streams, len(sizes))))]
        cur = torch.cuda.current_stream()
        xs_out, snaps_out = [None] * len(sizes), [None] * len(sizes)
        slots = {}                                           # graph: (batch size, stream) -> (xs, t, t_prev, noise, graph), captured once

        def slot(b, st):
            """The static buffers of a trajectory of b images on stream st and its captured step, which reads its noise from nz."""
            xs = torch.zeros(b, *shape, device=self.device)
            t_dev = torch.full((b,), self.noise_steps - 1, device=self.device, dtype=torch.long)
            tp_dev = torch.full((1,), pairs[0][1], device=self.device, dtype=torch.long) if eta is not None else None
            nz = torch.zeros_like(xs) if noisy else None

            def one_step():
                self._update(xs, b, self.predict_eps(model, xs, t_dev), nz, t_dev, tp_dev, eta=eta)
            # not `_capture`: the warm-up (allocator, cached weight transforms) runs on the trajectory's own stream, which also
            # captures, and needs no undo: it draws nothing and xs is overwritten with x_T afterwards
            one_step()
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                one_step()
            return xs, t_dev, tp_dev, nz, g

        def advance(k, key, x, i, tp):
            """One step (i -> tp) of trajectory k, in place on x; the last step adds no noise (ddpm_models.py:370-373) and is eager."""
            if graph and tp > 0:
                _, t_dev, tp_dev, nz, g = slots[key]
                t_dev.fill_(i)
                if tp_dev is not None:
                    tp_dev.fill_(tp)
                if nz is None:
                    pass
                elif noise_fn is None:
                    nz.normal_()
                else:
                    nz.copy_(noise_fn(k, i, x.shape))
                g.replay()
                return
            eps = self.predict_eps(model, x, self._t_full(x.shape[0], i, x.device))
            noise = None if not (noisy and tp > 0) else (torch.randn_like(x) if noise_fn is None else noise_fn(k, i, x.shape))
            self._update(x, x.shape[0], eps, noise, i, tp, eta=eta)

        with self._model_scope(model):
            for g0 in range(0, len(sizes), len(pool)):
                group = list(range(g0, min(g0 + len(pool), len(sizes))))
                xs, snaps = {}, {k: [] for k in group}
                for k in group:
                    st = pool[k - g0]
                    st.wait_stream(cur)
                    key = (sizes[k], k - g0)
                    with torch.cuda.stream(st):
                        if graph and key not in slots:
                            slots[key] = slot(sizes[k], st)
                        x_T = torch.randn(sizes[k], *shape, device=self.device) if noise_fn is None \
                            else noise_fn(k, self.noise_steps, (sizes[k], *shape))
                        xs[k] = slots[key][0].copy_(x_T) if graph else x_T.clone()      # (noise_fn's tensor is not written to)
                for i, tp in pairs:
                    for k in group:                                  # one denoise step of every trajectory of the group
                        with torch.cuda.stream(pool[k - g0]):
                            advance(k, (sizes[k], k - g0), xs[k], i, tp)
                            if self.ddim_snapshot(i, tp):
                                snaps[k].append(xs[k].clone())
                for k in group:
                    with torch.cuda.stream(pool[k - g0]):
                        xs_out[k] = ops.quantize_u8(xs[k])
                        snaps_out[k] = ops.quantize_u8(torch.cat(snaps[k] + [xs[k]]))
                    cur.wait_stream(pool[k - g0])
        for t in xs_out + snaps_out:
            t.record_stream(cur)
        return torch.cat(xs_out), torch.cat(snaps_out)

    def revert(self, model, n, image_channels, noise_source="reference", graph=None, steps=None, eta=0.0, sampler=None):
        """steps / eta / sampler: as for `sample`."""
        logging.info(f"Sampling {n} new images....")
        solver, pairs = self._check_sampler("revert", sampler, steps, eta)
        if solver == "dpmpp_2m":
            _, snaps = self._dpmpp_loop(model, n, image_channels, pairs, noise_source, graph)
        elif solver in self.UNIPC_SAMPLERS:
            _, snaps = self._unipc_loop(model, n, image_channels, pairs, self.UNIPC_SAMPLERS[solver], noise_source, graph)
        elif pairs is None:
            _, snaps = self._loop(model, n, image_channels, None, noise_source, graph)
        else:
            _, snaps = self._ddim_loop(model, n, image_channels, pairs, float(eta), noise_source, graph)
        return ops.quantize_u8(torch.cat(snaps))

    # under development in the reference (:388-419); kept as a host-driven loop over the HIP step
    def sample_shift(self, model, n, image_channels, shift=None, noise_source="reference", steps=None):
        """The shift schedule is laid out over the full chain: DDIM (steps=) is not supported."""
        if steps is not None:
            raise NotImplementedError("Diffusion.sample_shift: DDIM (steps=) is not supported")
        logging.info(f"Sampling {n} new images....")
        if shift == 0:
            shift = None
        idx = None
        if shift is not None:
            dur = np.abs(shift) / self.noise_steps
            idx = set(np.round(np.arange(0, self.noise_steps, dur)).astype(int)[1:].tolist())
        with self._model_scope(model):
            x = self._initial_noise(n, image_channels, noise_source)
            for i in reversed(range(1, self.noise_steps)):
                eps = self.predict_eps(model, x, self._t_full(n, i, x.device))
                noise = self._step_noise(x, noise_source) if i > 1 else None
                x = ops.denoise_step(x, eps, noise, self.alpha, self.alpha_hat, self.beta, i)
                if idx is not None and i in idx:
                    x = self.shift_2d_matrix(x, 1 * np.sign(shift), 0, self.device)
        return ops.quantize_u8(x)

    # F17 (Config E): the reference rotates on the CPU with scipy every step (D2H, single-threaded spline,
    # H2D).  For device tensors the same order-3 / grid-wrap / prefiltered spline runs in a HIP kernel (fp64).
    @staticmethod
    def rotate_2d_matrix(matrix, degrees, filter=None):
        if matrix.is_cuda:
            return ops.rotate_spline3_wrap(matrix, degrees)
        from scipy import ndimage
        r = ndimage.rotate(input=matrix.numpy(), angle=degrees, axes=(2, 3), reshape=False, mode="grid-wrap")
        return torch.from_numpy(r)

    @staticmethod
    def shift_2d_matrix(matrix, hshift, vshift, device):
        """ndimage.shift(x, (0,0,v,h), mode='grid-wrap') (ddpm_models.py:431-436).  The reference only ever
        shifts by whole pixels (:415), where the periodic spline shift is exactly a roll: done on the device.  A fractional
        shift of a device tensor is the affine spline kernel with the identity matrix and offset (-v, -h), which is what
        ndimage.shift computes; host tensors go through scipy."""
        if matrix.is_cuda and float(hshift).is_integer() and float(vshift).is_integer():
            return torch.roll(matrix, shifts=(int(vshift), int(hshift)), dims=(2, 3)).to(device)
        if matrix.is_cuda and matrix.dtype == torch.float32 and matrix.dim() == 4:
            return ops.affine_spline3_wrap(matrix, np.eye(2), (-float(vshift), -float(hshift))).to(device)
        from scipy import ndimage
        r = ndimage.shift(input=matrix.cpu().numpy(), shift=(0, 0, vshift, hshift), mode="grid-wrap")
        return torch.from_numpy(r).to(device)
