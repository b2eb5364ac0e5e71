"""Analytic-DPM (Bao et al., ICLR 2022): the optimal reverse variance of a trained eps / v / x0 model, in closed form from one
scalar per timestep, G_t = E|eps_theta(x_t, t)|^2 / d, estimated once over the training set (`Diffusion.
estimate_analytic_variance`; the per-row sums are ops.eps_sqnorm_rows).  `AnalyticVariance` holds that table on the host and turns
it into the sigmas of a chain: `Diffusion.sample_analytic(steps=, eta=)` draws with them (ops.ddim_step_var) and
`Diffusion.calc_bpd(sigma=)` scores with them.  DESIGN.md section 6zd has the derivation."""
import numpy as np
import torch


class AnalyticVariance:
    """gamma: (T,) fp64 host array, G_t where it was estimated and NaN elsewhere; count: (T,) int64, the rows behind each
    estimate.  noise_steps, schedule, prediction and alpha_hat (the fp32 table, as a numpy array) name the process it was
    estimated on: `sigma2` refuses another one."""

    def __init__(self, gamma, count, noise_steps, schedule, prediction, alpha_hat):
        T = int(noise_steps)
        self.gamma = np.ascontiguousarray(np.asarray(gamma, dtype=np.float64))
        self.count = np.ascontiguousarray(np.asarray(count, dtype=np.int64))
        if isinstance(alpha_hat, torch.Tensor):
            alpha_hat = alpha_hat.detach().cpu().numpy()
        self.alpha_hat = np.ascontiguousarray(np.asarray(alpha_hat, dtype=np.float32))
        if self.gamma.shape != (T,) or self.count.shape != (T,) or self.alpha_hat.shape != (T,):
            raise ValueError(f"AnalyticVariance: gamma, count and alpha_hat must have shape ({T},) (got {self.gamma.shape}, "
                             f"{self.count.shape}, {self.alpha_hat.shape})")
        self.noise_steps, self.schedule, self.prediction = T, str(schedule), str(prediction)

    @classmethod
    def for_diffusion(cls, diffusion, gamma, count=None):
        """The table `gamma` ((T,) values, NaN where there is none) bound to `diffusion`'s process."""
        gamma = np.asarray(gamma, dtype=np.float64)
        count = (~np.isnan(gamma)).astype(np.int64) if count is None else count
        return cls(gamma, count, diffusion.noise_steps, diffusion.schedule, diffusion.prediction, diffusion.alpha_hat)

    def save(self, path):
        """Write the table as an .npz file (`load` reads it back bit for bit)."""
        with open(path, "wb") as f:
            np.savez(f, gamma=self.gamma, count=self.count, alpha_hat=self.alpha_hat, noise_steps=np.int64(self.noise_steps),
                     schedule=np.array(self.schedule), prediction=np.array(self.prediction))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            return cls(z["gamma"], z["count"], int(z["noise_steps"]), str(z["schedule"]), str(z["prediction"]), z["alpha_hat"])

    def _check(self, diffusion, ts):
        """ValueError unless the table was estimated on diffusion's process and holds an estimate at every timestep of ts."""
        if diffusion.noise_steps != self.noise_steps:
            raise ValueError(f"AnalyticVariance: estimated with noise_steps = {self.noise_steps}, the process has "
                             f"{diffusion.noise_steps}")
        ah = diffusion.alpha_hat.detach().cpu().numpy()
        if ah.dtype != np.float32 or not np.array_equal(ah, self.alpha_hat):
            raise ValueError(f"AnalyticVariance: estimated on another noise schedule (a {self.schedule!r} one whose alpha_hat differs "
                             f"from this process's {diffusion.schedule!r} table)")
        ts = [int(t) for t in ts]
        if any(not 1 <= t < self.noise_steps for t in ts):
            raise ValueError(f"AnalyticVariance: every timestep must lie in [1, {self.noise_steps - 1}] (got {ts})")
        missing = [t for t in ts if np.isnan(self.gamma[t])]
        if missing:
            shown = ", ".join(str(t) for t in missing[:12]) + (", ..." if len(missing) > 12 else "")
            raise ValueError(f"AnalyticVariance: no estimate at timestep{'s' if len(missing) > 1 else ''} {shown} "
                             f"({len(missing)} of the chain's {len(ts)}): estimate the table on this chain's timesteps")

    def sigma2(self, diffusion, pairs, eta, last_sigma_max=None):
        """The optimal variance of each step (t, p) of `pairs`, an fp64 array, from the fp32 alpha_hat widened to fp64: with
        a_t = alpha_hat[t], a_p = alpha_hat[p] (p = 0 reads alpha_hat[0], as the DDIM step does),
          lam2  = eta^2 ((1 - a_p) / (1 - a_t)) (1 - a_t / a_p)            dir = sqrt(max((1 - a_p) - lam2, 0))
          sig*2 = lam2 + (sqrt((1 - a_t) a_p / a_t) - dir)^2 (1 - clip(G_t, 0, 1))
        lam2 and dir are DDIM's own at that eta, whose mean the step keeps.  last_sigma_max: a cap on sigma* of the last step
        that draws noise (the last pair with p > 0), the paper's clipping of the step before the noiseless one; None: no cap."""
        pairs = [(int(t), int(p)) for t, p in pairs]
        eta = float(eta)
        if not eta >= 0:
            raise ValueError(f"AnalyticVariance: eta must be >= 0 (got {eta})")
        if any(not 0 <= p < t for t, p in pairs):
            raise ValueError(f"AnalyticVariance: every pair needs 0 <= t_prev < t (got {pairs})")
        self._check(diffusion, [t for t, _ in pairs])
        if last_sigma_max is not None and not float(last_sigma_max) >= 0:
            raise ValueError(f"AnalyticVariance: last_sigma_max must be >= 0 or None (got {last_sigma_max!r})")
        ah = self.alpha_hat.astype(np.float64)
        out = np.zeros(len(pairs), dtype=np.float64)
        for k, (t, p) in enumerate(pairs):
            a_t, a_p = ah[t], ah[p]
            lam2 = (eta * eta) * (((1.0 - a_p) / (1.0 - a_t)) * (1.0 - a_t / a_p))
            dirc = np.sqrt(max((1.0 - a_p) - lam2, 0.0))
            g = min(max(self.gamma[t], 0.0), 1.0)
            out[k] = lam2 + (np.sqrt((1.0 - a_t) * a_p / a_t) - dirc) ** 2 * (1.0 - g)
        if last_sigma_max is not None:
            noisy = [k for k, (_, p) in enumerate(pairs) if p > 0]
            if noisy:
                out[noisy[-1]] = min(out[noisy[-1]], float(last_sigma_max) ** 2)
        return out

    def sigma_table(self, diffusion, pairs, eta, last_sigma_max=None):
        """(T,) fp32 host tensor, sqrt(sigma2) of each pair at index t, rounded once from fp64; 0 at every other index.  The
        table ops.ddim_step_var reads."""
        s2 = self.sigma2(diffusion, pairs, eta, last_sigma_max)
        tab = np.zeros(self.noise_steps, dtype=np.float64)
        tab[[int(t) for t, _ in pairs]] = np.sqrt(s2)
        return torch.from_numpy(tab.astype(np.float32))
