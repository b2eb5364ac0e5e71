"""Likelihoods from the probability-flow ODE (Song et al. 2021, section 4.3 and appendix D.2): the probes of
the Hutchinson trace estimate and `ode_likelihood_reference`, the loop of `Diffusion.ode_likelihood` in plain torch fp64 on CPU
tensors with autograd -- the oracle of the kernels' and the method's tests.  Nothing here touches a device.

With a = alpha_hat[t], sig = sqrt((1 - a) / a) and y = x / sqrt(a) the ODE is dy / dsig = eps(x, t) and
    log p_0(x_0) = log N(x_U; 0, I) + (d / 2) (log a_U - log a_0) + Integral_{sig_0}^{sig_U} sqrt(a) tr J_eps(x, t) dsig,
J_eps = d eps / d x = c1 I + c2 J_out for the network's output `out` (`Diffusion.eps_jacobian_coefficients`), so that for a
probe v and w = J_out^T v the estimate of the trace is v^T J_eps v = c1 |v|^2 + c2 v.w."""
import math

import torch

METHODS = ("heun", "euler")
PROBES = ("rademacher", "gaussian", "basis")


def basis_probes(n, shape):
    """The d = prod(shape) unit vectors as probes: fp32 (d, n, *shape), probe p is 1 at flat position p of every row.  Summed
    (not averaged) over the probes, v^T J v is the exact trace."""
    d = int(math.prod(shape))
    return torch.eye(d, dtype=torch.float32).view(d, 1, *shape).repeat(1, n, *([1] * len(shape))).contiguous()


def draw_probes(kind, probes, n, shape, device=None):
    """The probes of one call, fp32 (P, n, *shape), drawn once: "rademacher" (+-1, from torch.randint(0, 2)), "gaussian"
    (torch.randn), each as ONE draw of the whole (P, n, *shape) tensor from the global generator of `device` (None: the CPU
    generator), or "basis" (`basis_probes`: nothing is drawn and `probes` is ignored)."""
    if kind == "basis":
        return basis_probes(n, shape)
    full = (int(probes), int(n)) + tuple(shape)
    if kind == "rademacher":
        return (torch.randint(0, 2, full, device=device) * 2 - 1).to(torch.float32)
    if kind == "gaussian":
        return torch.randn(full, device=device, dtype=torch.float32)
    raise ValueError(f"likelihood.draw_probes: unknown probe {kind!r} (one of {PROBES})")


def sigma_levels(alpha_hat, levels):
    """-> (a, sig): alpha_hat[level] widened to fp64 and sqrt((1 - a) / a), two python lists over `levels`."""
    table = torch.as_tensor(alpha_hat).detach().cpu().double()
    a = [float(table[int(t)]) for t in levels]
    return a, [math.sqrt((1.0 - v) / v) for v in a]


def ode_likelihood_reference(eps_fn, x0, alpha_hat, levels, probes_tensor, method="heun", coefficients=None):
    """`Diffusion.ode_likelihood`'s loop in fp64 on CPU tensors.
    eps_fn(x, t) -> the network's output `out` at the fp64 (n, ...) state x and the int level t, differentiable by autograd;
    coefficients(t) -> (c1, c2), two floats with eps = c1 x + c2 out and so J_eps = c1 I + c2 J_out (None: (0, 1), the output is
    eps itself); x0: (n, ...) the images; alpha_hat: the schedule table (widened to fp64); levels: [0] + reversed(taus), ascending;
    probes_tensor: (P, n, ...), fixed along the trajectory; method: "heun" (the first move, out of level 0, is an Euler move) or
    "euler".  The state moves with the output of probe 0's evaluation.
    -> a dict: logp, bpd, prior_logp, trace (the mean over probes), trace_sem (n,) fp64; trace_probes (P, n), each probe's integral
    (their SUM is the exact trace for `basis_probes`); latents (n, ...) fp64, x_U; evaluations, a list of one dict per network
    evaluation in order {"t", "weight", "c1", "c2", "tr": (P, n) the estimates c1 |v|^2 + c2 v.w}; bound_scale (P, n), the sum over
    evaluations of |weight c2| |v| |w|, what the rounding error of a device run's trace is measured against."""
    if method not in METHODS:
        raise ValueError(f"ode_likelihood_reference: unknown method {method!r} (one of {METHODS})")
    levels = [int(t) for t in levels]
    if len(levels) < 2 or levels[0] != 0 or any(a >= b for a, b in zip(levels, levels[1:])):
        raise ValueError(f"ode_likelihood_reference: levels must ascend from 0 (got {levels})")
    a, sig = sigma_levels(alpha_hat, levels)
    x = x0.detach().cpu().double()
    v = probes_tensor.detach().cpu().double()
    P, n = int(v.shape[0]), int(x.shape[0])
    if tuple(v.shape[1:]) != tuple(x.shape):
        raise ValueError(f"ode_likelihood_reference: probes_tensor must be (P,) + {tuple(x.shape)} (got {tuple(v.shape)})")
    d = x[0].numel()
    vv = (v * v).flatten(2).sum(2)
    vnorm = vv.sqrt()
    trace = torch.zeros(P, n, dtype=torch.float64)
    scale = torch.zeros(P, n, dtype=torch.float64)
    evaluations = []

    def evaluate(xs, t, weight):
        """eps at (xs, t) from probe 0's forward; every probe's estimate, weighted, goes into `trace`."""
        c1, c2 = (0.0, 1.0) if coefficients is None else (float(c) for c in coefficients(t))
        tr = torch.empty(P, n, dtype=torch.float64)
        eps = None
        for p in range(P):
            with torch.enable_grad():
                leaf = xs.detach().clone().requires_grad_(True)
                out = eps_fn(leaf, t)
                (w,) = torch.autograd.grad(out, leaf, v[p])
            if p == 0:
                eps = c1 * xs + c2 * out.detach()
            tr[p] = c1 * vv[p] + c2 * (v[p] * w).flatten(1).sum(1)
            scale[p] += abs(weight * c2) * vnorm[p] * w.flatten(1).norm(dim=1)
        trace.add_(weight * tr)
        evaluations.append({"t": t, "weight": weight, "c1": c1, "c2": c2, "tr": tr})
        return eps

    for k in range(len(levels) - 1):
        s, u = levels[k], levels[k + 1]
        h = sig[k + 1] - sig[k]
        ra_s, ra_u = math.sqrt(a[k]), math.sqrt(a[k + 1])
        if method == "euler" or s == 0:
            eps = evaluate(x, u, h * ra_u)
            x = ra_u * (x / ra_s + h * eps)
            continue
        eps_s = evaluate(x, s, 0.5 * h * ra_s)
        pred = ra_u * (x / ra_s + h * eps_s)
        eps_u = evaluate(pred, u, 0.5 * h * ra_u)
        x = ra_u * (x / ra_s + h * (eps_s + eps_u) / 2)

    prior = -0.5 * (x * x).flatten(1).sum(1) - 0.5 * d * math.log(2.0 * math.pi)
    mean = trace.mean(0)
    sem = trace.std(0, unbiased=True) / math.sqrt(P) if P > 1 else torch.zeros(n, dtype=torch.float64)
    logp = prior + 0.5 * d * (math.log(a[-1]) - math.log(a[0])) + mean
    return {"logp": logp, "bpd": bpd_from_logp(logp, d), "prior_logp": prior, "trace": mean, "trace_sem": sem, "trace_probes": trace,
            "latents": x, "evaluations": evaluations, "bound_scale": scale}


def bpd_from_logp(logp, d):
    """bits per dimension of 8-bit data from the log-density (nats) of images scaled to [-1, 1]: -logp / (d ln 2) + log2(127.5),
    the change of variables from the 256 levels, one level 1 / 127.5 wide."""
    return -logp / (d * math.log(2.0)) + math.log2(127.5)
