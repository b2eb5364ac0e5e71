"""UniPC (Zhao et al. 2023), the multistep data-prediction form with B(h) = expm1(-h) ("bh2"): the order
rule, the weights rho of the predictor and the corrector, and `unipc_reference`, the loop of `Diffusion.sample(sampler="unipc_*")`
in plain torch fp64 on CPU tensors, written from the rho / D_i form -- the oracle of the folded coefficient table
(`Diffusion.unipc_coefficients`) and of the kernel.  Nothing here touches a device.

Levels lev = taus + [0]; alpha(t) = sqrt(a_t), sigma(t) = sqrt(1 - a_t), lam = log alpha - log sigma, a_t the fp32 alpha_hat[t]
widened to fp64.  Evaluation k runs the network at the predicted state x~_k of level lev[k]: m_k = (x~_k - sigma e) / alpha.
A move s -> u of order p from the state x with base m_0 = m at s and the earlier m_i at levels s_i (i = 1 .. p-1):
    h = lam(u) - lam(s), B = expm1(-h), r_i = (lam(s_i) - lam(s)) / h, D_i = (m_i - m_0) / r_i
    predictor:  x' = (sigma_u / sigma_s) x - alpha_u B m_0 - alpha_u B  sum_{i<p} rho_i D_i
    corrector:  the same sum plus rho_p (m_new - m_0), m_new the evaluation at the predictor's x'
rho solves R rho = b, R[j][i] = r_i^j (the corrector's r_p = 1), b_j = g_{j+1} (j+1)! / B with hh = -h, g_1 = expm1(hh) / hh - 1,
g_{j+1} = g_j / hh - 1 / (j+1)!; the predictor takes the leading (p-1) x (p-1) system (p = 2: rho = [1/2], as diffusers does);
the corrector of order 1 takes rho = [1/2]."""
import math

import torch

from .ops import NULL_LABEL

MAX_ORDER = 3


def unipc_order(k, S, P):
    """The order of the predictor's move out of evaluation k (0 <= k < S) of an S-step chain of order P: min(P, k + 1), and,
    when S < 15, also min(., S - k) (`Diffusion.dpmpp_order`'s lower-order-final rule)."""
    p = min(int(P), k + 1)
    return min(p, S - k) if S < 15 else p


def unipc_rho(rs, h, corrector):
    """The weights of one move of log-SNR width h: rs = [r_1 .. r_{p-1}] of the earlier evaluations -> rho, p - 1 values for the
    predictor, p for the corrector (the last one weighs m_new - m_0).  fp64."""
    p = len(rs) + 1
    hh = -h
    B = math.expm1(hh)
    g, fact, b = math.expm1(hh) / hh - 1.0, 1.0, []
    for j in range(1, p + 1):
        b.append(g * fact / B)
        fact *= j + 1
        g = g / hh - 1.0 / fact
    if not corrector:
        return [] if p == 1 else [0.5] if p == 2 else _solve_powers(list(rs), b[:-1])
    return [0.5] if p == 1 else _solve_powers(list(rs) + [1.0], b)


def _solve_powers(r, b):
    """rho with sum_i rho_i r_i^j = b_j for j = 0 .. len(r) - 1, two or three unknowns, in closed form: rho_i collects b against
    the coefficients of the Lagrange polynomial of node i (a table of S rows needs 2 S of these, on the host, before the first
    launch of a trajectory)."""
    if len(r) == 2:
        rho = (b[1] - b[0] * r[1]) / (r[0] - r[1])
        return [rho, b[0] - rho]
    (r1, r2, r3), node = r, lambda a, o1, o2: (b[2] - b[1] * (o1 + o2) + b[0] * o1 * o2) / ((a - o1) * (a - o2))
    return [node(r1, r2, r3), node(r2, r1, r3), node(r3, r1, r2)]


def schedule_levels(alpha_hat, pairs):
    """-> (lev, alpha, sigma, lam): the S + 1 levels taus + [0] of the chain `pairs` and alpha, sigma, lam at each, python floats
    (fp64) from the fp32 table."""
    ah = torch.as_tensor(alpha_hat).detach().cpu().tolist()
    lev = [int(t) for t, _ in pairs] + [int(pairs[-1][1])]
    alpha = [math.sqrt(ah[t]) for t in lev]
    sigma = [math.sqrt(1.0 - ah[t]) for t in lev]
    lam = [math.log(a) - math.log(s) for a, s in zip(alpha, sigma)]
    return lev, alpha, sigma, lam


def unipc_reference(model, x_T, pairs, order, diffusion, labels=None, cfg_scale=0.0, corrector=True):
    """`Diffusion._unipc_loop` in fp64 on CPU tensors.  model(x, t[, y]) -> eps at the fp64 (rows, ...) state x and the int64
    (rows,) timesteps t (y: int64 labels, passed only when `labels` is given); x_T: (n, ...) the start; pairs: the chain
    [(t, t_prev)], the last t_prev 0; order: P in 1 .. 3; diffusion: supplies alpha_hat.  With labels and cfg_scale > 0 every
    evaluation is one call on the 2n rows [x ; x] with the labels [labels ; NULL_LABEL] and
    eps = e_u + cfg_scale (e_c - e_u).  corrector=False leaves the corrector out (the bare predictor: DDIM at P = 1,
    DPM-Solver++(2M) at P = 2).  -> the fp64 sample, the last predictor's output."""
    P = int(order)
    if not 1 <= P <= MAX_ORDER:
        raise ValueError(f"unipc_reference: order must be 1, 2 or 3 (got {order!r})")
    lev, alpha, sigma, lam = schedule_levels(diffusion.alpha_hat, pairs)
    S = len(pairs)
    x = x_T.detach().cpu().double()
    n = x.shape[0]
    guided = labels is not None and cfg_scale > 0
    y = None
    if labels is not None:
        y = torch.as_tensor(labels).detach().cpu().long()
        if guided:
            y = torch.cat([y, torch.full_like(y, NULL_LABEL)])

    def eps_at(xs, t):
        rows = torch.cat([xs, xs]) if guided else xs
        tt = torch.full((rows.shape[0],), t, dtype=torch.long)
        e = (model(rows, tt) if y is None else model(rows, tt, y)).double()
        return e[n:] + cfg_scale * (e[:n] - e[n:]) if guided else e

    def move(x_from, s, u, base, earlier, m_new=None):
        """s, u: positions in lev; base: m at s; earlier: [(position, m)] of the p - 1 evaluations before it, latest first."""
        h = lam[u] - lam[s]
        B = math.expm1(-h)
        rs = [(lam[q] - lam[s]) / h for q, _ in earlier]
        rho = unipc_rho(rs, h, m_new is not None)
        res = torch.zeros_like(x_from)
        for (q, m), r, w in zip(earlier, rs, rho):
            res = res + w * ((m - base) / r)
        if m_new is not None:
            res = res + rho[-1] * (m_new - base)
        return (sigma[u] / sigma[s]) * x_from - alpha[u] * B * base - alpha[u] * B * res

    hist = []                                         # [(position, m)], latest first
    xc = x                                            # the corrected state at the last evaluation's level
    pred = x
    with torch.no_grad():
        for k in range(S):
            m = (pred - sigma[k] * eps_at(pred, lev[k])) / alpha[k]
            if k >= 1 and corrector:
                p = unipc_order(k - 1, S, P)
                xc = move(xc, k - 1, k, hist[0][1], hist[1:p], m_new=m)
            else:
                xc = pred
            p = unipc_order(k, S, P)
            pred = move(xc, k, k + 1, m, hist[:p - 1])
            hist = [(k, m)] + hist[:MAX_ORDER - 1]
    return pred
