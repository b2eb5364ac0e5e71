"""fp64 restatement, in torch, of the learned-variance definitions: the hybrid loss with its gradients by
autograd, the bound's per-row terms, and the ancestral step.  Shared by tests/test_lvar_host.py (on the CPU) and
tests/test_gpu_lvar.py (on the device: 1 + tanh cancels in the decoder's tails, where one ulp of a different tanh moves log P
by more than the gates, so the yardstick uses the device's fp64 tanh, as tests/test_gpu_bpd.py does)."""
import math

import torch

LN2 = math.log(2.0)


def tables64(beta, alpha, alpha_hat):
    """(T, 3) fp64 [lb_t, lbt_t, k_t] from the fp32 tables widened to fp64; row 0 is zeros."""
    b, a, ah = beta.detach().cpu().double(), alpha.detach().cpu().double(), alpha_hat.detach().cpu().double()
    T = b.numel()
    tab = torch.zeros(T, 3, dtype=torch.float64)
    t = torch.arange(1, T)
    bt = (1.0 - ah[t - 1]) / (1.0 - ah[t]) * b[t]
    tab[1:, 0] = torch.log(b[t])
    tab[1:, 1] = torch.log(bt)
    tab[1:, 2] = b[t] * b[t] / (a[t] * (1.0 - ah[t]))
    return tab


def logvar64(v, lb, lbt):
    f = (v + 1.0) / 2.0
    return f * lb + (1.0 - f) * lbt


def eps_hat32(kind, p, xt, sa, sb):
    """The output -> eps in fp32, one rounding per operation (pred_to_eps' expressions)."""
    if kind == "v":
        return sa * p + sb * xt
    if kind == "x0":
        return (xt - sa * p) / sb
    return p


def decoder_mean32(beta, alpha, alpha_hat, xt, eh):
    """denoise_step's fp32 expression at i = 1 without noise."""
    a, ah = alpha[1], alpha_hat[1]
    c1 = 1.0 / torch.sqrt(a)
    c2 = (1.0 - a) / torch.sqrt(1.0 - ah)
    return c1 * (xt - c2 * eh)


def decoder_logp64(x, mean, inv_stdv):
    c = x - mean

    def cdf(z):
        return 0.5 * (1.0 + torch.tanh(0.7978845608028654 * (z + 0.044715 * ((z * z) * z))))

    cp, cm = cdf(inv_stdv * (c + 1.0 / 255.0)), cdf(inv_stdv * (c - 1.0 / 255.0))
    P = torch.where(x < -0.999, cp, torch.where(x > 0.999, 1.0 - cm, cp - cm))
    return torch.log(torch.clamp(P, min=1e-12)), P


def hybrid(beta, alpha, alpha_hat, kind, out2, x0, eps, t, w=None, vlb_scale=0.0, xt=None, dev="cpu"):
    """out2 (B, 2 chw), x0, eps (B, chw) fp32; t (B,) int64; w (T,) fp32 or None.  -> dict of fp64 CPU tensors: L, L_vlb, dp, dv
    (the gradients of L for dloss = 1), term and sq per row, P (the decoder rows' bin probabilities before the clamp, row-major)
    and clamped (a bool mask over out2's v half).  xt: the noised rows when given (the bound), else recomputed in fp32."""
    beta, alpha, alpha_hat = (v.detach().to(dev).float() for v in (beta, alpha, alpha_hat))
    out2, x0, eps, t = out2.detach().to(dev), x0.detach().to(dev), eps.detach().to(dev), t.to(dev)
    B, chw = x0.shape
    N = B * chw
    tab = tables64(beta, alpha, alpha_hat).to(dev)
    lb, lbt, kt = (tab[t, i][:, None] for i in range(3))
    p = out2[:, :chw].double().requires_grad_(True)
    v = out2[:, chw:].double().requires_grad_(True)
    ah32 = alpha_hat[t][:, None]
    ah = ah32.double()
    sa, sb = torch.sqrt(ah), torch.sqrt(1.0 - ah)
    x, e = x0.double(), eps.double()
    target = {"eps": e, "x0": x, "v": sa * e - sb * x}[kind]
    wr = torch.ones(B, dtype=torch.float64, device=dev) if w is None else w.to(dev).double()[t]
    l_simple = (wr[:, None] * (p - target) ** 2).sum() / N
    f2 = {"eps": torch.ones_like(ah), "v": ah, "x0": ah / (1.0 - ah)}[kind]
    d2 = f2 * (p.detach() - target) ** 2
    lv = logvar64(v, lb, lbt)
    xx = lv - lbt
    kl = 0.5 * ((xx + torch.expm1(-xx)) + (kt * d2) * torch.exp(-lv))
    dec = t == 1
    term = kl.sum(dim=1)
    P = torch.zeros(0, chw, dtype=torch.float64)
    clamped = torch.zeros(B, chw, dtype=torch.bool)
    if bool(dec.any()):
        sa32, sb32 = torch.sqrt(ah32[dec]), torch.sqrt(1.0 - ah32[dec])
        xt32 = sa32 * x0[dec] + sb32 * eps[dec] if xt is None else xt.detach().to(dev)[dec]
        eh = eps_hat32(kind, out2[dec, :chw], xt32, sa32, sb32)
        mean = decoder_mean32(beta, alpha, alpha_hat, xt32, eh)
        lp, P = decoder_logp64(x[dec], mean.double(), torch.exp(-(lv[dec] / 2.0)))
        term = term.clone()
        term[dec] = -lp.sum(dim=1)
        clamped[dec.cpu()] = (P < 1e-12).cpu()
        P = P.detach().cpu()
    l_vlb = term.sum() / (N * LN2)
    L = l_simple + vlb_scale * l_vlb
    L.backward()
    cpu = lambda z: z.detach().cpu()
    return {"L": cpu(L), "L_vlb": cpu(l_vlb), "L_simple": cpu(l_simple), "dp": cpu(p.grad),
            "dv": cpu(v.grad) if v.grad is not None else torch.zeros(B, chw, dtype=torch.float64),
            "term": cpu(term), "sq": cpu(d2.sum(dim=1)), "P": P, "clamped": clamped}


def step64(beta, alpha, alpha_hat, kind, x, out2, noise, i, cfg_scale=None):
    """The ancestral step i -> i - 1 in fp64 on the CPU -> fp64 (B, chw).  x (B, chw); out2 (B, 2 chw), or (2 B, 2 chw) with
    cfg_scale (conditional rows, then unconditional); noise (B, chw) or None; no noise at i = 1."""
    tab = tables64(beta, alpha, alpha_hat)
    b, a, ah = (v.detach().cpu().double()[i] for v in (beta, alpha, alpha_hat))
    B, chw = x.shape
    xd, o = x.detach().cpu().double(), out2.detach().cpu().double()
    sa, sb = torch.sqrt(ah), torch.sqrt(1.0 - ah)

    def to_eps(p):
        return {"eps": p, "v": sa * p + sb * xd, "x0": (xd - sa * p) / sb}[kind]

    e = to_eps(o[:B, :chw])
    if cfg_scale is not None:
        eu = to_eps(o[B:, :chw])
        e = eu + cfg_scale * (e - eu)
    mean = (xd - (1.0 - a) / torch.sqrt(1.0 - ah) * e) / torch.sqrt(a)
    if noise is None or i == 1:
        return mean
    lv = logvar64(o[:B, chw:], tab[i, 0], tab[i, 1])
    return mean + torch.exp(0.5 * lv) * noise.detach().cpu().double()


def case(B, chw, T, seed, schedule_tables, kind):
    """The loss tests' inputs: x0 on the 8-bit grid with both ends present, eps ~ N(0, 1), the prediction such that
    eps_hat - eps ~ 0.1 N(0, 1) (formed in fp64, rounded once), v uniform in [-1.5, 1.5], and t with 1, 2 and T - 1 present
    whenever B >= 3 (B = 1: t = 2)."""
    beta, alpha, alpha_hat = schedule_tables
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 256, (B, chw), generator=g)
    k[:, ::7] = 0
    k[:, 3::11] = 255
    x0 = k.float() / 127.5 - 1.0
    eps = torch.randn(B, chw, generator=g)
    t = torch.randint(1, T, (B,), generator=g)
    if B >= 3:
        t[0], t[1], t[2] = 1, 2, T - 1
    else:
        t[0] = 2
    ah = alpha_hat.detach().cpu().double()[t][:, None]
    sa, sb = torch.sqrt(ah), torch.sqrt(1.0 - ah)
    eh = eps.double() + 0.1 * torch.randn(B, chw, generator=g).double()
    xt = sa * x0.double() + sb * eps.double()
    p = {"eps": eh, "v": (eh - sb * xt) / sa, "x0": (xt - sb * eh) / sa}[kind].float()
    v = torch.rand(B, chw, generator=g) * 3.0 - 1.5
    return torch.cat([p, v], dim=1).contiguous(), x0, eps, t


def decoder_case(rows, chw, seed):
    """Decoder rows (every t = 1, eps-prediction) that cover both edge bins, interior bins and the 1e-12 clamp: x0 on the 8-bit
    grid with 0 and 255 forced, eps_hat = eps + scale * N(0, 1) with the per-element scales of test_terms_kernel_against_fp64."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 256, (rows, chw), generator=g)
    k[:, ::5] = 0
    k[:, 1::9] = 255
    x0 = k.float() / 127.5 - 1.0
    eps = torch.randn(rows, chw, generator=g)
    scale = torch.tensor([0.0, 0.05, 0.5, 2.0, 8.0, 40.0, 400.0])[torch.randint(0, 7, (rows, chw), generator=g)]
    p = eps + scale * torch.randn(rows, chw, generator=g)
    v = torch.rand(rows, chw, generator=g) * 3.0 - 1.5
    t = torch.ones(rows, dtype=torch.long)
    return torch.cat([p, v], dim=1).contiguous(), x0, eps, t
