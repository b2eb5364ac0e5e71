"""The f16x2 token-chain kernels (csrc/tok_h2.hip, C = 64 and 128) behind afd_tok_{head,tail}_{fwd,bwd}: against the fp64
oracle at the project's TOL, against the fp32 forms (afd_debug_tok_path(3)) at the 5e-6 of the fused-block test, on tile
shapes that go wrong first, on a 2^24 spread of token magnitudes inside one tile, with parameters at odd float offsets,
and on zeros and infinities.  Path modes: 0 = by the rule, 3 = the fp32 forms, 4 = the f16x2 forms wherever they exist."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu
TOL = 1e-5            # tests/test_gpu_ops.py
TOL_FP32_FORMS = 5e-6
EPS = 1e-5


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    yield afdm, ops, gpu
    afdm.lib().afd_debug_tok_path(0)
    afdm.lib().afd_debug_tok_grid(0)


def _g(seed):
    return torch.Generator().manual_seed(seed)


class _path:
    def __init__(self, L, mode, grid=0):
        self.L, self.mode, self.grid = L, mode, grid

    def __enter__(self):
        self.L.afd_debug_tok_path(self.mode)
        self.L.afd_debug_tok_grid(self.grid)

    def __exit__(self, *exc):
        self.L.afd_debug_tok_path(0)
        self.L.afd_debug_tok_grid(0)


# B * P = 48 (one and a half tiles, tiles spanning images), 80, 144, 192 (six tiles: with four tiles per workgroup the
# second workgroup has idle waves that must still reach every barrier), 128 exactly
SHAPES = [(3, 4), (5, 4), (9, 4), (3, 8), (2, 8)]


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"B{b}_{s}x{s}" for b, s in SHAPES])
def test_block_vs_oracle_and_fp32_forms(A, C, shape):
    afdm, ops, dev = A
    B, S = shape
    g = _g(77 + B + C + S)
    torch.manual_seed(11 + C + S)
    mod = afdm.SelfAttention(C, S)
    with torch.no_grad():
        for q in mod.parameters():
            q.add_(0.1 * torch.randn(q.shape, generator=g))
    sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    x = torch.randn(B, C, S, S, generator=g)
    dy = torch.randn(B, C, S, S, generator=g)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    y64 = R.self_attention(sd64, "", x64)
    names = list(sd64)
    ref = torch.autograd.grad(y64, [x64] + [sd64[k] for k in names], dy.double())
    mod = mod.to(dev)
    L = afdm.lib()

    def run(mode, grid):
        with _path(L, mode, grid):
            xi = x.to(dev).requires_grad_(True)
            y = mod(xi)
            params = dict(mod.named_parameters())
            grads = torch.autograd.grad(y, [xi] + [params[k] for k in names], dy.to(dev))
            with torch.no_grad():
                y_inf = mod(x.to(dev))
            return y.detach().cpu(), [t.cpu() for t in grads], y_inf.cpu()

    def errs(out):
        y, grads, _ = out
        e = {"y": rel_l2(y, y64.detach()), "x": rel_l2(grads[0], ref[0])}
        for k, gk, rk in zip(names, grads[1:], ref[1:]):
            e[k] = rel_l2(gk, rk)
        return e

    fp32 = run(3, 0)
    e32 = errs(fp32)
    w32 = max(e32, key=e32.get)
    print(f"tok C{C} B{B} {S}x{S} fp32 forms : fwd {e32['y']:.2e}, worst {w32} {e32[w32]:.2e}")
    for tag, mode, grid in (("rule", 0, 0), ("f16x2", 4, 0), ("f16x2 one workgroup", 4, 1), ("rule one workgroup", 0, 1)):
        out = run(mode, grid)
        e = errs(out)
        worst = max(e, key=e.get)
        e_vs = max([rel_l2(out[0], fp32[0])] + [rel_l2(a, b) for a, b in zip(out[1], fp32[1])])
        print(f"tok C{C} B{B} {S}x{S} {tag:20s}: fwd {e['y']:.2e}, worst {worst} {e[worst]:.2e}, vs fp32 forms {e_vs:.2e}")
        assert e[worst] < TOL, (tag, e)
        assert e_vs < TOL_FP32_FORMS, (tag, e_vs)
        assert torch.equal(out[0], out[2]), tag                  # train form against inference form: bit-equal
    assert e32[w32] < TOL, e32


def _per_token_err(a, ref):
    """worst per-token rel-L2 of (B, C', S, S) tensors over the channel axis"""
    d = (a.double() - ref).pow(2).sum(1).sqrt()
    n = ref.pow(2).sum(1).sqrt()
    return float((d / n).max())


@pytest.mark.parametrize("C", [64, 128])
def test_token_dynamic_range(A, C):
    """Tokens of ONE 32-token tile scaled by powers of two from 2^-12 to 2^12: the per-token scale keeps every token's
    bits.  Per-token rel-L2 against fp64, worst token; the fp32 forms on the same inputs must pass the same check (they
    do on the full range, so it is not narrowed)."""
    afdm, ops, dev = A
    L = afdm.lib()
    B, S = 3, 4                                                   # 48 tokens; tokens 0..31 are the first tile
    g = _g(5 + C)
    P = S * S
    tok_scale = torch.ones(B * P)
    tok_scale[:32] = 2.0 ** (torch.arange(32) * 24 // 31 - 12).float()
    tok_scale = tok_scale[torch.randperm(32, generator=g).tolist() + list(range(32, B * P))]
    sc = tok_scale.reshape(B, 1, S, S)
    mk = lambda *sh: torch.randn(*sh, generator=g)
    x = mk(B, C, S, S) * sc
    gamma, beta, w_in, b_in = 1 + 0.1 * mk(C), 0.1 * mk(C), mk(3 * C, C) / C ** 0.5, 0.1 * mk(3 * C)
    dqkv = mk(B, 3 * C, S, S)
    att = mk(B, C, S, S) * sc
    xres = mk(B, C, S, S)
    wo, w1, w2 = (mk(C, C) / C ** 0.5 for _ in range(3))
    bo, b1, b2, g2, be2 = 0.1 * mk(C), 0.1 * mk(C), 0.1 * mk(C), 1 + 0.1 * mk(C), 0.1 * mk(C)

    def tokens(t):                                                # (B, C', S, S) -> (B, P, C')
        return t.reshape(t.shape[0], t.shape[1], -1).transpose(1, 2)

    def image(t):
        return t.transpose(1, 2).reshape(B, -1, S, S)

    # fp64: head forward / backward, tail forward
    x64 = x.double().requires_grad_(True)
    h64 = F.layer_norm(tokens(x64), (C,), gamma.double(), beta.double(), EPS)
    qkv64 = image(h64 @ w_in.double().T + b_in.double())
    (dx64,) = torch.autograd.grad(qkv64, x64, dqkv.double())
    a64 = tokens(att.double()) @ wo.double().T + bo.double() + tokens(xres.double())
    f64 = F.layer_norm(a64, (C,), g2.double(), be2.double(), EPS)
    out64 = image(F.gelu(f64 @ w1.double().T + b1.double()) @ w2.double().T + b2.double() + a64)

    D = lambda t: t.to(dev).contiguous()
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    res = {}
    for mode in (3, 4):
        with _path(L, mode):
            xd = D(x).requires_grad_(True)
            qkv, _ = ops.AttnHead.apply(xd, D(gamma), D(beta), D(w_in), D(b_in))
            (dx,) = torch.autograd.grad(qkv, xd, D(dqkv))
            t = [D(v) for v in (att, xres, wo, bo, g2, be2, w1, b1, w2, b2)]
            out = torch.empty(B, C, S, S, device=dev)
            L.afd_tok_tail_fwd(*[p(v) for v in t], None, None, None, None, None, p(out), B, C, P, EPS, s)
            torch.cuda.synchronize()
        res[mode] = (_per_token_err(qkv.detach().cpu(), qkv64.detach()), _per_token_err(dx.cpu(), dx64),
                     _per_token_err(out.cpu(), out64))
    for mode, name in ((3, "fp32 forms"), (4, "f16x2")):
        print(f"tok C{C} token range 2^-12..2^12, worst token, {name:10s}: qkv {res[mode][0]:.2e}, dx {res[mode][1]:.2e}, tail out {res[mode][2]:.2e}")
    assert max(res[3]) < TOL, res[3]                              # the inputs are fair: the fp32 forms pass
    assert max(res[4]) < TOL, res[4]


@pytest.mark.parametrize("C", [64, 128])
def test_unaligned_weights(A, C):
    """Every parameter a view at an odd float offset of one flat buffer: the image build assumes no 16-byte alignment.
    The arithmetic does not depend on the addresses, so outputs and dx equal those of aligned copies bit for bit."""
    afdm, ops, dev = A
    L = afdm.lib()
    B, S = 3, 4
    g = _g(9 + C)
    shapes = [(C,), (C,), (3 * C, C), (3 * C,), (C, C), (C,), (C,), (C,), (C, C), (C,), (C, C), (C,)]
    flat = torch.empty(sum(torch.Size(s).numel() + 5 for s in shapes) + 8, device=dev)
    views, off = [], 1
    for sh in shapes:
        n = torch.Size(sh).numel()
        v = flat[off:off + n].view(sh)
        v.copy_((torch.randn(sh, generator=g) / (C ** 0.5 if len(sh) == 2 else 4.0)).to(dev))
        assert v.data_ptr() % 8 == 4
        views.append(v)
        off += n + (2 if n % 2 == 0 else 1)                      # stay on odd offsets
    x = torch.randn(B, C, S, S, generator=g).to(dev)
    dy = torch.randn(B, C, S, S, generator=g).to(dev)

    def run(ps):
        xi = x.clone().requires_grad_(True)
        qkv, xr = ops.AttnHead.apply(xi, *ps[:4])
        att = ops.Attention.apply(qkv, 4)
        y = ops.AttnTail.apply(att, xr, *ps[4:])
        (dx,) = torch.autograd.grad(y, xi, dy)
        return y.detach().cpu(), dx.cpu()

    with _path(L, 4):
        y_u, dx_u = run(views)
        y_a, dx_a = run([v.clone() for v in views])
    assert torch.isfinite(y_u).all() and torch.isfinite(dx_u).all()
    assert torch.equal(y_u, y_a) and torch.equal(dx_u, dx_a)


@pytest.mark.parametrize("C", [64, 128])
def test_special_values(A, C):
    """An all-zero tile and an all-zero token give finite, exactly zero products; one inf in one token reaches that
    token's outputs only."""
    afdm, ops, dev = A
    L = afdm.lib()
    B, S = 5, 4                                                   # 80 tokens: tiles 0, 1 and half of 2
    P = S * S
    g = _g(3 + C)
    mk = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    att, xres = mk(B, C, S, S), mk(B, C, S, S)
    wo, w1, w2 = (mk(C, C) / C ** 0.5 for _ in range(3))
    bo, b1, b2, g2, be2 = 0.1 * mk(C), 0.1 * mk(C), 0.1 * mk(C), 1 + 0.1 * mk(C), 0.1 * mk(C)
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream

    def tail(att_):
        a, f, u, gg, out = (torch.empty_like(att_) for _ in range(5))
        st = torch.empty(B, P, 2, device=dev)
        L.afd_tok_tail_fwd(p(att_), p(xres), p(wo), p(bo), p(g2), p(be2), p(w1), p(b1), p(w2), p(b2), p(a), p(st), p(f), p(u), p(gg),
                           p(out), B, C, P, EPS, s)
        torch.cuda.synchronize()
        return a, out

    tokens = lambda t: t.reshape(B, C, P).transpose(1, 2).reshape(B * P, C)    # copy: (token, channel)
    with _path(L, 4):
        a0, out0 = tail(att)
        az = tokens(att).clone()
        az[32:64] = 0.0                                           # tile 1 all zero
        az[70] = 0.0                                              # and one token of the half-live tile
        att_z = az.reshape(B, P, C).transpose(1, 2).reshape(B, C, S, S).contiguous()
        a, out = tail(att_z)
        assert torch.isfinite(a).all() and torch.isfinite(out).all()
        want = bo[None, :] + tokens(xres)                         # 0 . W_o is exactly zero: a = (0 + b_o) + x
        zero = list(range(32, 64)) + [70]
        assert torch.equal(tokens(a)[zero], want[zero])
        ai = tokens(att).clone()
        ai[37, 5] = float("inf")
        att_i = ai.reshape(B, P, C).transpose(1, 2).reshape(B, C, S, S).contiguous()
        a, out = tail(att_i)
        others = [t for t in range(B * P) if t != 37]
        assert not torch.isfinite(tokens(out)[37]).any()
        assert torch.equal(tokens(out)[others], tokens(out0)[others]) and torch.equal(tokens(a)[others], tokens(a0)[others])
        # backward: a zero tile of dqkv gives dh = 0 exactly
        x, dqkv = mk(B, C, S, S), mk(B, 3 * C, S, S)
        dq = dqkv.reshape(B, 3 * C, P).transpose(1, 2).reshape(B * P, 3 * C).clone()
        dq[0:32] = 0.0
        dqz = dq.reshape(B, P, 3 * C).transpose(1, 2).reshape(B, 3 * C, S, S).contiguous()
        g1, w_in = 1 + 0.1 * mk(C), mk(3 * C, C) / C ** 0.5
        st = torch.stack([x.mean(1).reshape(B, P), (x.var(1, unbiased=False).reshape(B, P) + EPS).rsqrt()], -1).contiguous()
        dres, dh, dx = torch.zeros_like(x), torch.empty_like(x), torch.empty_like(x)
        L.afd_tok_head_bwd(p(dqz), p(x), p(st), p(g1), p(w_in), p(dres), p(dh), p(dx), B, C, P, s)
        torch.cuda.synchronize()
        assert torch.isfinite(dh).all() and torch.isfinite(dx).all()
        assert (tokens(dh)[0:32] == 0).all() and (tokens(dx)[0:32] == 0).all()
