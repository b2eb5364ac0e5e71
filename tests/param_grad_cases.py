"""Cases for the parameter gradients in the in-place mode of a training step (ops.inplace_param_grads), shared by
tests/test_gpu_param_grads.py (the HIP kernels against fp64) and tests/test_param_grad_cases_host.py (torch's CPU fp32
against fp64 on the same inputs under the same gates: the inputs are fair, a gate missed on the device is the kernel's).

What the out-of-place tests (torch.autograd.grad on fresh tensors) cannot see, and every case here has:

  layout     parameters and their gradients are views of two flat fp32 buffers, as training.FlatParams builds them, but
             a spacer of 1, 2 or 3 floats precedes every tensor (one more float leads a buffer whose first tensor is the
             aligned control, 3 follow the last tensor): over the cases of an op the
             data pointers sit 4, 8 and 12 bytes past a 16-byte boundary, and on one (the control).  The spacers of both
             buffers hold SENTINEL; a store past a tensor's end, or a 16-byte store at a rounded-down address, breaks one.
  g0         every gradient view starts as randn * rms(fp64 gradient), not as zeros: `=` instead of `+=` fails the gate.
  reference  plain torch (F.conv2d, F.group_norm, F.layer_norm, F.linear, F.silu, F.gelu, F.embedding) and autograd, in
             float64 on the CPU, with a parameter that is used twice TIED in the reference too.

A case holds CPU fp32 tensors: `params` (they own a slice of the flat buffers), `acts` (inputs that need a gradient: the
same backward returns dx / dres / demb / dtemb, gated like the parameters), `consts`, the cotangents `dys`, and `fwd(P, A, K)`
-> tuple of outputs in whatever dtype P and A have.  All builders are deterministic (seeded torch.Generator)."""
import functools
import math
import zlib

import torch
import torch.nn.functional as F

from oracle import ref_ops as R

TOL = 1e-5                    # the ops' contract (tests/test_gpu_ops.py), for parameters and activations alike
SENTINEL = 7.25               # as the filter guard-band test (test_filt_fast_paths_do_not_write_outside_their_tensors)
CYCLE = (1, 2, 3, 0)          # a tensor's first float, in floats past a 16-byte boundary: 4, 8, 12 bytes, then the control
HEAD, TAIL = 1, 3             # sentinel floats that lead the buffer where the FIRST tensor is the aligned control (a spacer alone cannot put it there), and that follow the last tensor
GN_EPS = LN_EPS = 1e-5


def gen(seed):
    return torch.Generator().manual_seed(seed)


class Layout:
    """Offsets of named tensors in a flat buffer: before each one a spacer of 1..3 floats, chosen so that the tensors take the
    residues of CYCLE in turn, starting at CYCLE[rot] (a residue that would need a spacer of 0 or 4 floats is skipped)."""

    def __init__(self, shapes, rot=0):
        self.head = HEAD if CYCLE[rot % 4] == 0 else 0
        self.slots, end, i = {}, self.head, rot
        for name, shape in shapes.items():
            n = int(math.prod(shape))
            for step in range(4):
                sp = (CYCLE[(i + step) % 4] - end) % 4
                if sp:
                    break
            i += step + 1
            self.slots[name] = (end + sp, n, tuple(shape))
            end += sp + n
        self.numel = end + TAIL

    def residue(self, name):
        """bytes past a 16-byte boundary (of a 16-byte-aligned buffer)"""
        return self.slots[name][0] % 4 * 4

    def view(self, flat, name):
        o, n, shape = self.slots[name]
        return flat[o:o + n].view(shape)

    def fill(self, tensors):
        """new flat CPU buffer: SENTINEL in the spacers, tensors[name] in the slots"""
        flat = torch.full((self.numel,), SENTINEL, dtype=torch.float32)
        for name in self.slots:
            self.view(flat, name).copy_(tensors[name])
        return flat

    def spacers(self):
        m = torch.ones(self.numel, dtype=torch.bool)
        for o, n, _ in self.slots.values():
            m[o:o + n] = False
        return m

    def sentinels_intact(self, flat):
        s = flat.detach().cpu()[self.spacers()]
        return torch.equal(s.view(torch.int32), torch.full_like(s, SENTINEL).view(torch.int32))


class Case:
    def __init__(self, family, name, kind, params, acts, dys, fwd, consts=None, rot=0, tied=False, oop_equal=True):
        self.family, self.name, self.kind = family, name, kind
        self.params, self.acts, self.dys, self.fwd, self.consts = params, acts, dys, fwd, dict(consts or {})
        self.tied = tied
        # out of place (torch.autograd.grad, then g0 + dw) gives the bits of the in-place result; False where it cannot
        # (said at the case): autograd adds a tied parameter's two gradients BEFORE g0, or another kernel sums in another order
        self.oop_equal = oop_equal and not tied
        self.layout = Layout({k: v.shape for k, v in params.items()}, rot)

    def run(self, dtype):
        """-> (outputs, {name: gradient}) of params and acts in `dtype` on the CPU"""
        P = {k: v.to(dtype).requires_grad_(True) for k, v in self.params.items()}
        A = {k: v.to(dtype).requires_grad_(True) for k, v in self.acts.items()}
        K = {k: (v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in self.consts.items()}
        outs = self.fwd(P, A, K)
        leaves = {**P, **A}
        grads = torch.autograd.grad(outs, list(leaves.values()), [d.to(dtype) for d in self.dys])
        return [o.detach() for o in outs], dict(zip(leaves, grads))

    @functools.cached_property
    def ref(self):
        """the fp64 reference, computed once and shared"""
        return self.run(torch.float64)

    @functools.cached_property
    def g0(self):
        """what every gradient view holds before backward: randn * rms(fp64 gradient)"""
        g = gen(zlib.crc32(self.name.encode()))
        return {k: torch.randn(v.shape, generator=g) * float(self.ref[1][k].pow(2).mean().sqrt()) for k, v in self.params.items()}


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def accumulated(got, g0):
    """what backward added to a gradient view that held g0 (both fp32), in fp64: the gate compares THIS with the fp64 gradient"""
    return got.double() - g0.double()


# ---- convolutions ------------------------------------------------------------------------------------------------------------
def _conv_fwd(P, A, K):
    y = A["x"]
    for _ in range(K["uses"]):
        y = F.conv2d(y, P["w"], P.get("b"), padding=K["ks"] // 2)
    return (y,)


def _conv(name, B, ci, co, S, ks, bias, rot, switches=(), form=None, uses=1):
    g = gen(zlib.crc32(name.encode()))
    params = {"w": torch.randn(co, ci, ks, ks, generator=g) / math.sqrt(ci * ks * ks)}
    if bias:
        params["b"] = torch.randn(co, generator=g)
    acts = {"x": torch.randn(B, ci, S, S, generator=g)}
    dys = [torch.randn(B, co, S, S, generator=g)]
    return Case("conv3x3" if ks == 3 else "conv1x1", name, "conv", params, acts, dys, _conv_fwd,
                {"ks": ks, "uses": uses, "switches": tuple(switches), "form": form, "geom": (B, ci, co, S, S, ks)}, rot, tied=uses > 1)


def _conv_cross_fwd(P, A, K):
    """three 1x1 convolutions: (w1, b2), (w2, b2), (w1, b1).  Backward runs them last to first: (w1, b1) and (w2, b2) are dealt
    to two different side streams where there are two, then (w1, b2) writes one gradient of each -- the case ops.deal_lane
    reports as a conflict"""
    y = F.conv2d(A["x"], P["w1"], P["b2"])
    y = F.conv2d(y, P["w2"], P["b2"])
    return (F.conv2d(y, P["w1"], P["b1"]),)


def _conv_cross(name, B, C, S, rot):
    g = gen(zlib.crc32(name.encode()))
    params = {k: (torch.randn(C, C, 1, 1, generator=g) / math.sqrt(C) if k[0] == "w" else torch.randn(C, generator=g)) for k in ("w1", "b1", "w2", "b2")}
    return Case("conv1x1", name, "conv_cross", params, {"x": torch.randn(B, C, S, S, generator=g)}, [torch.randn(B, C, S, S, generator=g)],
                _conv_cross_fwd, {}, rot, tied=True)


# afd_debug_conv_path switches that force each weight-gradient form (afd_conv_wgrad_form says which one a shape takes):
# 85 / 86 = the matrix-core bf16x3 / f16x2 form off / wherever covered, 97 / 98 = Winograd off / wherever covered,
# 78 / 79 = f16x2 / bf16x3 arithmetic.  Form 3 (Cin = 3) is taken by rule.
FORM_SWITCHES = {3: (), 0: (85, 97), 1: (85, 98), 4: (86, 78), 2: (86, 79)}
# (name, B, Cin, Cout, S, bias, form)
CONV3 = [("first layer vector form", 3, 3, 32, 32, False, 3),
         ("direct fp32", 3, 64, 64, 16, False, 0),
         ("winograd", 3, 64, 64, 16, False, 1),
         ("f16x2", 5, 128, 128, 8, False, 4),
         ("f16x2 4x4 bias", 6, 64, 96, 4, True, 4),
         ("bf16x3", 5, 128, 128, 8, False, 2),
         ("direct fp32 ragged K N", 2, 12, 40, 8, False, 0)]
# (name, B, Cin, Cout, S); every one with a bias; each with the matrix-core 1x1 form by rule (88) and off (89)
CONV1 = [("32to96 16x16", 2, 32, 96, 16), ("32to32 4x4", 5, 32, 32, 4), ("24to40 8x8", 2, 24, 40, 8), ("output layer 32to3 32x32", 2, 32, 3, 32)]


def conv3_cases():
    return [_conv(f"conv3x3 {n}", B, ci, co, S, 3, bias, i, FORM_SWITCHES[form], form) for i, (n, B, ci, co, S, bias, form) in enumerate(CONV3)]


def conv1_cases():
    out = []
    for i, (n, B, ci, co, S) in enumerate(CONV1):
        for sw in (88, 89):
            out.append(_conv(f"conv1x1 {n} [{sw}]", B, ci, co, S, 1, True, i + (sw == 89), (sw,)))
    return out


# ---- normalisations ----------------------------------------------------------------------------------------------------------
def _gn(x, gamma, beta):
    return F.group_norm(x, 1, gamma, beta, GN_EPS)


def _gn1_fwd(P, A, K):
    y = A["x"]
    for _ in range(K["uses"]):
        y = _gn(y, P["gamma"], P["beta"])
        if "res" in A:
            y = y + A["res"]
        if K["act"]:
            y = F.gelu(y)
        if "emb" in A:
            y = y + A["emb"][:, :, None, None]
    return (y,)


def _gn1(name, shape, res, emb, act, rot, uses=1):
    g = gen(zlib.crc32(name.encode()))
    B, C = shape[:2]
    params = {"gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g)}
    acts = {"x": torch.randn(shape, generator=g) * 1.7 + 0.3}
    if res:
        acts["res"] = torch.randn(shape, generator=g)
    if emb:
        acts["emb"] = torch.randn(B, C, generator=g)
    return Case("GroupNorm1", name, "gn1", params, acts, [torch.randn(shape, generator=g)], _gn1_fwd, {"act": act, "uses": uses}, rot,
                tied=uses > 1)


def _gnfa_fwd(P, A, K):
    z = _gn(A["x"], P["gamma"], P["beta"])
    if "res" in A:
        z = z + A["res"]
    return (R.filt_act(z, K["ku"], K["kd"]),)


def _gnfa(name, shape, rot):
    g = gen(zlib.crc32(name.encode()))
    C = shape[1]
    k = R.lowpass_kernel(math.pi / 2, 3, 2)
    params = {"gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g)}
    acts = {"x": torch.randn(shape, generator=g) * 2 + 0.5, "res": torch.randn(shape, generator=g)}
    return Case("GroupNormFiltAct", name, "gnfa", params, acts, [torch.randn(shape, generator=g)], _gnfa_fwd, {"ku": k, "kd": k.clone()}, rot)


def _ln(x, gamma, beta):
    B, C, H, W = x.shape
    return F.layer_norm(x.reshape(B, C, H * W).transpose(1, 2), (C,), gamma, beta, LN_EPS).transpose(1, 2).reshape(B, C, H, W)


def _lnc_fwd(P, A, K):
    """(y, x again): the node routes the residual, so backward gets both gradients of x"""
    x = A["x"]
    return _ln(x, P["gamma"], P["beta"]), x.view_as(x)


def _lnc_tied_fwd(P, A, K):
    x = A["x"]
    h = _ln(x, P["gamma"], P["beta"])
    return (_ln(h, P["gamma"], P["beta"]) + h + x,)


def _lnc(name, shape, rot, tied=False):
    g = gen(zlib.crc32(name.encode()))
    C = shape[1]
    params = {"gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g)}
    acts = {"x": torch.randn(shape, generator=g) * 3 + 1}
    dys = [torch.randn(shape, generator=g)] if tied else [torch.randn(shape, generator=g), torch.randn(shape, generator=g)]
    # out of place LayerNormC.backward takes afd_layernorm_c_bwd, whose dx kernel sums the (B, 2, C) plane partials in its
    # tail in shuffle-tree order (fold_param_grads / block_sum); in place the same partials go through colsum2_k or
    # fold_batched_k in row order: for B = 3 that is (p0 + p2) + p1 against (p0 + p1) + p2 -- one final add each, other bits
    return Case("LayerNormC", name, "lnc_tied" if tied else "lnc", params, acts, dys, _lnc_tied_fwd if tied else _lnc_fwd, {}, rot,
                tied=tied, oop_equal=shape[0] <= 2)


# ---- the token chains of the attention block: AttnHead -> Attention -> AttnTail ----------------------------------------------
ATTN_PARAMS = ("ln_w", "ln_b", "w_in", "b_in", "wo", "bo", "ln2_w", "ln2_b", "w1", "b1", "w2", "b2")


def _attn_fwd(P, A, K):
    x, heads = A["x"], K["heads"]
    B, C, H, W = x.shape
    L, d = H * W, C // heads
    tok = x.reshape(B, C, L).transpose(1, 2)
    qkv = F.linear(F.layer_norm(tok, (C,), P["ln_w"], P["ln_b"], LN_EPS), P["w_in"], P["b_in"])
    sh = lambda z: z.reshape(B, L, heads, d).transpose(1, 2)
    q, k, v = qkv.split(C, dim=-1)
    att = torch.softmax((sh(q) / math.sqrt(d)) @ sh(k).transpose(-1, -2), dim=-1) @ sh(v)
    a = F.linear(att.transpose(1, 2).reshape(B, L, C), P["wo"], P["bo"]) + tok
    f = F.gelu(F.linear(F.layer_norm(a, (C,), P["ln2_w"], P["ln2_b"], LN_EPS), P["w1"], P["b1"]))
    return ((F.linear(f, P["w2"], P["b2"]) + a).transpose(1, 2).reshape(B, C, H, W),)


def _attn(name, B, C, S, tok_path, rot):
    g = gen(zlib.crc32(f"attn {B} {C} {S}".encode()))                       # (the same inputs under both settings of the switch)
    r = lambda *s: torch.randn(*s, generator=g)
    lin = lambda n, k: r(n, k) / math.sqrt(k)
    params = {"ln_w": 1 + 0.1 * r(C), "ln_b": 0.1 * r(C), "w_in": lin(3 * C, C), "b_in": 0.1 * r(3 * C), "wo": lin(C, C), "bo": 0.1 * r(C),
              "ln2_w": 1 + 0.1 * r(C), "ln2_b": 0.1 * r(C), "w1": lin(C, C), "b1": 0.1 * r(C), "w2": lin(C, C), "b2": 0.1 * r(C)}
    return Case("AttnHead + AttnTail", name, "attn", params, {"x": r(B, C, S, S)}, [r(B, C, S, S)], _attn_fwd,
                {"heads": 4, "tok_path": tok_path}, rot)


# ---- the embedding ops -------------------------------------------------------------------------------------------------------
def _silu_fwd(P, A, K):
    outs = []
    for i in range(K["uses"]):
        t = A["temb"] if "temb" in A else K[f"temb{i}"]
        outs.append(F.linear(F.silu(t), P["w"], P.get("b")))
    return tuple(outs)


def _silu(name, kind, N, temb_grad, rot, uses=1, bias=True, Bt=5, Kt=256):
    g = gen(zlib.crc32(name.encode()))
    params = {"w": torch.randn(N, Kt, generator=g) / math.sqrt(Kt)}
    if bias:
        params["b"] = torch.randn(N, generator=g)
    tembs = [torch.randn(Bt, Kt, generator=g) for _ in range(uses)]
    acts = {"temb": tembs[0]} if temb_grad else {}
    consts = {"uses": uses, **({} if temb_grad else {f"temb{i}": t for i, t in enumerate(tembs)})}
    return Case("SiluLinear" if kind == "silu" else "SiluLinearPre", name, kind, params, acts, [torch.randn(Bt, N, generator=g) for _ in range(uses)],
                _silu_fwd, consts, rot, tied=uses > 1)


EMBED_LABELS = (3, 0, 3, -1, 9, 3, 5)           # B = 7 of K = 10 classes: class 3 three times, one null label (no embedding, no gradient)


def _embed_fwd(P, A, K):
    y = K["labels"]
    rows = F.embedding(y.clamp(min=0), P["table"]) * (y >= 0).to(P["table"].dtype)[:, None]
    return (A["temb"] + rows,)


def _embed(rot):
    g = gen(77)
    Bt, Kc, D = len(EMBED_LABELS), 10, 256
    return Case("EmbedAdd", f"EmbedAdd B7 K10 D256 at {4 * CYCLE[rot]} bytes", "embed", {"table": torch.randn(Kc, D, generator=g)}, {"temb": torch.randn(Bt, D, generator=g)},
                [torch.randn(Bt, D, generator=g)], _embed_fwd, {"labels": torch.tensor(EMBED_LABELS)}, rot)


# ---- the lists ----------------------------------------------------------------------------------------------------------------
def norm_cases():
    return [_gn1("GroupNorm1 3x32x16x16 res emb gelu", (3, 32, 16, 16), True, True, 1, 0),
            _gn1("GroupNorm1 2x5x3x3", (2, 5, 3, 3), False, False, 0, 2),
            _gnfa("GroupNormFiltAct 3x32x16x16 sample-resident", (3, 32, 16, 16), 0),
            _gnfa("GroupNormFiltAct 2x6x6x10 stats + act", (2, 6, 6, 10), 2),
            _lnc("LayerNormC 3x64x16x16", (3, 64, 16, 16), 0),
            _lnc("LayerNormC 1x12x3x5", (1, 12, 3, 5), 2)]


def attn_cases():
    return [_attn(f"attn B{B} C{C} {S}x{S} tok_path {tp}", B, C, S, tp, rot) for rot, (B, C, S) in enumerate([(3, 64, 8), (5, 128, 4)]) for tp in (0, 3)]


def embed_cases():
    out = []
    for i, N in enumerate((32, 96)):
        out.append(_silu(f"SiluLinear N{N} temb grad", "silu", N, True, i))
        out.append(_silu(f"SiluLinear N{N}", "silu", N, False, i + 2))
        # (silu_linear_batched, whose value SiluLinearPre hands on, takes a time embedding that needs NO gradient: its contract)
        out.append(_silu(f"SiluLinearPre N{N}", "silupre", N, False, 2 * i))
    return out + [_embed(rot) for rot in range(4)]                # (its one tensor at each of the four offsets)


def tied_cases():
    return [_conv("tied conv3x3 64to64 16x16", 3, 64, 64, 16, 3, False, 1, uses=2),
            _conv("tied conv1x1 bias 32to32 8x8", 3, 32, 32, 8, 1, True, 0, uses=2),
            _gn1("tied GroupNorm1 3x32x16x16", (3, 32, 16, 16), False, False, 1, 3, uses=2),
            _lnc("tied LayerNormC 3x64x16x16", (3, 64, 16, 16), 1, tied=True),
            _silu("tied SiluLinearPre N32", "silupre", 32, False, 1, uses=2),
            _conv_cross("tied conv1x1 crossed weight and bias 32to32 8x8", 3, 32, 8, 2)]


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = conv3_cases() + conv1_cases() + norm_cases() + attn_cases() + embed_cases() + tied_cases()
    assert len({c.name for c in cases}) == len(cases)
    return {c.name: c for c in cases}


# ---- the queueing configurations of ops.inplace_param_grads: (side streams, fold_every, batch) -------------------------------
CONFIGS = [(0, 2, 8)] + [(1, fe, b) for fe in (0, 1, 2) for b in (1, 8)] + [(2, 2, b) for b in (1, 8)]
