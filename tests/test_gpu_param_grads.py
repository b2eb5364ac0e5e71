"""Parameter gradients in the mode a training step produces them in: ops.inplace_param_grads.  There the kernels ADD
(accumulate = 1) into preallocated `.grad` tensors that are views at arbitrary 4-byte offsets of one flat buffer, the
producers are queued, dealt to one or two side streams and finished by batched afd_fold_batched launches.  The op tests
elsewhere reach the kernels only through torch.autograd.grad: fresh 256-byte-aligned tensors, accumulate = 0, stream order.

Every case of tests/param_grad_cases.py (inputs, fp64 reference and gates live there; tests/test_param_grad_cases_host.py
shows that plain fp32 passes every gate) runs under each queueing configuration of PG.CONFIGS -- no side stream; one side
stream with fold_every 0, 1, 2; two side streams with fold_every 2; batch 1 and 8 -- and once out of place:

  * what backward ADDED to a gradient view pre-filled with g0 = randn * rms(gradient) is the fp64 gradient to 1e-5
    (`=` for `+=` misses by > 0.5), and so is every activation gradient the same backward returns (dx, dres, demb, dtemb);
  * every sentinel in the spacers of both flat buffers is bit-intact, the parameter buffer is unchanged;
  * the whole flat gradient buffer is torch.equal across the configurations: the bits depend neither on the stream count
    nor on how the folds are batched (csrc/fold.hip, LayerNormC.backward);
  * out of place, g0 + dw passes the same gate, and has the very bits of the in-place result wherever `case.oop_equal`.

Which accumulates are ONE final add (read from the kernels; g0 + t in fp32 either way, so in place == out of place + g0 when
both ways sum t in the same order): fold_batched_k (`*o = acc ? *o + t : t`: every matrix-core / Winograd / first-layer 3x3
and 1x1 weight and bias gradient, the GroupNorm / LayerNorm column sums on a side stream), conv_direct_wgrad and
conv_dbias_final (planes the tiler cannot cut), colsum2_k (GroupNorm / LayerNorm without a side stream), fold_param_grads
(the tail of gn_bwd_apply and of the ln_c_bwd_dx kernels), silu_linear_dw_k, embed_add_bwd_k.  That is all of them; no
producer accumulates slab by slab.  The two exceptions to bit equality are in how t is summed, not in the accumulate:
LayerNormC out of place sums the plane partials in the dx kernel's tail in shuffle-tree order, in place in row order (B = 3:
other bits; noted, not asserted), and autograd adds a tied parameter's two gradients before g0 is added (noted).

A 3x3 convolution WITH a bias takes the direct fp32 form with bias slabs whatever afd_conv_wgrad_form says (conv_wgrad_impl:
the matrix-core, Winograd and first-layer forms have no bias row), so the `f16x2 4x4 bias` case pins that path.

Tied parameters (one parameter used twice in one backward) and the fall-backs (a plain tensor as weight, a Parameter without
.grad, SiluLinear without bias) are at the end.  Each case runs once per configuration; nothing is repeated to make a race show."""
import pytest
import torch

import param_grad_cases as PG
from conftest import check, note

pytestmark = pytest.mark.gpu
RESTORE = (0, 34, 8, 80, 60, 74, 84, 92, 64, 96)          # the list of test_conv_fwd_dgrad_wgrad ...
RESTORE_MORE = (78, 88)                                   # ... and the two switches it never moves
FAM = "param grads in place: "


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    from afdm import ops
    return afdm, ops, gpu, [torch.cuda.Stream(), torch.cuda.Stream()]


def _names(cases):
    return [c.name for c in cases]


# ---- the ops on the device ---------------------------------------------------------------------------------------------------
def _fwd(ops, c, P, A, K):
    kind = c.kind
    if kind == "conv":
        y = A["x"]
        for _ in range(K["uses"]):
            y = ops.conv(y, P["w"], P.get("b"))
        return (y,)
    if kind == "conv_cross":
        y = ops.conv(ops.conv(A["x"], P["w1"], P["b2"]), P["w2"], P["b2"])
        return (ops.conv(y, P["w1"], P["b1"]),)
    if kind == "gn1":
        y = A["x"]
        for _ in range(K["uses"]):
            y = ops.GroupNorm1.apply(y, P["gamma"], P["beta"], A.get("res"), A.get("emb"), K["act"])
        return (y,)
    if kind == "gnfa":
        return (ops.GroupNormFiltAct.apply(A["x"], P["gamma"], P["beta"], A.get("res"), ops.Taps(K["ku"]), ops.Taps(K["kd"])),)
    if kind == "lnc":
        return tuple(ops.LayerNormC.apply(A["x"], P["gamma"], P["beta"]))
    if kind == "lnc_tied":
        h, x = ops.LayerNormC.apply(A["x"], P["gamma"], P["beta"])
        y, h2 = ops.LayerNormC.apply(h, P["gamma"], P["beta"])
        return (y + h2 + x,)
    if kind == "attn":
        qkv, xr = ops.AttnHead.apply(A["x"], P["ln_w"], P["ln_b"], P["w_in"], P["b_in"])
        att = ops.Attention.apply(qkv, K["heads"])
        return (ops.AttnTail.apply(att, xr, P["wo"], P["bo"], P["ln2_w"], P["ln2_b"], P["w1"], P["b1"], P["w2"], P["b2"]),)
    if kind == "silu":
        return (ops.SiluLinear.apply(A["temb"] if "temb" in A else K["temb0"], P["w"], P.get("b")),)
    if kind == "silupre":
        outs = []
        for i in range(K["uses"]):
            t = K[f"temb{i}"]
            (o,) = ops.silu_linear_batched(t, [(P["w"], P.get("b"))])
            outs.append(ops.SiluLinearPre.apply(o, t, P["w"], P.get("b")))
        return tuple(outs)
    assert kind == "embed"
    return (ops.EmbedAdd.apply(A["temb"], P["table"], K["labels"]),)


def _device_case(c, dev):
    """the two flat buffers on the device and the Parameters as views of them, homed as training.FlatParams homes them"""
    lay = c.layout
    flat_p, flat_g = lay.fill(c.params).to(dev), lay.fill(c.g0).to(dev)
    assert flat_p.data_ptr() % 16 == 0 and flat_g.data_ptr() % 16 == 0
    P = {}
    for k in c.params:
        q = torch.nn.Parameter(torch.empty(0, device=dev))
        q.data = lay.view(flat_p, k)
        q.grad = lay.view(flat_g, k)
        assert q.data_ptr() % 16 == lay.residue(k) and q.grad.data_ptr() % 16 == lay.residue(k) and q.grad.is_contiguous()
        P[k] = q
    A = {k: v.to(dev).requires_grad_(True) for k, v in c.acts.items()}
    K = {k: (v.to(dev) if isinstance(v, torch.Tensor) and k not in ("ku", "kd") else v) for k, v in c.consts.items()}
    return flat_p, flat_g, P, A, K


def _in_place(ops, c, dev, streams, cfg):
    n_side, fold_every, batch = cfg
    flat_p, flat_g, P, A, K = _device_case(c, dev)
    outs = _fwd(ops, c, P, A, K)
    with ops.inplace_param_grads(streams[:n_side] if n_side else None, batch, fold_every=fold_every):
        with torch.autograd.set_multithreading_enabled(False):                  # on the calling thread, as TrainStep runs it
            torch.autograd.backward(list(outs), [d.to(dev) for d in c.dys])
    torch.cuda.synchronize()
    assert all(P[k].grad.data_ptr() == c.layout.view(flat_g, k).data_ptr() for k in P)          # still the views
    return flat_p.cpu(), flat_g.cpu(), {k: a.grad.cpu() for k, a in A.items()}, [o.detach().cpu() for o in outs]


def _out_of_place(ops, c, dev):
    flat_p, flat_g, P, A, K = _device_case(c, dev)
    outs = _fwd(ops, c, P, A, K)
    leaves = {**P, **A}
    grads = torch.autograd.grad(outs, list(leaves.values()), [d.to(dev) for d in c.dys])
    torch.cuda.synchronize()
    assert torch.equal(flat_g.cpu(), c.layout.fill(c.g0))                       # out of place touches no .grad
    return {k: g.cpu() for k, g in zip(leaves, grads)}


def _gates(c, cfg, flat_p, flat_g, dacts, outs):
    """-> list of failures (strings) of one configuration; every figure goes to the ledger first"""
    lay, (_, g64), bad = c.layout, c.ref, []
    for o, o64 in zip(outs, c.ref[0]):
        e = PG.rel_l2(o, o64)
        note(FAM + c.family + " (forward)", e, (c.name, cfg))
        if not e < PG.TOL:
            bad.append(f"{cfg}: forward {e:.2e}")
    for k in c.params:
        e = PG.rel_l2(PG.accumulated(lay.view(flat_g, k), c.g0[k]), g64[k])
        note(FAM + c.family, e, (c.name, k, cfg))
        if not e < PG.TOL:
            bad.append(f"{cfg}: d{k} added to g0 {e:.2e}")
    for k in c.acts:
        e = PG.rel_l2(dacts[k], g64[k])
        note(FAM + c.family + " (activation gradients)", e, (c.name, k, cfg))
        if not e < PG.TOL:
            bad.append(f"{cfg}: d{k} {e:.2e}")
    if not (lay.sentinels_intact(flat_g) and lay.sentinels_intact(flat_p)):
        bad.append(f"{cfg}: a sentinel was overwritten")
    if not torch.equal(flat_p.view(torch.int32), lay.fill(c.params).view(torch.int32)):
        bad.append(f"{cfg}: the parameter buffer changed")
    return bad


def _case(A, c):
    afdm, ops, dev, streams = A
    L = afdm.lib()
    try:
        for m in c.consts.get("switches", ()):
            L.afd_debug_conv_path(m)
        if c.consts.get("form") is not None:
            assert L.afd_conv_wgrad_form(*c.consts["geom"]) == c.consts["form"], (c.name, L.afd_conv_wgrad_form(*c.consts["geom"]))
        L.afd_debug_tok_path(c.consts.get("tok_path", 0))
        bad, first = [], None
        for cfg in PG.CONFIGS:
            flat_p, flat_g, dacts, outs = _in_place(ops, c, dev, streams, cfg)
            bad += _gates(c, cfg, flat_p, flat_g, dacts, outs)
            if first is None:
                first = flat_g
            elif not torch.equal(first.view(torch.int32), flat_g.view(torch.int32)):
                d = PG.rel_l2(flat_g, first)
                bad.append(f"{cfg}: the gradient buffer differs from {PG.CONFIGS[0]}'s (rel-L2 {d:.2e})")
        oop = _out_of_place(ops, c, dev)
    finally:
        for m in RESTORE + RESTORE_MORE:
            L.afd_debug_conv_path(m)
        L.afd_debug_tok_path(0)
    for k in c.params:
        got = c.g0[k] + oop[k]
        check("param grads out of place, g0 + dw: " + c.family, PG.accumulated(got, c.g0[k]), c.ref[1][k], PG.TOL, (c.name, k))
        inpl = c.layout.view(first, k)
        if c.oop_equal:
            if not torch.equal(got, inpl):
                bad.append(f"out of place: g0 + d{k} has other bits than in place (rel-L2 {PG.rel_l2(got, inpl):.2e})")
        else:
            note("param grads in place vs out of place + g0 (other summation order): " + c.family, PG.rel_l2(got, inpl), (c.name, k))
    for k in c.acts:
        check("param grads out of place, g0 + dw: " + c.family + " (activation gradients)", oop[k], c.ref[1][k], PG.TOL, (c.name, k))
    for line in bad:
        print(f"{c.name}: {line}")
    assert not bad, (c.name, bad)


@pytest.mark.parametrize("name", _names(PG.conv3_cases()))
def test_conv3x3_weight_gradients_in_place(A, name):
    """one case per weight-gradient form (forced by afd_debug_conv_path, asserted by afd_conv_wgrad_form)"""
    _case(A, PG.all_cases()[name])


@pytest.mark.parametrize("name", _names(PG.conv1_cases()))
def test_conv1x1_weight_and_bias_gradients_in_place(A, name):
    """with the matrix-core 1x1 form by rule (88) and off (89); the output layer's (96 + 3)-element pair is the odd-sized one"""
    _case(A, PG.all_cases()[name])


@pytest.mark.parametrize("name", _names(PG.norm_cases()))
def test_norm_parameter_gradients_in_place(A, name):
    _case(A, PG.all_cases()[name])


@pytest.mark.parametrize("name", _names(PG.attn_cases()))
def test_token_chain_parameter_gradients_in_place(A, name):
    """AttnHead -> Attention -> AttnTail: four _linear_grads and two _ln_param_grads producers queued in one backward"""
    _case(A, PG.all_cases()[name])


@pytest.mark.parametrize("name", _names(PG.embed_cases()))
def test_embedding_parameter_gradients_in_place(A, name):
    _case(A, PG.all_cases()[name])


@pytest.mark.parametrize("name", _names(PG.tied_cases()))
def test_tied_parameter_gradients_in_place(A, name, monkeypatch):
    """One parameter used twice in one backward.  Before the rule of ops.deal_lane / ops.fold_batches its two folds could share
    a launch (a non-atomic read-modify-write of one dst from two workgroups) and its two producers two side streams."""
    ops = A[1]
    dealt, deal = [], ops.deal_lane
    monkeypatch.setattr(ops, "deal_lane", lambda *a: dealt.append(deal(*a)) or dealt[-1])
    _case(A, PG.all_cases()[name])
    # the crossed pair really takes the path that orders the side streams against each other (two streams: twice, batch 1 and 8)
    assert sum(conflict for _, conflict in dealt) == (2 if "crossed" in name else 0), dealt


# ---- fall-backs: in the in-place scope, what has no .grad to add into comes back through autograd, as out of place ------------
def _both_ways(ops, dev, streams, build, run):
    """build() -> leaves; run(leaves) -> (outputs, cotangents).  -> gradients out of place, and per configuration the leaves'
    .grad after a backward inside the scope"""
    leaves = build()
    outs, dys = run(leaves)
    want = [g.cpu() for g in torch.autograd.grad(outs, leaves, dys)]
    got = {}
    for n_side, fold_every, batch in ((0, 2, 8), (1, 2, 8), (2, 2, 1)):
        leaves = build()
        outs, dys = run(leaves)
        with ops.inplace_param_grads(streams[:n_side] if n_side else None, batch, fold_every=fold_every):
            with torch.autograd.set_multithreading_enabled(False):
                torch.autograd.backward(outs, dys)
        torch.cuda.synchronize()
        got[(n_side, fold_every, batch)] = [None if t.grad is None else t.grad.cpu() for t in leaves]
    return want, got


_NO_GRAD = ["plain tensors", "Parameters without .grad"]
_PLAIN_BIAS = "Parameter weight with .grad, plain bias"


@pytest.mark.parametrize("name,how", [("conv3x3 direct fp32 ragged K N", h) for h in _NO_GRAD] +
                         [(n, h) for n in ("conv1x1 24to40 8x8 [88]", "conv3x3 f16x2 4x4 bias") for h in _NO_GRAD + [_PLAIN_BIAS]])
def test_conv_without_a_grad_to_add_into_falls_back(A, name, how):
    """ops.conv with a plain leaf tensor as weight (no Parameter: Conv.backward used to reach wp.grad on None), with Parameters
    whose .grad is None, and with a plain tensor as the bias of a Parameter weight: the out-of-place gradients, bit for bit"""
    _, ops, dev, streams = A
    c = PG.all_cases()[name]
    g64 = c.ref[1]
    keys = [k for k in ("x", "w", "b") if k in c.params or k in c.acts]

    def build():
        t = {"x": c.acts["x"].to(dev).requires_grad_(True)}
        for k in c.params:
            v = c.params[k].to(dev)
            if how == "plain tensors" or (k == "b" and how.endswith("plain bias")):
                t[k] = v.requires_grad_(True)
            else:
                t[k] = torch.nn.Parameter(v)
                if how.endswith("plain bias"):
                    t[k].grad = torch.zeros_like(v)
        return [t[k] for k in keys]

    def run(leaves):
        t = dict(zip(keys, leaves))
        return [ops.conv(t["x"], t["w"], t.get("b"))], [c.dys[0].to(dev)]

    want, got = _both_ways(ops, dev, streams, build, run)
    for k, w in zip(keys, want):
        check("param grads, fall-back in the in-place scope: conv", w, g64[k], PG.TOL, (name, how, k))
    for cfg, grads in got.items():
        for k, w, g in zip(keys, want, grads):
            assert g is not None and torch.equal(g, w), (name, how, cfg, k)


@pytest.mark.parametrize("how", ["Parameter with .grad", "Parameter without .grad", "plain tensor"])
@pytest.mark.parametrize("temb_grad", [False, True])
def test_silu_linear_without_bias(A, how, temb_grad):
    """SiluLinear accepts bias = None (afd_silu_linear_fwd / _bwd take NULL); in the in-place scope it used to reach bp.grad on None"""
    _, ops, dev, streams = A
    g = PG.gen(5)
    temb, w, dy = torch.randn(5, 256, generator=g), torch.randn(40, 256, generator=g) / 16, torch.randn(5, 40, generator=g)
    lv = [temb.double().requires_grad_(True), w.double().requires_grad_(True)]
    g64 = torch.autograd.grad(torch.nn.functional.linear(torch.nn.functional.silu(lv[0]), lv[1]), lv, dy.double())

    def build():
        t = temb.to(dev).requires_grad_(temb_grad)
        q = w.to(dev).requires_grad_(True) if how == "plain tensor" else torch.nn.Parameter(w.to(dev))
        if how == "Parameter with .grad":
            q.grad = torch.zeros_like(q)
        return [t, q] if temb_grad else [q]

    def run(leaves):
        t = leaves[0] if temb_grad else temb.to(dev)
        return [ops.SiluLinear.apply(t, leaves[-1], None)], [dy.to(dev)]

    want, got = _both_ways(ops, dev, streams, build, run)
    check("param grads, fall-back in the in-place scope: SiluLinear without bias", want[-1], g64[1], PG.TOL, (how, "dw"))
    if temb_grad:
        check("param grads, fall-back in the in-place scope: SiluLinear without bias", want[0], g64[0], PG.TOL, (how, "dtemb"))
    for cfg, grads in got.items():
        for w_, g_ in zip(want, grads):
            assert g_ is not None and torch.equal(g_, w_), (how, temb_grad, cfg)      # 0 + dw == dw: the same kernel either way


# ---- the activations' side of the weight-gradient entry point ---------------------------------------------------------------
@pytest.mark.parametrize("geom", [(5, 128, 128, 8, 8, 3), (3, 64, 64, 16, 16, 3), (2, 32, 96, 16, 16, 1)], ids=lambda g: "x".join(map(str, g)))
def test_conv_wgrad_with_unaligned_activations_takes_the_scalar_forms(A, geom):
    """The f16x2 / bf16x3 / Winograd weight-gradient kernels stage x and dy with 16-byte loads; afd_conv_wgrad sends an x or dy
    that is not 16-byte aligned (a contiguous view 4 bytes past a boundary) to the fp32 form with scalar loads instead.  The
    shapes are ones whose rule picks a 16-byte form; the result meets the same gate."""
    afdm, ops, dev, _ = A
    L = afdm.lib()
    B, ci, co, H, W, ks = geom
    assert L.afd_conv_wgrad_form(*geom) in (1, 2, 4)
    g = PG.gen(sum(geom))
    x, dy = torch.randn(B, ci, H, W, generator=g), torch.randn(B, co, H, W, generator=g)
    w64 = torch.zeros(co, ci, ks, ks, dtype=torch.float64, requires_grad=True)
    (dw64,) = torch.autograd.grad(torch.nn.functional.conv2d(x.double(), w64, padding=ks // 2), w64, dy.double())

    def at_offset(t):
        buf = torch.full((t.numel() + 4,), PG.SENTINEL, device=dev)
        v = buf[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return buf, v

    (bx, xv), (bd, dv) = at_offset(x), at_offset(dy)
    ws = torch.empty(max(L.afd_conv_wgrad_workspace_bytes(*geom) // 4, 1), device=dev)
    dw = torch.empty(co, ci, ks, ks, device=dev)
    db = torch.empty(co, device=dev) if ks == 1 else None
    L.afd_conv_wgrad(ops._p(xv), ops._p(dv), ops._p(dw), ops._p(db), B, ci, co, H, W, ks, 0, ops._p(ws), ops._stream())
    torch.cuda.synchronize()
    check("conv wgrad with x, dy 4 bytes past a 16-byte boundary", dw.cpu(), dw64, PG.TOL, geom)
    if db is not None:
        check("conv wgrad with x, dy 4 bytes past a 16-byte boundary", db.cpu(), dy.double().sum(dim=(0, 2, 3)), PG.TOL, (geom, "db"))
