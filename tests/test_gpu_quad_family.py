"""The per-row quad kernels (csrc/objective.hip: the objective and learned-variance kernels that walk (row, 256-quad segment)
items, and the gathered noising) through their `ops` wrappers, bit for bit against a restatement in numpy fp32 that calls none
of them: one numpy operation per rounding, every operand a float32.  They share one walk and one set of lane-wise helpers, so
comparing them with each other cannot catch a mistake they share; this can.

Shapes (B, chw) are the smallest at which the walk can go wrong: below one quad, an odd row with a ragged last quad, exactly
one full segment (16-byte form), three segments whose last has threads with 5, 1 and no floats left, more rows than the 1024
workgroups the launch is capped at (so the item loop and mse_final_k's strided loop wrap; scalar and 16-byte form), and a full
segment one float into a larger buffer (an unaligned pointer forces the scalar kernel on a shape that would vectorise).

What goes through device exp / expm1 / tanh / log in fp64 (the hybrid loss's bound and its v-half gradient, the step's noise
scale) cannot be restated bit for bit and is not checked here: tests/test_gpu_lvar.py gates it against fp64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 1000
KINDS = ("eps", "v", "x0")
CASES = [(1, 1, 0), (2, 3, 0), (3, 255, 0), (2, 1024, 0), (2, 2053, 0), (1030, 5, 0), (1030, 8, 0), (2, 1024, 1)]   # (B, chw, offset)
IDS = [f"{b}x{c}+{o}" for b, c, o in CASES]
SCALES = (0.3, 3.0)                     # both branches of the lerp
F = np.float32


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=gpu, variance="learned")
    tab = {k: getattr(diff, k).detach().cpu().numpy() for k in ("alpha", "alpha_hat", "beta")}
    assert all(v.dtype == np.float32 for v in tab.values())
    w = torch.rand(T, generator=torch.Generator().manual_seed(5)) + 0.5
    return afdm.ops, gpu, diff, tab, w.to(gpu), w.numpy()


def _same_bits(got, want):
    got = got.detach().cpu().contiguous().numpy()
    return got.shape == want.shape and got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def _placed(v, dev, off):
    """v on the device, contiguous, `off` elements into a larger buffer (off 0: 16-byte aligned)"""
    v = torch.from_numpy(v) if isinstance(v, np.ndarray) else v
    buf = torch.zeros(v.numel() + off, dtype=v.dtype, device=dev)
    d = buf[off:].view(v.shape)
    d.copy_(v)
    assert d.is_contiguous() and d.data_ptr() % 16 == (d.element_size() * off) % 16
    return d


@pytest.fixture(scope="module")
def lv(A):
    """the learned variance's (T, 3) fp64 table on the device"""
    return A[2].lvar_coefficients().to(A[1]).contiguous()


@pytest.fixture(scope="module")
def inputs():
    """The cases' inputs, each made once and dropped, device copies included, when the module is done"""
    made = {}
    yield made
    made.clear()


def _case(case, dev, _inputs):
    """Host inputs of one case, as numpy, and their device copies; made once.  p2: the (2 B, 2 chw) learned-variance output of a
    guided forward (its first B rows serve the unguided entry points), p: an (B, chw) prediction, t: 1, a mid value and T - 1."""
    if case not in _inputs:
        B, chw, off = case
        g = torch.Generator().manual_seed(100003 * off + 7 * B + chw)
        h = {k: torch.randn(B, chw, generator=g).numpy() for k in ("p", "x0", "eps", "x", "z")}
        h["p2"] = torch.randn(2 * B, 2 * chw, generator=g).numpy()
        h["p2"][:, chw:] = torch.rand(2 * B, chw, generator=g).numpy() * 3.0 - 1.5        # the variance coefficient
        h["t"] = np.array([(1, 500, T - 1)[(b + CASES.index(case)) % 3] for b in range(B)], dtype=np.int64)
        h["img"] = torch.randint(0, B, (B,), generator=g).numpy()
        d = {k: _placed(v, dev, off if v.dtype == np.float32 else 0) for k, v in h.items()}
        d["p2_1"] = _placed(h["p2"][:B], dev, off)
        _inputs[case] = (h, d)
    return _inputs[case]


# ---- the restatement: numpy fp32, one operation per rounding --------------------------------------------------------------------
def _roots(ah):
    ah = np.asarray(ah, dtype=F)
    return np.sqrt(ah), np.sqrt(F(1) - ah)


def _row_roots(tab, t):
    sa, sb = _roots(tab["alpha_hat"][t])
    return sa[:, None], sb[:, None]


def _noised(sa, sb, x, e):
    return sa * x + sb * e


def _eps_of_pred(kind, p, xt, sa, sb):
    if kind == "v":
        return _noised(sa, sb, p, xt)
    if kind == "x0":
        return (xt - sa * p) / sb
    return p.copy()


def _diff(kind, p, x0, e, sa, sb):
    if kind == "v":
        return p - (sa * e - sb * x0)
    return p - (x0 if kind == "x0" else e)


def _lerp(u, c, s):
    """ATen's scalar lerp (aten/src/ATen/native/Lerp.h)"""
    s, d = F(s), c - u
    return u + s * d if abs(s) < F(0.5) else c - d * (F(1) - s)


def _grad_restated(kind, p, h, tab, w, dloss, B, chw):
    """(dloss * (2 / (B chw)) [* w[t_b]]) * (pred - target)"""
    g0 = F(dloss) * (F(2) / F(B * chw))
    g = np.full((B, 1), g0, dtype=F) if w is None else (g0 * w[h["t"]])[:, None]
    return _diff(kind, p, h["x0"], h["eps"], *_row_roots(tab, h["t"])) * g


def _tree(v):
    """block_sum of 256 threads per row of v (n, 256): the xor butterfly 32 .. 1 inside each wave of 64, read at lane 0, then the four
    wave sums added in order from 0.f"""
    v = v.reshape(v.shape[0], 4, 64).copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lanes ^ o]
    s = np.zeros(v.shape[0], dtype=F)
    for wv in range(4):
        s = s + v[:, wv, 0]
    return s


def _loss_restated(kind, p, h, tab, w, B, chw):
    """objective_partial_k and mse_final_k as launched: per-thread sums in item order blockIdx.x, + gridDim.x, ...; per item
    dx^2 (+ dy^2 + dz^2 + dw^2) left to right, then s += w r; the workgroup's tree; mse_final_k's strided per-thread sums of the
    partials, the same tree, times 1 / (B chw)."""
    segs = ((chw + 3) // 4 + 255) // 256
    items = B * segs
    nb = min(items, 1024)
    sa, sb = _row_roots(tab, h["t"])
    d = _diff(kind, p, h["x0"], h["eps"], sa, sb)
    sq = np.zeros((B, segs * 1024), dtype=F)
    sq[:, :chw] = d * d
    sq = sq.reshape(B, segs, 256, 4)
    left = (chw - 4 * (256 * np.arange(segs)[:, None] + np.arange(256)[None, :]))[None]          # (1, segs, 256)
    r = sq[..., 0]
    for i in (1, 2, 3):
        r = np.where(left > i, r + sq[..., i], r)
    wb = np.ones(B, dtype=F) if w is None else w[h["t"]]
    wr = (wb[:, None, None] * r).reshape(items, 256)
    valid = np.broadcast_to(left > 0, (B, segs, 256)).reshape(items, 256)
    s = np.zeros((nb, 256), dtype=F)
    for first in range(0, items, nb):
        n = min(nb, items - first)
        s[:n] = np.where(valid[first:first + n], s[:n] + wr[first:first + n], s[:n])
    part = _tree(s)
    fin = np.zeros(256, dtype=F)
    for first in range(0, nb, 256):
        n = min(256, nb - first)
        fin[:n] = fin[:n] + part[first:first + n]
    out = _tree(fin[None]) * (F(1) / F(B * chw))
    assert out.dtype == np.float32
    return out.reshape(())


def _step_restated(kind, x, c, u, tab, i, s):
    """Ddpm's mean at step i from the prediction c (guided: lerp of the eps of c and u), plus +0: c1 (x - c2 eps_hat) + 0"""
    a, ah = tab["alpha"][i], tab["alpha_hat"][i]
    sa, sb = _roots(ah)
    c1, c2 = F(1) / np.sqrt(a), (F(1) - a) / np.sqrt(F(1) - ah)
    e = _eps_of_pred(kind, c, x, sa, sb)
    if u is not None:
        e = _lerp(_eps_of_pred(kind, u, x, sa, sb), e, s)
    out = c1 * (x - c2 * e) + F(0)
    assert out.dtype == np.float32
    return out


# ---- conversions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("v", "x0"))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pred_to_eps(A, inputs, case, kind):
    ops, dev, diff, tab, _, _ = A
    (B, chw, off), (h, d) = case, _case(case, dev, inputs)
    want = _eps_of_pred(kind, h["p"], h["x"], *_row_roots(tab, h["t"]))
    got = ops.pred_to_eps(d["p"], d["x"], d["t"], diff.alpha_hat, kind)
    assert _same_bits(got, want)
    assert _same_bits(d["p"], h["p"])                          # out of place: the input is left alone
    inplace = _placed(h["p"], dev, off)
    assert ops.pred_to_eps(inplace, d["x"], d["t"], diff.alpha_hat, kind, eps_out=inplace).data_ptr() == inplace.data_ptr()
    assert _same_bits(inplace, want)


@pytest.mark.parametrize("want_v", (False, True))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_split_pred(A, inputs, case, kind, want_v):
    ops, dev, diff, tab, _, _ = A
    (B, chw, off), (h, d) = case, _case(case, dev, inputs)
    want = _eps_of_pred(kind, np.ascontiguousarray(h["p2"][:B, :chw]), h["x"], *_row_roots(tab, h["t"]))
    got = ops.split_pred(d["p2_1"], d["x"], d["t"], diff.alpha_hat, kind, eps_out=_placed(np.zeros_like(want), dev, off), want_v=want_v)
    eps, v = got if want_v else (got, None)
    assert _same_bits(eps, want)
    if want_v:
        assert _same_bits(v, np.ascontiguousarray(h["p2"][:B, chw:]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_noise_images_gather(A, inputs, case):
    ops, dev, diff, tab, _, _ = A
    (B, chw, off), (h, d) = case, _case(case, dev, inputs)
    want = _noised(*_row_roots(tab, h["t"]), h["x0"][h["img"]], h["eps"])
    got = ops.noise_images_gather(d["x0"], d["img"], d["eps"], d["t"], diff.alpha_hat, out=_placed(np.zeros_like(want), dev, off))
    assert _same_bits(got, want)


# ---- the losses -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_objective_loss_forward_and_backward(A, inputs, case, kind, weighted):
    ops, dev, diff, tab, w_d, w = A
    (B, chw, off), (h, d) = case, _case(case, dev, inputs)
    w_d, w = (w_d, w) if weighted else (None, None)
    p = _placed(h["p"], dev, off).requires_grad_(True)
    loss = ops.objective_loss(p, d["x0"], d["eps"], d["t"], diff.alpha_hat, w_d, kind)
    want = _loss_restated(kind, h["p"], h, tab, w, B, chw)
    assert _same_bits(loss, want)
    loss.backward(torch.tensor(3.0, device=dev))
    assert _same_bits(p.grad, _grad_restated(kind, h["p"], h, tab, w, 3.0, B, chw))


@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lvar_loss_simple_part(A, inputs, lv, case, kind, weighted):
    """vlb_scale = 0: L = L_simple + 0 L_vlb exactly, so the loss must be objective_loss's on the prediction half, bit for bit.
    The prediction half of the gradient is L_simple's whatever the scale."""
    ops, dev, diff, tab, w_d, w = A
    (B, chw, off), (h, d) = case, _case(case, dev, inputs)
    w_d, w = (w_d, w) if weighted else (None, None)
    args = (d["x0"], d["eps"], d["t"], diff.alpha, diff.alpha_hat, diff.beta, lv, w_d, kind)
    p_half = np.ascontiguousarray(h["p2"][:B, :chw])
    loss0, vlb = ops.lvar_loss(d["p2_1"], *args, 0.0)
    assert bool(torch.isfinite(vlb))
    simple = ops.objective_loss(_placed(p_half, dev, off), d["x0"], d["eps"], d["t"], diff.alpha_hat, w_d, kind)
    assert torch.equal(loss0.view(torch.int32), simple.view(torch.int32))
    assert _same_bits(loss0, _loss_restated(kind, p_half, h, tab, w, B, chw))
    out2 = _placed(h["p2"][:B], dev, off).requires_grad_(True)
    ops.lvar_loss(out2, *args, 0.5)[0].backward(torch.tensor(3.0, device=dev))
    assert _same_bits(out2.grad[:, :chw], _grad_restated(kind, p_half, h, tab, w, 3.0, B, chw))


# ---- the learned-variance step where it is pure fp32: without noise, and at step 1 ------------------------------------------------
@pytest.mark.parametrize("form", ("host", "dev"))
@pytest.mark.parametrize("guided", (False, True))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_lvar_step_without_noise(A, inputs, lv, case, kind, guided, form):
    ops, dev, diff, tab, _, _ = A
    (B, chw, off), (h, d) = case, _case(case, dev, inputs)
    tabs = (diff.alpha, diff.alpha_hat, diff.beta, lv, kind)
    c, u = np.ascontiguousarray(h["p2"][:B, :chw]), np.ascontiguousarray(h["p2"][B:, :chw])
    for i, z in ((T - 1, None), (500, None), (1, None), (1, d["z"])):
        index = torch.full((1,), i, device=dev, dtype=torch.long) if form == "dev" else i
        x = _placed(h["x"], dev, off)
        out = x if form == "dev" else _placed(np.zeros_like(h["x"]), dev, off)           # the _dev forms run in place
        for s in SCALES if guided else (None,):
            want = _step_restated(kind, h["x"], c, u if guided else None, tab, i, s)
            if guided:
                out2 = _placed(np.full_like(h["x"], np.nan), dev, off)
                got = getattr(ops, "denoise_step_lvar_cfg" + "_dev" * (form == "dev"))(x, d["p2"], z, *tabs, index, s, out, out2)
                assert _same_bits(out2, want), (i, s)
            else:
                got = getattr(ops, "denoise_step_lvar" + "_dev" * (form == "dev"))(x, d["p2_1"], z, *tabs, index, out)
            assert got.data_ptr() == out.data_ptr() and _same_bits(got, want), (i, s, z is not None)
            if form == "dev":
                x.copy_(torch.from_numpy(h["x"]))
