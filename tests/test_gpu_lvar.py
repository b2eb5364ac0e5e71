"""Learned reverse-process variances on the GPU: the hybrid loss (forward / backward), the bound's terms, the ancestral step
kernels and the output split against the fp64 restatement of tests/lvar_oracle.py; TrainStep, the DDPM chain, calc_bpd and
ddpm_run on a UNet(c_out=2 C)."""
import math
import os

import numpy as np
import pytest
import torch

import lvar_oracle as O
from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
GATE = 1e-5                  # the project's per-op rel-L2 gate
STEP_GATE = 1e-6             # the samplers' updates against fp64
KINDS = ("eps", "v", "x0")
SHAPES = ((1, 1), (3, 255), (4, 3072))
T = 1000


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _model(afdm, dev, seed=42, num_classes=None, c_out=6):
    afdm.set_seed(seed)
    kw = {} if num_classes is None else {"num_classes": num_classes}
    return afdm.UNet(c_in=3, c_out=c_out, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, **kw).to(dev)


def _placed(x, dev, shift):
    """x on the device as a contiguous view that starts `shift` floats into its buffer (shift 0: 16-byte aligned)."""
    buf = torch.empty(x.numel() + 4, device=dev, dtype=torch.float32)
    v = buf[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * shift
    return v


def _tables(diff):
    return diff.beta, diff.alpha, diff.alpha_hat


def _loss(afdm, diff, o_d, x_d, e_d, t_d, w_d, kind, scale):
    return afdm.ops.lvar_loss(o_d, x_d, e_d, t_d, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), w_d, kind, scale, return_sums=True)


# ---- the hybrid loss against fp64 autograd -------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule", ("linear", "cosine"))
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_lvar_loss_against_fp64(A, kind, weighted, schedule):
    afdm, dev = A
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, schedule=schedule, prediction=kind, variance="learned")
    w = diff.snr_weights("min_snr", 5.0).float() if weighted else None
    w_d = None if w is None else w.to(dev)
    scale = 0.001 * (T - 1)
    for B, chw in SHAPES:
        out2, x0, eps, t = O.case(B, chw, T, 7 * B + chw, _tables(diff), kind)
        assert B < 3 or {1, 2, T - 1} <= set(t.tolist())
        want = O.hybrid(*_tables(diff), kind, out2, x0, eps, t, w, scale, dev=dev)
        t_d = t.to(dev)
        got = {}
        for shift in (0, 1):
            o_d = _placed(out2, dev, shift).requires_grad_(True)
            x_d, e_d = _placed(x0, dev, shift), _placed(eps, dev, shift)
            runs = []
            for _ in range(2):
                o_d.grad = None
                loss, vlb, sums = _loss(afdm, diff, o_d, x_d, e_d, t_d, w_d, kind, scale)
                loss.backward()
                runs.append((loss.detach().clone(), vlb.clone(), sums.clone(), o_d.grad.clone()))
            assert all(torch.equal(a, b) for a, b in zip(*runs))                       # identical bytes run to run
            got[shift] = runs[0]
            loss, vlb, sums, grad = (v.cpu() for v in runs[0])
            tag = f"{kind} w={weighted} {schedule} B={B} chw={chw} shift={shift}"
            check("lvar loss: L vs fp64", loss.reshape(1), want["L"].reshape(1), GATE, tag)
            check("lvar loss: L_vlb vs fp64", vlb.reshape(1), want["L_vlb"].reshape(1), GATE, tag)
            check("lvar loss: L_vlb (fp64 output) vs fp64", sums[1:], want["L_vlb"].reshape(1), 1e-9, tag)
            check("lvar loss: dp vs fp64", grad[:, :chw], want["dp"], GATE, tag)
            check("lvar loss: dv vs fp64", grad[:, chw:], want["dv"], GATE, tag)
            # dp is the objective loss's gradient, bit for bit (the mean is stopped in L_vlb)
            p_d = _placed(out2[:, :chw].contiguous(), dev, shift).requires_grad_(True)
            afdm.ops.objective_loss(p_d, x_d, e_d, t_d, diff.alpha_hat, w_d, kind).backward()
            assert torch.equal(runs[0][3][:, :chw], p_d.grad), tag
        assert all(torch.equal(a, b) for a, b in zip(got[0], got[1]))                  # vector path == scalar path
    # dloss scales both halves of the gradient (the kernel reads it from the device)
    o_d = out2.to(dev).requires_grad_(True)
    (_loss(afdm, diff, o_d, x0.to(dev), eps.to(dev), t_d, w_d, kind, scale)[0] * 3.0).backward()
    check("lvar loss: dv vs fp64", o_d.grad.cpu()[:, chw:], 3.0 * want["dv"], GATE, f"{kind} dloss=3")
    check("lvar loss: dp vs fp64", o_d.grad.cpu()[:, :chw], 3.0 * want["dp"], GATE, f"{kind} dloss=3")


@pytest.mark.parametrize("shape", ((5, 255), (8, 3072)))
def test_lvar_loss_decoder_rows_cover_edge_bins_and_the_clamp(A, shape):
    """Every row is a decoder row (t = 1); tests/test_lvar_host.py checks the same inputs' coverage on the CPU."""
    afdm, dev = A
    rows, chw = shape
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, variance="learned")
    out2, x0, eps, t = O.decoder_case(rows, chw, 11)
    scale = 0.999
    want = O.hybrid(*_tables(diff), "eps", out2, x0, eps, t, None, scale, dev=dev)
    cl, lo, hi = want["clamped"], x0 < -0.999, x0 > 0.999
    assert int((cl & lo).sum()) > 0 and int((cl & hi).sum()) > 0 and int((~cl & lo).sum()) > 0 and int((~cl & hi).sum()) > 0
    assert int(cl.sum()) > 100 and int((~cl).sum()) > 100
    o_d = out2.to(dev).requires_grad_(True)
    loss, vlb, sums = _loss(afdm, diff, o_d, x0.to(dev), eps.to(dev), t.to(dev), None, "eps", scale)
    loss.backward()
    dv = o_d.grad.cpu()[:, chw:]
    assert bool((dv[cl] == 0).all())                                                   # exactly zero under the clamp, as torch.clamp
    assert bool((dv[~cl] != 0).any())
    check("lvar loss: decoder rows, L_vlb vs fp64", sums.cpu()[1:], want["L_vlb"].reshape(1), 1e-9, shape)
    check("lvar loss: decoder rows, dv vs fp64", dv, want["dv"], GATE, shape)


# ---- the bound's terms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ((1, 1), (5, 255), (8, 3072)))
def test_vlb_terms_lvar_against_fp64(A, shape, kind):
    afdm, dev = A
    from afdm import ops
    rows, per = shape
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, prediction=kind, variance="learned")
    out2, x0, eps, t = O.case(rows, per, T, 5 * rows + per, _tables(diff), kind)
    if rows >= 5:
        d2, dx, de, _ = O.decoder_case(1, per, 2)                   # one decoder row with the clamp and the edge bins in it
        if kind == "eps":
            out2[3], x0[3], eps[3], t[3] = d2[0], dx[0], de[0], 1
    img = torch.arange(rows)                                        # the gather: row r scores image rows - 1 - r
    x0_img = x0.flip(0).contiguous()
    img = (rows - 1 - img).contiguous()
    t_d, i_d = t.to(dev), img.to(dev)
    xt = ops.noise_images_gather(x0_img.to(dev), i_d, eps.to(dev), t_d, diff.alpha_hat)
    want = O.hybrid(*_tables(diff), kind, out2, x0, eps, t, xt=xt, dev=dev)
    args = (x0_img.to(dev), i_d, xt, eps.to(dev), out2.to(dev), t_d, diff._lv(), diff.alpha, diff.alpha_hat, diff.beta, kind)
    term, sq = ops.vlb_terms_lvar(*args)
    term2, sq2 = ops.vlb_terms_lvar(*args)
    assert torch.equal(term, term2) and torch.equal(sq, sq2)        # deterministic
    got, got_sq = term.cpu(), sq.cpu()
    dec = t == 1
    rel = (got - want["term"]).abs() / want["term"].abs()
    rel_sq = (got_sq - want["sq"]).abs() / want["sq"].abs()
    kl_worst = float(rel[~dec].max()) if bool((~dec).any()) else 0.0
    dec_worst = float(rel[dec].max()) if bool(dec.any()) else 0.0
    note("lvar bound: KL rows vs fp64 (relative, per row)", kl_worst, (shape, kind))
    note("lvar bound: decoder rows vs fp64 (relative, per row)", dec_worst, (shape, kind))
    print(f"lvar terms vs fp64 {shape} {kind}: KL worst {kl_worst:.2e}, decoder worst {dec_worst:.2e}, sq worst {float(rel_sq.max()):.2e}")
    assert kl_worst < 1e-12 and float(rel_sq.max()) < 1e-12         # tests/test_gpu_bpd.py's gates
    assert dec_worst < 1e-10
    # the training loss reports the same bound: sum term / (N ln 2) == L_vlb of the loss kernel on the same inputs
    _, _, sums = _loss(afdm, diff, out2.to(dev), x0.to(dev), eps.to(dev), t_d, None, kind, 0.5)
    from_terms = float(got.sum()) / (rows * per * math.log(2.0))
    e = abs(float(sums[1]) - from_terms) / abs(from_terms)
    note("lvar bound: sum of terms vs the loss kernel's L_vlb (relative)", e, (shape, kind))
    assert e < 1e-12, (shape, kind, e)


# ---- the ancestral step ---------------------------------------------------------------------------------------------------------
def _step_case(B, chw, seed, rows2=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, chw, generator=g)
    out2 = torch.randn(rows2 * B, 2 * chw, generator=g)
    out2[:, chw:] = torch.rand(rows2 * B, chw, generator=g) * 3.0 - 1.5
    return x, out2, torch.randn(B, chw, generator=g)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("schedule", ("linear", "cosine"))
def test_lvar_step_kernels_against_fp64(A, kind, schedule):
    """Steps T - 1, 500, 2 and 1.  On the cosine schedule alpha[T - 1] = 0.001, and for a v- or x0-prediction eps_hat is x_t plus a
    small term, so the fixed fp32 mean c1 (x - c2 eps_hat) (afd_denoise_step's, not changed here) cancels to about alpha |x|: its
    fp32 roundings, 6e-8 |x| each, are amplified by c1 / 1 = 32 to a few 1e-6 of the output, above this gate whatever the variance
    does.  Those two kinds are therefore checked at 900 in place of T - 1 there (alpha = 0.97); the eps kind keeps T - 1."""
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, schedule=schedule, prediction=kind, variance="learned")
    tabs = (diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), kind)
    for B, chw in SHAPES:
        for i in (900 if schedule == "cosine" and kind != "eps" else T - 1, 500, 2, 1):
            i_dev = torch.full((B,), i, device=dev, dtype=torch.long)
            for shift in (0, 1):
                x, out2, z = _step_case(B, chw, B + chw + i)
                x_d, o_d, z_d = (_placed(v, dev, shift) for v in (x, out2, z))
                want = O.step64(*_tables(diff), kind, x, out2, z, i).float()
                got = ops.denoise_step_lvar(x_d, o_d, z_d, *tabs, i, out=_placed(torch.zeros_like(x), dev, shift))
                tag = f"{kind} {schedule} B={B} chw={chw} i={i} shift={shift}"
                check("lvar step vs fp64", got.cpu(), want, STEP_GATE, tag)
                got_dev = ops.denoise_step_lvar_dev(x_d, o_d, z_d, *tabs, i_dev, _placed(torch.zeros_like(x), dev, shift))
                assert torch.equal(got, got_dev), tag
                if shift == 0:
                    first = got.clone()
                else:
                    assert torch.equal(got, first), tag                                # vector path == scalar path
                if i == 1:                                                             # no noise at the last step; None is accepted
                    assert torch.equal(got, ops.denoise_step_lvar(x_d, o_d, None, *tabs, 1)), tag
                    assert torch.equal(got, ops.denoise_step_lvar(x_d, o_d, z_d * 7.0, *tabs, 1)), tag
                # guided: 2 B rows, the eps of the two halves lerped, the variance from the conditional rows
                for s in (0.3, 3.0):
                    xg, og, zg = _step_case(B, chw, B + chw + i + 1, rows2=2)
                    xg_d, og_d, zg_d = (_placed(v, dev, shift) for v in (xg, og, zg))
                    want = O.step64(*_tables(diff), kind, xg, og, zg, i, cfg_scale=s).float()
                    both = _placed(torch.zeros(2 * B, chw), dev, shift)
                    got = ops.denoise_step_lvar_cfg(xg_d, og_d, zg_d, *tabs, i, s, both[:B], both[B:])
                    check("guided lvar step vs fp64", got.cpu(), want, STEP_GATE, f"{tag} s={s}")
                    assert torch.equal(both[:B], both[B:])                             # x_out2 receives the same values
                    inplace = xg_d.clone() if shift == 0 else _placed(xg, dev, shift)
                    ops.denoise_step_lvar_cfg_dev(inplace, og_d, zg_d, *tabs, i_dev, s, inplace)      # x_out is x
                    assert torch.equal(inplace, got), tag


def test_lvar_step_with_v_one_is_the_fixed_step(A):
    """v = +1 everywhere: logvar = log beta_t, so the step is afd_denoise_step's up to the noise scale (float)exp(log(beta) / 2)
    against sqrtf(beta): at most one fp32 ulp of sqrt(beta) apart, which moves the noise term by 2^-23 |sqrt(beta) z| plus its
    own rounding and the sum's: |out - fixed| <= 2^-22 |sqrt(beta) z| + 2^-23 |fixed|.  The mean is bit-identical (i = 1)."""
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, variance="learned")
    x, out2, z = _step_case(4, 3072, 3)
    out2[:, 3072:] = 1.0
    x_d, o_d, z_d = x.to(dev), out2.to(dev), z.to(dev)
    eps_d = o_d[:, :3072].contiguous()
    worst = 0.0
    for i in (T - 1, 500, 2, 1):
        got = ops.denoise_step_lvar(x_d, o_d, z_d if i > 1 else None, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), "eps", i)
        fixed = ops.denoise_step(x_d, eps_d, z_d if i > 1 else None, diff.alpha, diff.alpha_hat, diff.beta, i)
        if i == 1:
            assert torch.equal(got, fixed)
            continue
        nz = (torch.sqrt(diff.beta[i]) * z_d).abs()
        bound = 1.01 * (2.0 ** -22 * nz + 2.0 ** -23 * fixed.abs())
        assert bool(((got - fixed).abs() <= bound).all()), i
        worst = max(worst, float(((got - fixed).abs() / nz.clamp_min(1e-30)).max()))
    note("lvar step with v = +1 vs the fixed step (max |diff| / |noise term|)", worst)


def test_split_pred_is_the_slice_and_pred_to_eps(A):
    afdm, dev = A
    from afdm import ops
    for kind in KINDS:
        diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, prediction=kind, variance="learned")
        for (B, chw), shift in ((s, sh) for s in SHAPES for sh in (0, 1)):
            g = torch.Generator().manual_seed(B + chw)
            out2, xt = torch.randn(B, 2 * chw, generator=g), torch.randn(B, chw, generator=g)
            t_d = torch.randint(1, T, (B,), generator=g).to(dev)
            o_d, x_d = _placed(out2, dev, shift), _placed(xt, dev, shift)
            eps, v = ops.split_pred(o_d, x_d, t_d, diff.alpha_hat, kind, want_v=True)
            p = o_d[:, :chw].contiguous()
            want = p if kind == "eps" else ops.pred_to_eps(p, x_d.contiguous(), t_d, diff.alpha_hat, kind)
            assert torch.equal(eps, want) and torch.equal(v, o_d[:, chw:]), (kind, B, chw, shift)
            assert torch.equal(ops.split_pred(o_d, x_d, t_d, diff.alpha_hat, kind), want)


def test_lvar_kernels_reject_bad_arguments_and_write_nothing(A):
    afdm, dev = A
    lib = afdm.lib()
    p = lambda v: v.data_ptr()
    diff = afdm.Diffusion(noise_steps=5, img_size=32, device=dev, variance="learned")
    lv = diff._lv()
    al, ah, be = diff.alpha, diff.alpha_hat, diff.beta
    B, chw = 3, 8
    out2 = torch.zeros(2 * B, 2 * chw, device=dev)              # (the guided steps read 2 B rows, everything else the first B)
    x0, eps, x = torch.zeros(B, chw, device=dev), torch.zeros(B, chw, device=dev), torch.zeros(B, chw, device=dev)
    t = torch.full((B,), 2, dtype=torch.long, device=dev)
    img = torch.zeros(B, dtype=torch.long, device=dev)
    nan32 = torch.full((4096 + 64,), float("nan"), device=dev)
    nan64 = torch.full((64,), float("nan"), dtype=torch.float64, device=dev)
    loss, sums, ws, dout, xo = nan32[:2], nan64[:2], nan32[64:], nan32[64:64 + 2 * B * chw], nan32[64:64 + B * chw]
    E = afdm.AfdError

    def fwd(o=out2, x0_=x0, kind=0, lo=loss, w=ws, B_=B, scale=0.5):
        lib.afd_lvar_loss_fwd(p(o) if o is not None else None, p(x0_), p(eps), p(t), p(al), p(ah), p(be), p(lv), None, kind, scale,
                              p(lo), p(sums), p(w), B_, chw, None)

    def bwd(o=out2, d=dout, kind=0, B_=B):
        lib.afd_lvar_loss_bwd(p(o), p(x0), p(eps), p(t), p(al), p(ah), p(be), p(lv), None, kind, 0.5, p(loss), p(d) if d is not None else None,
                              B_, chw, None)

    def step(name, o=out2, xo_=xo, x_=x, kind=0, B_=B, nz=None, xo2=None):
        cfg, dev_ = "cfg" in name, name.endswith("dev")
        a = [p(x_), p(o), nz, p(al), p(ah), p(be), p(lv), kind, p(t) if dev_ else 2]
        a += [1.5, p(xo_), xo2] if cfg else [p(xo_)]
        getattr(lib, name)(*a, B_, chw, None)

    with pytest.raises(E, match="positive"):
        fwd(B_=0)
    with pytest.raises(E, match="kind"):
        fwd(kind=3)
    with pytest.raises(E, match="NULL"):
        fwd(o=None)
    with pytest.raises(E, match="vlb_scale"):
        fwd(scale=float("nan"))
    with pytest.raises(E, match="must not overlap"):
        fwd(lo=x0)
    with pytest.raises(E, match="must not overlap"):
        fwd(w=out2)
    with pytest.raises(E, match="positive"):
        bwd(B_=-1)
    with pytest.raises(E, match="kind"):
        bwd(kind=-1)
    with pytest.raises(E, match="NULL"):
        bwd(d=None)
    with pytest.raises(E, match="must not overlap"):
        bwd(d=out2)
    for name in ("afd_denoise_step_lvar", "afd_denoise_step_lvar_dev", "afd_denoise_step_lvar_cfg", "afd_denoise_step_lvar_cfg_dev"):
        with pytest.raises(E, match="positive"):
            step(name, B_=0)
        with pytest.raises(E, match="kind"):
            step(name, kind=7)
        with pytest.raises(E, match="overlap"):
            step(name, xo_=out2)                                             # the output over the network's output
        with pytest.raises(E, match="overlap"):
            step(name, nz=p(xo))                                             # ... over the noise
        with pytest.raises(E, match="overlap"):
            step(name, x_=nan32[64 + 4:])                                    # a partial overlap with x (x itself is allowed)
    with pytest.raises(E, match="overlap"):
        step("afd_denoise_step_lvar_cfg", xo2=p(xo))                          # x_out2 over x_out
    with pytest.raises(E, match="overlap"):
        step("afd_denoise_step_lvar_cfg", xo2=p(x))                           # x_out2 over x
    with pytest.raises(E, match="i >= 1"):
        lib.afd_denoise_step_lvar(p(x), p(out2), None, p(al), p(ah), p(be), p(lv), 0, 0, p(xo), B, chw, None)
    with pytest.raises(E, match="positive"):
        lib.afd_split_pred(p(out2), p(x), p(t), p(ah), 1, p(xo), None, B, 0, None)
    with pytest.raises(E, match="kind"):
        lib.afd_split_pred(p(out2), p(x), p(t), p(ah), 5, p(xo), None, B, chw, None)
    with pytest.raises(E, match="NULL"):
        lib.afd_split_pred(p(out2), None, p(t), p(ah), 1, p(xo), None, B, chw, None)
    with pytest.raises(E, match="must not overlap"):
        lib.afd_split_pred(p(out2), p(x), p(t), p(ah), 1, p(out2), None, B, chw, None)
    with pytest.raises(E, match="must not overlap"):
        lib.afd_split_pred(p(out2), p(x), p(t), p(ah), 1, p(xo), p(xo), B, chw, None)
    terms = lambda term, sq, rows=B, kind=0: lib.afd_vlb_terms_lvar(p(x0), B, p(img), p(x), p(eps), p(out2), p(t), p(lv), 5, p(al), p(ah),
                                                                    p(be), kind, term, sq, rows, chw, None)
    with pytest.raises(E, match="term and sq must not overlap"):
        terms(p(nan64), p(nan64) + 16)
    with pytest.raises(E, match="term and sq must not overlap"):
        terms(p(lv), p(nan64))
    with pytest.raises(E, match="positive"):
        terms(p(nan64), p(nan64) + 256, rows=0)
    with pytest.raises(E, match="kind"):
        terms(p(nan64), p(nan64) + 256, kind=9)
    with pytest.raises(E, match="NULL"):
        terms(None, p(nan64))
    torch.cuda.synchronize()
    assert bool(torch.isnan(nan32).all()) and bool(torch.isnan(nan64).all())
    assert bool((lv.cpu() == diff.lvar_coefficients()).all())
    assert all(bool((v == 0).all()) for v in (out2, x0, eps, x))
    # the Python layer names the two channel counts
    with pytest.raises(E, match=r"6 channels, the prediction's 3 and the variance coefficient's 3"):
        afdm.ops.lvar_loss(torch.zeros(2, 3, 4, 4, device=dev), torch.zeros(2, 3, 4, 4, device=dev), torch.zeros(2, 3, 4, 4, device=dev),
                           t[:2], al, ah, be, lv)


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _batch(dev, B=16, seed=0, labels=False):
    g = torch.Generator().manual_seed(seed)
    images = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    steps = [(torch.randint(1, T, (B,), generator=g), torch.randn(B, 3, 32, 32, generator=g).to(dev)) for _ in range(3)]
    y = torch.randint(0, 5, (B,), generator=g) if labels else None
    return images, steps, y


def _torch_hybrid(diff, out, images, eps, t_d, w, scale):
    """The hybrid loss in torch ops on the device (fp32 autograd through `out`), KL rows only (the batch holds no t = 1)."""
    C = images.shape[1]
    p, v = out[:, :C], out[:, C:]
    target = diff.training_target(images, eps, t_d)
    l_simple = (w[t_d][:, None, None, None] * (p - target) ** 2).mean()
    tab = diff.lvar_coefficients().to(out.device)
    lb, lbt, kt = (tab[t_d, i][:, None, None, None] for i in range(3))
    ah = diff.alpha_hat.double()[t_d][:, None, None, None]
    f2 = {"eps": torch.ones_like(ah), "v": ah, "x0": ah / (1 - ah)}[diff.prediction]
    d2 = f2 * (p.detach().double() - target.double()) ** 2
    lv = O.logvar64(v.double(), lb, lbt)
    xx = lv - lbt
    l_vlb = (0.5 * ((xx + torch.expm1(-xx)) + kt * d2 * torch.exp(-lv))).mean() / math.log(2.0)
    return l_simple + (scale * l_vlb).float(), l_vlb


@pytest.mark.parametrize("kind,weighting", (("eps", None), ("v", "min_snr")))
def test_train_step_parity_with_the_hybrid_loss_in_torch_ops(A, kind, weighting):
    afdm, dev = A
    images, steps, _ = _batch(dev)
    t, eps = steps[0]
    t = t.clamp_min(2)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, schedule="cosine", prediction=kind, variance="learned")
    step = afdm.TrainStep(_model(afdm, dev), diff, lr=3e-4, loss_weighting=weighting, vlb_lambda=0.002)
    loss = step(images, t=t, eps=eps)
    fp = step.opt.fp
    got_grad = fp.grad[:fp.n_active].clone()
    ref = afdm.TrainStep(_model(afdm, dev), diff, lr=3e-4)
    t_d = t.to(dev)
    x_t, _ = diff.noise_images(images, t_d, eps)
    out = ref.model(x_t, t_d)
    w = torch.ones(T, device=dev) if weighting is None else diff.snr_weights(weighting, 5.0).float().to(dev)
    want_loss, want_vlb = _torch_hybrid(diff, out, images, eps, t_d, w, 0.002 * (T - 1))
    ref.opt.zero_grad()
    with afdm.ops.inplace_param_grads(ref.wgrad_stream, ref.wgrad_batch):
        want_loss.backward()
    torch.cuda.synchronize()
    want_grad = ref.opt.fp.grad[:ref.opt.fp.n_active]
    tag = f"{kind} {weighting}"
    print(f"{tag}: loss {float(loss):.6f} against {float(want_loss):.6f}; L_vlb {float(step.last_vlb):.6f} against {float(want_vlb):.6f}")
    check("TrainStep hybrid loss vs torch ops", loss.cpu().reshape(1), want_loss.detach().cpu().reshape(1), GATE, tag)
    check("TrainStep hybrid L_vlb vs torch ops", step.last_vlb.cpu().reshape(1), want_vlb.detach().cpu().reshape(1), GATE, tag)
    check("TrainStep hybrid flat gradient vs torch ops", got_grad.cpu(), want_grad.cpu(), GATE, tag)


def _make_step(afdm, dev, mode, learned):
    import copy
    model = _model(afdm, dev, num_classes=5, c_out=6 if learned else 3)
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, **(dict(schedule="cosine", prediction="v", variance="learned") if learned else {}))
    kw = dict(loss_weighting="min_snr") if learned else {}
    kw.update(ema=afdm.EMA(0.9), ema_model=copy.deepcopy(model), ema_start=1, max_grad_norm=0.5, conditional=True,
              lr_schedule=afdm.LRSchedule("cosine", warmup=1, total=3, min_ratio=0.1))
    return afdm.TrainStep(model, diff, lr=3e-4, graph=mode, **kw)


def test_hybrid_step_in_every_launch_mode(A):
    afdm, dev = A
    images, steps, y = _batch(dev, labels=True)
    got = {}
    for mode in (False, True, "lanes"):
        step = _make_step(afdm, dev, mode, True)
        out = [(step(images, t=t, eps=e, y=y).clone(), step.last_vlb.clone()) for t, e in steps]
        torch.cuda.synchronize()
        assert all(math.isfinite(float(l)) and math.isfinite(float(v)) for l, v in out)
        got[mode] = [torch.stack([l for l, _ in out]), torch.stack([v for _, v in out]), step.opt.fp.flat.clone(), step.opt.m.clone(),
                     step.opt.v.clone(), step._ema_home.flat.clone()]
    default = _make_step(afdm, dev, "lanes", False)
    default(images, t=steps[0][0], eps=steps[0][1], y=y)
    print("work nodes of the replayed step: hybrid", step.lanes_counts[0], "default", default.lanes_counts[0])
    assert step.lanes_counts[0] == default.lanes_counts[0]                 # no launch more than the default step
    for mode in (True, "lanes"):
        for a, b, tag in zip(got[mode], got[False], ("losses", "vlb", "params", "m", "v", "ema")):
            assert torch.equal(a, b), (mode, tag)


class EpsHalf(torch.nn.Module):
    """A learned-variance model read as a fixed-variance one: its prediction half."""

    def __init__(self, net, C=3):
        super().__init__()
        self.net, self.C = net, C
        self.label_emb = getattr(net, "label_emb", None)

    _t_range = property(lambda self: self.net._t_range, lambda self, v: setattr(self.net, "_t_range", v))      # Diffusion._hint

    def forward(self, x, t, y=None):
        out = self.net(x, t) if y is None else self.net(x, t, y)
        return out[:, :self.C].contiguous()


def test_ddpm_chain_graph_equals_eager_and_uses_the_learned_variance(A):
    afdm, dev = A
    net, cnet = _model(afdm, dev), _model(afdm, dev, seed=43, num_classes=5)
    d4 = afdm.Diffusion(noise_steps=4, img_size=32, device=dev, variance="learned")
    labels = torch.tensor([1, 3])
    runs = {"plain": lambda gr: d4.sample(net, n=2, image_channels=3, noise_source="device", return_float=True, graph=gr)[2],
            "guided": lambda gr: d4.sample(cnet, n=2, image_channels=3, noise_source="device", return_float=True, graph=gr, labels=labels,
                                           cfg_scale=3.0)[2],
            "revert": lambda gr: d4.revert(net, n=1, image_channels=3, noise_source="device", graph=gr)}
    for name, run in runs.items():
        got = {}
        for gr in (False, True):
            afdm.set_seed(9)
            got[gr] = run(gr).clone()
        assert bool(torch.isfinite(got[False].float()).all())
        assert torch.equal(got[True], got[False]), name
    # the chain is the step kernel's: the same seed, by hand
    afdm.set_seed(9)
    x = torch.randn(2, 3, 32, 32, device=dev)
    net.eval()
    with torch.no_grad():
        for i in (3, 2, 1):
            out2 = net(x, torch.full((2,), i, device=dev, dtype=torch.long))
            z = torch.randn_like(x) if i > 1 else None
            x = afdm.ops.denoise_step_lvar(x, out2.contiguous(), z, d4.alpha, d4.alpha_hat, d4.beta, d4._lv(), "eps", i)
    net.train()
    afdm.set_seed(9)
    assert torch.equal(d4.sample(net, n=2, image_channels=3, noise_source="device", return_float=True)[2], x)
    # ... and differs from the fixed-variance chain on the prediction half
    afdm.set_seed(9)
    fixed = afdm.Diffusion(noise_steps=4, img_size=32, device=dev).sample(EpsHalf(net), n=2, image_channels=3, noise_source="device",
                                                                          return_float=True)[2]
    assert not torch.equal(fixed, x)


def test_ddim_and_dpmpp_read_the_prediction_half(A):
    afdm, dev = A
    net = _model(afdm, dev)
    for kind in ("eps", "v"):
        learned = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, prediction=kind, variance="learned")
        fixed = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, prediction=kind)
        for kw in (dict(steps=5, eta=0.0), dict(steps=5, eta=1.0), dict(steps=5, sampler="dpmpp_2m")):
            afdm.set_seed(9)
            got = learned.sample(net, n=2, image_channels=3, noise_source="device", return_float=True, **kw)[2]
            afdm.set_seed(9)
            want = fixed.sample(EpsHalf(net), n=2, image_channels=3, noise_source="device", return_float=True, **kw)[2]
            assert torch.equal(got, want), (kind, kw)


class _Recorder:
    def __init__(self, dev):
        self.chunks, self.dev = [], dev

    def __call__(self, shape):
        z = torch.randn(shape, device=self.dev)
        self.chunks.append(z)
        return z


class _Cheat(torch.nn.Module):
    """Returns the noise of the chunk being scored, and the constant v; `noisy` adds a fixed error to the noise."""

    def __init__(self, rec, v, noisy=0.0, learned=True):
        super().__init__()
        self.rec, self.v, self.noisy, self.learned = rec, v, noisy, learned

    def forward(self, x, t):
        e = self.rec.chunks[-1]
        e = e + self.noisy * torch.sin(37.0 * x) if self.noisy else e
        return torch.cat([e, torch.full_like(e, self.v)], dim=1) if self.learned else e


def test_calc_bpd_learned_at_the_two_ends_of_the_interpolation(A):
    afdm, dev = A
    Tn, n = 21, 3
    learned = afdm.Diffusion(noise_steps=Tn, img_size=32, device=dev, variance="learned")
    fixed = afdm.Diffusion(noise_steps=Tn, img_size=32, device=dev)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8)
    # exact noise and v = -1 (the posterior variance): every KL term is zero, as test_exact_noise_model_has_zero_kl_terms finds
    rec = _Recorder(dev)
    r = learned.calc_bpd(_Cheat(rec, -1.0), x0, sigma="learned", batch=7, noise_fn=rec, return_terms=True)
    assert torch.all(r["terms"][:, 2:] == 0.0) and torch.all(r["vb_bpd"] == 0.0) and torch.all(r["mse"][:, 1:] == 0.0)
    assert torch.allclose(r["bpd"], r["prior_bpd"] + r["decoder_bpd"], rtol=1e-15, atol=0)
    afdm.set_seed(3)
    rec = _Recorder(dev)
    post = fixed.calc_bpd(_Cheat(rec, 0.0, learned=False), x0, sigma="posterior", batch=7, noise_fn=rec)
    afdm.set_seed(3)
    rec = _Recorder(dev)
    r = learned.calc_bpd(_Cheat(rec, -1.0), x0, sigma="learned", batch=7, noise_fn=rec)
    e = float(((r["bpd"] - post["bpd"]).abs() / post["bpd"].abs()).max())
    note("calc_bpd learned, v = -1 vs sigma='posterior' (max rel)", e)
    assert e < 1e-12
    # v = +1 is sigma = "beta", on a model with an error in its noise
    for noisy in (0.0, 0.05):
        res = {}
        for name, d, kw in (("learned", learned, dict(sigma="learned")), ("beta", fixed, dict(sigma="beta")),
                            ("half", learned, dict(sigma="beta"))):
            afdm.set_seed(3)
            rec = _Recorder(dev)
            res[name] = d.calc_bpd(_Cheat(rec, 1.0, noisy, learned=name != "beta"), x0, batch=7, noise_fn=rec, **kw)
        for key in ("bpd", "vb_bpd", "decoder_bpd", "prior_bpd"):
            e = float(((res["learned"][key] - res["beta"][key]).abs() / res["beta"][key].abs()).max())
            note("calc_bpd learned, v = +1 vs sigma='beta' (max rel)", e, (noisy, key))
            assert e < 1e-12, (noisy, key, e)
            assert torch.equal(res["half"][key], res["beta"][key])         # the fixed sigmas score the prediction half
    with pytest.raises(ValueError, match="unknown sigma"):
        fixed.calc_bpd(_Cheat(rec, 1.0, learned=False), x0, sigma="learned")


def test_ddpm_run_with_a_learned_variance(A, tmp_path, monkeypatch):
    afdm, dev = A
    from PIL import Image
    rng = np.random.default_rng(0)
    for c in ("a", "b"):
        os.makedirs(tmp_path / "data" / c)
        for i in range(4):
            Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(tmp_path / "data" / c / f"{i}.png")
    monkeypatch.chdir(tmp_path)
    params = {"unet_v": 3, "dataset": "synthetic", "epochs": 1, "batchsize": 4, "image_size": 32, "image_channels": 3,
              "device": "cuda", "lr": 3e-4, "noise_steps": 12, "image_gen_per_epoch": 2, "dataset_dir": str(tmp_path / "data"),
              "f_kernel": 3, "f_beta": 2, "f_down": math.pi / 2, "f_up": math.pi / 2, "save_trining": False,
              "gen_per_batch": 4, "gen_total": 4, "collage_n_per_image": 4, "collage_n": 4, "seed": 42,
              "noise_schedule": "cosine", "variance": "learned", "vlb_lambda": 0.01, "eval_bpd": 2, "eval_bpd_sigma": "learned"}
    seen = []
    init = afdm.TrainStep.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        seen.append((self.learned, self.vlb_lambda, self.diffusion.schedule, self.model.outc.out_channels))
    monkeypatch.setattr(afdm.TrainStep, "__init__", spy)
    out = afdm.ddpm_run(dict(params))
    assert seen == [(True, 0.01, "cosine", 6)]
    run = "DDPM_Uncondtional_synthetic_3"
    text = (tmp_path / "runs" / run / "settings_synthetic_3.txt").read_text()
    assert text.endswith("\nnoise_schedule: cosine\nvariance: learned\nvlb_lambda: 0.01")
    assert "sigma: learned" in (tmp_path / "runs" / run / "bpd_synthetic_3.txt").read_text()
    ckpt = tmp_path / "models" / run / "ckpt_synthetic_3.pt"
    assert ckpt.exists() and all(math.isfinite(l) for l in out["loss_all"]) and math.isfinite(out["bpd"])
    assert tuple(out["sample"].shape) == (6, 3, 32, 32) and out["sample"].dtype == torch.uint8
    # the evaluators build the model and its Diffusion from the same keys
    args = afdm.argument(image_size=32, image_channels=3, device="cuda", noise_steps=12, noise_schedule="cosine", variance="learned")
    data = {"args": args, "unet_v": 3, "seed": 42, "f_settings": dict(F_SET), "modelpath": str(ckpt)}
    images = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8)
    r = afdm.bpd_results(data, images, sigma="learned")
    assert bool(torch.isfinite(r["bpd"]).all())
    assert not torch.equal(r["bpd"], afdm.bpd_results(data, images, sigma="beta")["bpd"])
