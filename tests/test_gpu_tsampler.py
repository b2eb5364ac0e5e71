"""Loss-aware timestep sampling on the GPU: the per-row loss kernels, the sampler's tick and draw against the fp64 numpy
restatement of tests/test_tsampler_host.py, lvar_loss(vw=), and TrainStep(t_sampler=) in every launch mode."""
import math

import numpy as np
import pytest
import torch

import lvar_oracle as O
from conftest import check, note
from test_tsampler_host import Oracle

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
GATE = 1e-5                  # the project's per-op gate
KINDS = ("eps", "v", "x0")
T, H, B = 12, 3, 8
CHWS = (48, 5)               # the vector path, the scalar path
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _placed(x, dev, shift):
    """x on the device as a contiguous view that starts `shift` floats into its buffer (shift 0: 16-byte aligned)."""
    buf = torch.empty(x.numel() + 4, device=dev, dtype=torch.float32)
    v = buf[shift:shift + x.numel()].view(x.shape)
    v.copy_(x)
    return v


def _tables(diff):
    return diff.beta, diff.alpha, diff.alpha_hat


def _simple_rows64(diff, kind, p, x0, eps, t, w):
    """(1 / chw) w[t_b] sum_i (pred - target)^2 per row, numpy fp64 on the fp32 inputs."""
    ah = diff.alpha_hat.cpu().double().numpy()[t.numpy()][:, None]
    sa, sb = np.sqrt(ah), np.sqrt(1.0 - ah)
    P, X, E = (v.double().numpy() for v in (p, x0, eps))
    target = {"eps": E, "x0": X, "v": sa * E - sb * X}[kind]
    wr = np.ones(len(t)) if w is None else w.double().numpy()[t.numpy()]
    return wr * ((P - target) ** 2).sum(axis=1) / P.shape[1]


def _worst_rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want))))


# ---- row losses ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_row_losses_against_fp64(A, kind, weighted):
    afdm, dev = A
    ops = afdm.ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, prediction=kind, variance="learned")
    w = diff.snr_weights("min_snr", 5.0).float() if weighted else None
    w_d = None if w is None else w.to(dev)
    scale = 0.001 * (T - 1)
    for chw in CHWS:
        out2, x0, eps, t = O.case(B, chw, T, 11 * chw + 1, _tables(diff), kind)
        p = out2[:, :chw].contiguous()
        want_s = _simple_rows64(diff, kind, p, x0, eps, t, w)
        terms = O.hybrid(*_tables(diff), kind, out2, x0, eps, t, w, scale, dev=dev)["term"].numpy()
        want_l = want_s + (scale / (chw * LN2)) * terms
        t_d = t.to(dev)
        got = {}
        for shift in (0, 1):
            p_d, o_d, x_d, e_d = (_placed(v, dev, shift) for v in (p, out2, x0, eps))
            runs = [(ops.loss_rows(p_d, x_d, e_d, t_d, diff.alpha_hat, w_d, kind),
                     ops.lvar_loss_rows(o_d, x_d, e_d, t_d, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), w_d, kind, scale))
                    for _ in range(2)]
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])      # identical bytes run to run
            rs, rl = runs[0]
            assert rs.dtype == torch.float64 and tuple(rs.shape) == (B,) and tuple(rl.shape) == (B,)
            tag = f"{kind} w={weighted} chw={chw} shift={shift}"
            es, el = _worst_rel(rs.cpu().numpy(), want_s), _worst_rel(rl.cpu().numpy(), want_l)
            note("loss_rows vs fp64 (relative, per row)", es, tag)
            note("lvar_loss_rows vs fp64 (relative, per row)", el, tag)
            print(f"row losses vs fp64 {tag}: fixed {es:.2e}, learned {el:.2e}")
            assert es < GATE and el < GATE, (tag, es, el)
            # (1 / B) sum rows is the loss the existing kernels return
            loss = ops.objective_loss(p_d, x_d, e_d, t_d, diff.alpha_hat, w_d, kind)
            lv = ops.lvar_loss(o_d, x_d, e_d, t_d, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), w_d, kind, scale)[0]
            check("mean of loss_rows vs objective_loss", rs.mean().cpu().reshape(1), loss.double().cpu().reshape(1), GATE, tag)
            check("mean of lvar_loss_rows vs lvar_loss", rl.mean().cpu().reshape(1), lv.double().cpu().reshape(1), GATE, tag)
            got[shift] = (rs, rl)
        if chw % 4 == 0:
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])          # vector path == scalar path
    out = torch.zeros(B, device=dev, dtype=torch.float64)
    assert ops.loss_rows(p_d, x_d, e_d, t_d, diff.alpha_hat, w_d, kind, out=out) is out and torch.equal(out, got[1][0])
    with pytest.raises(afdm.AfdError, match="out must be"):
        ops.loss_rows(p_d, x_d, e_d, t_d, diff.alpha_hat, w_d, kind, out=out.float())


# ---- the tick ------------------------------------------------------------------------------------------------------------------------
class _State:
    def __init__(self, dev, T_, H_, lo=1):
        z = lambda *s, dt=torch.float64: torch.zeros(*s, device=dev, dtype=dt)
        self.hist, self.count, self.prob, self.cdf = z(T_, H_), z(T_, dt=torch.int32), z(T_), z(T_ - lo)
        self.wtab, self.vwtab, self.warm = z(T_, dt=torch.float32), z(T_, dt=torch.float32), z(1, dt=torch.int32)
        self.dev, self.lo = dev, lo

    def tick(self, ops, t, rows, up, w_base):
        ops.tsampler_tick(torch.as_tensor(t, dtype=torch.long).to(self.dev), torch.as_tensor(rows, dtype=torch.float64).to(self.dev),
                          self.hist, self.count, self.lo, up, w_base, self.prob, self.cdf, self.wtab, self.vwtab, self.warm)


def _within_one_ulp(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


def _same_as_oracle(st, o, tag):
    assert np.array_equal(st.hist.cpu().numpy(), o.hist), tag                            # exactly
    assert np.array_equal(st.count.cpu().numpy(), o.count), tag
    assert bool(st.warm.item()) == o.warm, tag
    prob, cdf = st.prob.cpu().numpy(), st.cdf.cpu().numpy()
    assert prob[0] == 0.0 and cdf[-1] == 1.0 and np.all(np.diff(cdf) >= 0), tag
    ep, ec = _worst_rel(prob[1:], o.prob[1:]), _worst_rel(cdf, o.cdf)
    note("tsampler tick: prob vs fp64 numpy (relative)", ep, tag)
    note("tsampler tick: cdf vs fp64 numpy (relative)", ec, tag)
    assert ep < 1e-12 and ec < 1e-12, (tag, ep, ec)
    assert _within_one_ulp(st.wtab.cpu().numpy(), o.wtab) and _within_one_ulp(st.vwtab.cpu().numpy(), o.vwtab), tag


@pytest.mark.parametrize("with_base", (False, True))
def test_tick_against_the_oracle(A, with_base):
    afdm, dev = A
    g = np.random.default_rng(3)
    w_base = (g.random(T) * 3 + 0.1).astype(np.float32) if with_base else None
    w_d = None if w_base is None else torch.from_numpy(w_base).to(dev)
    up = 0.05
    st, o = _State(dev, T, H), Oracle(T, H, up, w_base)
    # one t five times (more than H: its history wraps within the batch), a NaN row (t = 7 stays unseen), t = 11 never seen
    t0 = [5, 5, 3, 5, 5, 7, 5, 2]
    r0 = (g.random(B) * 4 + 0.01).tolist()
    r0[5] = float("nan")
    st.tick(afdm.ops, t0, r0, up, w_d)
    o.update(t0, r0)
    assert o.count[5] == H and o.hist[5].tolist() == [r0[3], r0[4], r0[6]] and o.count[7] == 0 and o.count[11] == 0
    _same_as_oracle(st, o, "first batch")
    # before warm-up the tables are the base weights and ones, exactly, and the distribution is uniform
    assert not o.warm
    assert np.array_equal(st.wtab.cpu().numpy(), o.w_base) and np.array_equal(st.vwtab.cpu().numpy(), np.ones(T, dtype=np.float32))
    assert np.array_equal(st.prob.cpu().numpy()[1:], np.full(T - 1, 1.0 / (T - 1)))
    # warm up: every t in [1, T) three times over, in batches of 8, with an inf row on the way
    seq = list(range(1, T)) * H + [5, 5, 5, 5, 5, 1, 1]
    for i in range(0, len(seq), B):
        tb = seq[i:i + B]
        rb = (g.random(len(tb)) * 4 + 0.01).tolist()
        if i == B:
            tb, rb = tb + [4], rb + [float("inf")]
        st.tick(afdm.ops, tb, rb, up, w_d)
        o.update(tb, rb)
        _same_as_oracle(st, o, f"warm-up batch {i // B}")
    assert o.warm and int(st.warm.item()) == 1
    prob = st.prob.cpu().numpy()
    assert abs(prob.sum() - 1.0) < 1e-12 and prob[1:].max() / prob[1:].min() > 1.05      # no longer uniform
    assert not np.array_equal(st.vwtab.cpu().numpy(), np.ones(T, dtype=np.float32))


def test_tick_with_an_all_zero_history_is_uniform(A):
    afdm, dev = A
    w_base = torch.linspace(0.5, 2.0, T, device=dev)
    st = _State(dev, T, H)
    st.count[1:] = H
    st.tick(afdm.ops, [1], [float("nan")], 0.001, w_base)
    assert int(st.warm.item()) == 1 and bool((st.hist == 0).all())
    assert np.array_equal(st.prob.cpu().numpy(), np.array([0.0] + [1.0 / (T - 1)] * (T - 1)))
    assert torch.equal(st.wtab, w_base) and bool((st.vwtab == 1).all())
    assert float(st.cdf[-1]) == 1.0


def test_tick_with_more_timesteps_and_rows_than_threads(A):
    """T = 600 and B = 300: every thread owns several timesteps, the batch passes through LDS in two pieces, and the prefix sum
    runs over chunks of three."""
    afdm, dev = A
    T2, H2, B2, up = 600, 2, 300, 0.001
    g = np.random.default_rng(5)
    o = Oracle(T2, H2, up)
    o.hist[1:] = g.random((T2 - 1, H2)) * 2 + 0.01
    o.count[1:] = H2
    o.count[17] = 1                                       # not warm at first
    o.refresh()
    st = _State(dev, T2, H2)
    st.hist.copy_(torch.from_numpy(o.hist))
    st.count.copy_(torch.from_numpy(o.count))
    t = np.concatenate([g.integers(1, 40, B2 // 2), g.integers(1, T2, B2 - B2 // 2)])
    rows = g.random(B2) * 3 + 0.01
    rows[7], rows[290] = float("nan"), float("-inf")
    t[299] = 17                                           # the last row fills the one short history: warm after this batch
    for rnd in range(2):
        st.tick(afdm.ops, t, rows, up, None)
        o.update(t, rows)
        _same_as_oracle(st, o, f"T=600 round {rnd}")
    assert o.warm and abs(float(st.prob.sum()) - 1.0) < 1e-12


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def _draw_inputs(cdf):
    """u with every value at least 1e-9 from an edge of cdf: just inside both ends and the middle of every bin, 0 and 1 - 2^-53."""
    edges = np.concatenate([[0.0], cdf])
    u = [0.0, 1.0 - 2.0 ** -53]
    for a, b in zip(edges[:-1], edges[1:]):
        assert b - a > 4e-9
        u += [a + 1e-9, (a + b) / 2.0, b - 1e-9]
    u = np.array(u)
    d = np.abs(u[:, None] - cdf[None, :-1])               # (the last edge is 1: u < 1 always)
    assert d.min() >= 1e-9 * (1 - 1e-6)
    return u


@pytest.mark.parametrize("warm", (False, True))
def test_draw_against_searchsorted(A, warm):
    afdm, dev = A
    g = np.random.default_rng(9)
    o = Oracle(T, H, 0.01)
    if warm:
        o.hist[1:] = g.random((T - 1, H)) * 5 + 0.01
        o.count[1:] = H
        o.refresh()
    assert o.warm == warm
    u = _draw_inputs(o.cdf)
    got = afdm.ops.tsampler_draw(torch.from_numpy(o.cdf).to(dev), torch.from_numpy(u).to(dev), 1)
    assert got.dtype == torch.long and np.array_equal(got.cpu().numpy(), o.draw(u))
    assert set(got.tolist()) == set(range(1, T))                                       # every timestep is reached, 0 never
    assert got[0].item() == 1 and got[1].item() == T - 1
    # a long table and more rows than one workgroup
    o2 = Oracle(600, 2, 0.001)
    o2.hist[1:] = g.random((599, 2)) + 0.01
    o2.count[1:] = 2
    o2.refresh()
    u2 = g.random(1000)
    u2 = u2[np.abs(u2[:, None] - o2.cdf[None, :]).min(axis=1) >= 1e-9]
    got2 = afdm.ops.tsampler_draw(torch.from_numpy(o2.cdf).to(dev), torch.from_numpy(u2).to(dev), 1)
    assert np.array_equal(got2.cpu().numpy(), o2.draw(u2)) and int(got2.min()) >= 1 and int(got2.max()) <= 599


# ---- lvar_loss(vw=) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lvar_loss_with_the_second_table(A, kind):
    afdm, dev = A
    ops = afdm.ops
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev, prediction=kind, variance="learned")
    w = diff.snr_weights("min_snr", 5.0).float()
    w_d = w.to(dev)
    scale = 0.001 * (T - 1)
    g = torch.Generator().manual_seed(4)
    vw = torch.rand(T, generator=g) * 1.5 + 0.5
    for chw in CHWS:
        out2, x0, eps, t = O.case(B, chw, T, 5 * chw + 2, _tables(diff), kind)
        x_d, e_d, t_d = x0.to(dev), eps.to(dev), t.to(dev)

        def run(vw_d):
            o_d = out2.to(dev).requires_grad_(True)
            loss, vlb, sums = ops.lvar_loss(o_d, x_d, e_d, t_d, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), w_d, kind, scale,
                                            return_sums=True, vw=vw_d)
            loss.backward()
            return loss.detach(), vlb, sums, o_d.grad

        plain, ones = run(None), run(torch.ones(T, device=dev))
        assert all(torch.equal(a, b) for a, b in zip(plain, ones)), (kind, chw)            # vw == 1: the bits of vw=None
        loss, vlb, sums, grad = (v.cpu() for v in run(vw.to(dev)))
        want = O.hybrid(*_tables(diff), kind, out2, x0, eps, t, w, scale, dev=dev)
        r = vw.double()[t]
        want_vlb = (r * want["term"]).sum() / (B * chw * LN2)
        want_L = want["L_simple"] + scale * want_vlb
        tag = f"{kind} chw={chw}"
        check("lvar loss (vw): L vs fp64", loss.reshape(1), want_L.reshape(1), GATE, tag)
        check("lvar loss (vw): L_vlb vs fp64", vlb.reshape(1), want_vlb.reshape(1), GATE, tag)
        check("lvar loss (vw): L_vlb (fp64 output) vs fp64", sums[1:], want_vlb.reshape(1), 1e-9, tag)
        check("lvar loss (vw): dp vs fp64", grad[:, :chw], want["dp"], GATE, tag)
        check("lvar loss (vw): dv vs fp64", grad[:, chw:], r[:, None] * want["dv"], GATE, tag)
    with pytest.raises(afdm.AfdError, match="vw must be"):
        ops.lvar_loss(out2.to(dev), x_d, e_d, t_d, diff.alpha, diff.alpha_hat, diff.beta, diff._lv(), w_d, kind, scale,
                      vw=torch.ones(T + 1, device=dev))


# ---- the step ------------------------------------------------------------------------------------------------------------------------
TS, HS = 6, 2                # noise steps and history of the step tests: warm after two steps of the batches below
STEP_T = ([1, 2, 3, 4, 5, 1, 2, 3], [4, 5, 4, 5, 1, 2, 3, 3], [5, 1, 1, 2, 4, 3, 5, 5], [2, 2, 3, 4, 1, 5, 4, 1], [3, 5, 2, 1, 4, 4, 2, 5])


def _model(afdm, dev, c_out=3, seed=42):
    afdm.set_seed(seed)
    return afdm.UNet(c_in=3, c_out=c_out, image_size=32, f_settings=dict(F_SET), device=dev, variant=3).to(dev)


def _batches(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    return images, [(torch.tensor(t), torch.randn(B, 3, 32, 32, generator=g).to(dev)) for t in STEP_T]


def _make_step(afdm, dev, mode, learned, sampler=True):
    """learned: variance="learned" (eps-prediction); else v-prediction with loss_weighting="min_snr"."""
    diff = afdm.Diffusion(noise_steps=TS, img_size=32, device=dev, **(dict(variance="learned") if learned else dict(prediction="v")))
    kw = dict(vlb_lambda=0.01) if learned else dict(loss_weighting="min_snr")
    if sampler:
        kw["t_sampler"] = afdm.LossSecondMomentSampler(diff, history_per_term=HS, uniform_prob=0.01)
    return afdm.TrainStep(_model(afdm, dev, 6 if learned else 3), diff, lr=3e-4, graph=mode, **kw)


@pytest.mark.parametrize("learned", (False, True))
def test_step_loss_is_the_importance_weighted_mean_of_the_row_losses(A, learned):
    afdm, dev = A
    ops = afdm.ops
    images, steps = _batches(dev)
    step = _make_step(afdm, dev, False, learned)
    ts, d = step.t_sampler, step.diffusion
    o = Oracle(TS, HS, 0.01, None if step.loss_weights is None else step.loss_weights.cpu().numpy())
    uniform = np.array([0.0] + [1.0 / (TS - 1)] * (TS - 1))
    for i, (t, eps) in enumerate(steps):
        t_d = t.to(dev)
        # both factors of the estimate, before the step: the weights, and the row losses of the model as it stands
        iw = ts.weights().double()[t_d]
        x_t, _ = d.noise_images(images, t_d, eps)
        pred = step.model(x_t, t_d).detach()
        if learned:
            rows = ops.lvar_loss_rows(pred, images, eps, t_d, d.alpha, d.alpha_hat, d.beta, d._lv(), step.loss_weights, "eps",
                                      0.01 * (TS - 1))
        else:
            rows = ops.loss_rows(pred, images, eps, t_d, d.alpha_hat, step.loss_weights, "v")
        assert np.array_equal(ts.probabilities().cpu().numpy(), uniform) == (i < 2)      # warm after two steps
        assert ts.warmed_up == (i >= 2)
        loss = step(images, t=t, eps=eps)
        want = (iw * rows).mean()
        print(f"step {i} learned={learned}: loss {float(loss):.6f} against (1/B) sum iw l = {float(want):.6f}")
        check("TrainStep(t_sampler): loss vs (1/B) sum iw[t] l", loss.cpu().reshape(1), want.cpu().reshape(1), GATE, (learned, i))
        # the tick saw the step's own rows; the sampler's state is the oracle's
        mine = ts.rows_buffer(B).clone()
        check("TrainStep(t_sampler): the step's rows vs ops.*_loss_rows", mine.cpu(), rows.cpu(), GATE, (learned, i))
        o.update(t.numpy(), mine.cpu().numpy())
        assert np.array_equal(ts.hist.cpu().numpy(), o.hist) and np.array_equal(ts.count.cpu().numpy(), o.count)
        prob = ts.probabilities().cpu().numpy()
        assert _worst_rel(prob[1:], o.prob[1:]) < 1e-12 and abs(prob.sum() - 1.0) < 1e-12
        assert _within_one_ulp(ts.wtab.cpu().numpy(), o.wtab) and _within_one_ulp(ts.weights().cpu().numpy(), o.vwtab)
    assert not np.array_equal(prob, uniform)                                             # the distribution moved after warm-up
    mean, count = ts.loss_by_timestep()
    assert count.tolist() == [0] + [HS] * (TS - 1) and math.isnan(float(mean[0]))
    assert np.allclose(mean[1:].cpu().numpy(), o.hist[1:].mean(axis=1), rtol=1e-14, atol=0)
    if learned:
        assert math.isfinite(float(step.last_vlb))


@pytest.mark.parametrize("learned", (False, True))
def test_sampler_step_is_bit_identical_in_every_launch_mode(A, learned):
    afdm, dev = A
    images, steps = _batches(dev)
    got = {}
    for mode in (False, True, "lanes"):
        step = _make_step(afdm, dev, mode, learned)
        losses = [step(images, t=t, eps=e).clone() for t, e in steps]
        torch.cuda.synchronize()
        ts = step.t_sampler
        assert ts.warmed_up and all(math.isfinite(float(l)) for l in losses)
        got[mode] = [torch.stack(losses), step.opt.fp.flat.clone(), ts.hist.clone(), ts.count.clone(), ts.prob.clone(), ts.wtab.clone()]
    default = _make_step(afdm, dev, "lanes", learned, sampler=False)
    default(images, t=steps[0][0], eps=steps[0][1])
    print(f"work nodes of the replayed step (learned={learned}): sampler", step.lanes_counts[0], "default", default.lanes_counts[0])
    assert step.lanes_counts[0] <= default.lanes_counts[0] + 2                            # the row losses and the tick
    for mode in (True, "lanes"):
        for a, b, tag in zip(got[mode], got[False], ("losses", "params", "hist", "count", "prob", "wtab")):
            assert torch.equal(a, b), (mode, tag)


@pytest.mark.parametrize("mode", (False, "lanes"))
def test_drawn_timesteps_stay_in_range_and_leave_the_cpu_generator_alone(A, mode):
    afdm, dev = A
    images, steps = _batches(dev)
    step = _make_step(afdm, dev, mode, False)
    ts = step.t_sampler
    seen = []
    draw = ts.draw
    ts.draw = lambda n, u=None, out=None: seen.append(draw(n, u, out)) or seen[-1]
    state = torch.get_rng_state()
    for _, eps in steps:
        assert math.isfinite(float(step(images, eps=eps)))
        seen[-1] = seen[-1].clone()
    assert torch.equal(torch.get_rng_state(), state)                                     # torch's CPU generator did not advance
    assert len(seen) == len(steps)
    t = torch.stack(seen).cpu()
    assert t.dtype == torch.long and tuple(t.shape) == (len(steps), B) and int(t.min()) >= 1 and int(t.max()) <= TS - 1
    assert int(ts.count[0]) == 0
    hist_t = torch.bincount(t.flatten(), minlength=TS).clamp(max=HS)
    assert torch.equal(ts.count.cpu().long(), hist_t)                                    # the tick saw exactly the drawn timesteps
    if mode:
        assert torch.equal(step._static["t"].cpu(), t[-1])                                # drawn straight into the static buffer


def test_sampler_state_dict_round_trip_continues_bit_identically(A):
    afdm, dev = A
    images, steps = _batches(dev)
    step = _make_step(afdm, dev, False, False)
    for t, e in steps[:3]:
        step(images, t=t, eps=e)
    a = step.t_sampler
    state = a.state_dict()
    assert all(not v.is_cuda for v in (state["hist"], state["count"])) and state["history_per_term"] == HS
    b = afdm.LossSecondMomentSampler(step.diffusion, history_per_term=HS, uniform_prob=0.5)
    b.set_base_weights(step.loss_weights)
    b.load_state_dict(state)
    assert b.uniform_prob == a.uniform_prob and b.warmed_up
    g = torch.Generator().manual_seed(1)
    for _ in range(2):
        for x, y in zip(a.buffers(), b.buffers()):
            assert torch.equal(x, y)
        u = torch.rand(64, generator=g, dtype=torch.float64).to(dev)
        assert torch.equal(a.draw(64, u), b.draw(64, u))
        t = torch.randint(1, TS, (B,), generator=g).to(dev)
        rows = torch.rand(B, generator=g, dtype=torch.float64).to(dev)
        a.update(t, rows)
        b.update(t, rows)
    with pytest.raises(ValueError, match="another"):
        afdm.LossSecondMomentSampler(step.diffusion, history_per_term=HS + 1).load_state_dict(state)


def test_step_without_a_sampler_is_unchanged(A):
    """t_sampler=None against a step built without the keyword: bit-identical training, the same replay list, and the timesteps
    still come from torch's CPU generator."""
    afdm, dev = A
    images, steps = _batches(dev)
    got = []
    for kw in (dict(), dict(t_sampler=None)):
        diff = afdm.Diffusion(noise_steps=TS, img_size=32, device=dev, prediction="v")
        step = afdm.TrainStep(_model(afdm, dev), diff, lr=3e-4, graph="lanes", loss_weighting="min_snr", **kw)
        assert step.t_sampler is None
        losses = [step(images, t=t, eps=e).clone() for t, e in steps[:3]]
        torch.manual_seed(123)
        state = torch.get_rng_state()
        losses.append(step(images, eps=steps[3][1]).clone())
        assert not torch.equal(torch.get_rng_state(), state)                             # Diffusion.sample_timesteps drew
        torch.cuda.synchronize()
        got.append((torch.stack(losses), step.opt.fp.flat.clone(), step.lanes_counts))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and got[0][2] == got[1][2]


def test_train_saves_the_sampler_state_beside_the_checkpoint(A, tmp_path, monkeypatch):
    afdm, dev = A
    monkeypatch.chdir(tmp_path)
    images, _ = _batches(dev)
    diff = afdm.Diffusion(noise_steps=TS, img_size=32, device=dev)
    args = afdm.argument(run_name="ts", epochs=1, batch_size=B, image_size=32, image_channels=3, device=dev, lr=3e-4, noise_steps=TS,
                         image_gen_n=1, t_sampler="loss_second_moment", t_sampler_history=HS, t_sampler_uniform_prob=0.02)
    ckpt = tmp_path / "ckpt.pt"
    losses = afdm.train(args, model_path=str(ckpt), dataloader=[(images.cpu(), None)] * 3, model=_model(afdm, dev), diffusion=diff)
    assert len(losses) == 1 and math.isfinite(losses[0]) and ckpt.exists()
    state = torch.load(afdm.training.t_sampler_path(str(ckpt)), weights_only=True)
    assert state["history_per_term"] == HS and state["uniform_prob"] == 0.02
    assert tuple(state["hist"].shape) == (TS, HS) and int(state["count"][0]) == 0 and 1 <= int(state["count"].sum()) <= 3 * B
