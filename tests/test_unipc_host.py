"""CPU-side tests of UniPC sampling (orders 1-3): the folded coefficient table against a restatement of the rho / D_i definition,
the identities that tie it to DDIM and DPM-Solver++(2M), `unipc_reference` on a data set whose probability-flow ODE is solved in
closed form, the sampler's argument checks, and the C ABI of the two entry points with their argument checks (which return
before any device is touched)."""
import ctypes
import math

import numpy as np
import pytest
import torch

F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_float
CHAINS = [5, 12, 16, 20, [999, 700, 640, 300, 120, 40, 3]]


def _diff(T=1000):
    import afdm
    return afdm.Diffusion(noise_steps=T, img_size=32, device="cpu")


def _levels(d, pairs):
    ah = d.alpha_hat.tolist()
    lev = [t for t, _ in pairs] + [0]
    alpha = [math.sqrt(ah[t]) for t in lev]
    sigma = [math.sqrt(1.0 - ah[t]) for t in lev]
    lam = [math.log(a) - math.log(s) for a, s in zip(alpha, sigma)]
    return lev, alpha, sigma, lam


def _order(k, S, P_):
    p = min(P_, k + 1)
    return min(p, S - k) if S < 15 else p


def _rho(rs, h, corrector):
    """The issue's definition: R[j][i] = r_i^j, b_j = g_{j+1} (j+1)! / B, hh = -h."""
    p = len(rs) + 1
    hh = -h
    B = math.expm1(hh)
    g = math.expm1(hh) / hh - 1.0
    b = []
    for j in range(p):
        b.append(g * math.factorial(j + 1) / B)
        g = g / hh - 1.0 / math.factorial(j + 2)
    if corrector:
        if p == 1:
            return [0.5]
        r = rs + [1.0]
        return list(np.linalg.solve(np.array([[v ** j for v in r] for j in range(p)]), np.array(b)))
    if p == 1:
        return []
    if p == 2:
        return [0.5]
    return list(np.linalg.solve(np.array([[v ** j for v in rs] for j in range(p - 1)]), np.array(b[:p - 1])))


def _apply_move(alpha, sigma, lam, s, u, x, base, earlier, m_new=None):
    """One move in the rho / D_i form on numbers or tensors; earlier: [(position, m)], latest first."""
    h = lam[u] - lam[s]
    B = math.expm1(-h)
    rs = [(lam[q] - lam[s]) / h for q, _ in earlier]
    rho = _rho(rs, h, m_new is not None)
    res = 0.0
    for (q, m), r, w in zip(earlier, rs, rho):
        res = res + w * ((m - base) / r)
    if m_new is not None:
        res = res + rho[-1] * (m_new - base)
    return sigma[u] / sigma[s] * x - alpha[u] * B * base - alpha[u] * B * res


def _table_restated(d, pairs, P_):
    """Each folded weight is the move's response to a unit input: the definition applied to basis vectors."""
    _, alpha, sigma, lam = _levels(d, pairs)
    S = len(pairs)
    rows = []
    for k in range(S):
        c = [1.0, 0.0, 0.0, 0.0, 0.0]
        if k >= 1:
            p = _order(k - 1, S, P_)
            # inputs: x_{k-1}, m_k, m_{k-1}, m_{k-2}, m_{k-3}
            c = []
            for unit in range(5):
                v = [1.0 if j == unit else 0.0 for j in range(5)]
                earlier = [(k - 1 - i, v[2 + i]) for i in range(1, p)]
                c.append(_apply_move(alpha, sigma, lam, k - 1, k, v[0], v[2], earlier, m_new=v[1]))
        p = _order(k, S, P_)
        q = []
        for unit in range(4):                                   # inputs: x_k, m_k, m_{k-1}, m_{k-2}
            v = [1.0 if j == unit else 0.0 for j in range(4)]
            earlier = [(k - i, v[1 + i]) for i in range(1, p)]
            q.append(_apply_move(alpha, sigma, lam, k, k + 1, v[0], v[1], earlier))
        rows.append([alpha[k], sigma[k]] + c + q + [float(k % 3)])
    return np.array(rows, dtype=np.float64)


@pytest.mark.parametrize("steps", CHAINS, ids=str)
@pytest.mark.parametrize("order", [1, 2, 3])
def test_folded_table_matches_the_rho_definition(steps, order):
    d = _diff()
    pairs = d.dpmpp_pairs(steps)
    S = len(pairs)
    t64 = d.unipc_coefficients(pairs, order, dtype=torch.float64)
    t32 = d.unipc_coefficients(pairs, order)
    assert t64.dtype == torch.float64 and t32.dtype == torch.float32 and tuple(t64.shape) == tuple(t32.shape) == (S, 12)
    want = _table_restated(d, pairs, order)
    got = t64.numpy()
    for k in range(S):
        assert np.all(np.abs(got[k] - want[k]) <= 1e-10 * np.max(np.abs(want[k]))), (k, got[k], want[k])
    assert torch.equal(t32.view(torch.int32), torch.tensor(got.astype(np.float32)).view(torch.int32))
    # row 0 has no corrector; the slot is k mod 3, exact; weights beyond the step's order are exactly 0
    assert got[0, 2:7].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert t32[:, 11].tolist() == [float(k % 3) for k in range(S)]
    for k in range(S):
        p = d.unipc_order(k, S, order)
        assert [got[k, 9 + j] != 0.0 for j in range(2)] == [j < p - 1 for j in range(2)]
        if k >= 1:
            pc = d.unipc_order(k - 1, S, order)
            assert got[k, 3] != 0.0 and [got[k, 5 + j] != 0.0 for j in range(2)] == [j < pc - 1 for j in range(2)]


@pytest.mark.parametrize("S", [1, 2, 5, 14, 15, 20])
def test_unipc_order_follows_its_definition(S):
    d = _diff()
    for P_ in (1, 2, 3):
        got = [d.unipc_order(k, S, P_) for k in range(S)]
        assert got == [min(P_, k + 1, S - k) if S < 15 else min(P_, k + 1) for k in range(S)]
    assert [d.unipc_order(k, S, 2) for k in range(S)] == [d.dpmpp_order(k, S) for k in range(S)]
    if S == 14:
        assert [d.unipc_order(k, S, 3) for k in (0, 1, 2, 11, 12, 13)] == [1, 2, 3, 3, 2, 1]
    if S == 15:
        assert [d.unipc_order(k, S, 3) for k in (0, 1, 2, 12, 13, 14)] == [1, 2, 3, 3, 3, 3]


@pytest.mark.parametrize("steps", CHAINS, ids=str)
def test_table_identities(steps):
    d = _diff()
    pairs = d.dpmpp_pairs(steps)
    S = len(pairs)
    _, alpha, sigma, lam = _levels(d, pairs)
    rel = lambda a, b: abs(a - b) <= 1e-12 * abs(b)
    # order 1: the predictor is DDIM's eta = 0 step, x' = sqrt(a_p) x0 + sqrt(1 - a_p) e with e = (x - alpha x0) / sigma
    t1 = d.unipc_coefficients(pairs, 1, dtype=torch.float64).numpy()
    for k in range(S):
        assert rel(t1[k, 7], sigma[k + 1] / sigma[k]) and rel(t1[k, 8], alpha[k + 1] - sigma[k + 1] * alpha[k] / sigma[k])
        assert t1[k, 9] == 0.0 and t1[k, 10] == 0.0
    # order 2: the predictor is DPM-Solver++(2M) wherever both are second order (and the first-order rows agree too)
    t2 = d.unipc_coefficients(pairs, 2, dtype=torch.float64).numpy()
    hs = [lam[k + 1] - lam[k] for k in range(S)]
    seconds = 0
    for k in range(S):
        B = -alpha[k + 1] * math.expm1(-hs[k])
        if d.dpmpp_order(k, S) == 2:
            assert d.unipc_order(k, S, 2) == 2
            r = hs[k - 1] / hs[k]
            want = (sigma[k + 1] / sigma[k], B * (1 + 1 / (2 * r)), -B / (2 * r))
            seconds += 1
        else:
            want = (sigma[k + 1] / sigma[k], B, 0.0)
        assert all(rel(t2[k, 7 + j], want[j]) if want[j] else t2[k, 7 + j] == 0.0 for j in range(3)), (k, t2[k, 7:10], want)
    assert seconds == (S - 2 if S < 15 else S - 1)
    # against the project's own table, fp32: equal up to the rounding of two fp64 values that agree to 1e-12
    dp = d.dpmpp_coefficients(pairs).double().numpy()
    u2 = d.unipc_coefficients(pairs, 2).double().numpy()
    assert np.all(np.abs(u2[:, 7:10] - dp[:, 2:5]) <= 2.0 ** -23 * np.abs(dp[:, 2:5]))
    # every order: a constant m is integrated exactly by both moves
    for order in (1, 2, 3):
        t = d.unipc_coefficients(pairs, order, dtype=torch.float64).numpy()
        for k in range(S):
            pw = -alpha[k + 1] * math.expm1(-hs[k])
            assert abs(t[k, 8:11].sum() - pw) <= 1e-12 * np.abs(t[k, 8:11]).max(), (order, k)
            if k >= 1:
                cw = -alpha[k] * math.expm1(-hs[k - 1])
                assert abs(t[k, 3:7].sum() - cw) <= 1e-12 * np.abs(t[k, 3:7]).max(), (order, k)
            else:
                assert t[0, 2:7].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    with pytest.raises(ValueError, match="order"):
        d.unipc_coefficients(pairs, 4)


# ---- the reference loop on Gaussian data, whose probability-flow ODE has a closed-form solution ------------------------------
@pytest.fixture(scope="module")
def gauss():
    """x0 ~ N(mu, 0.5^2 I) on one 4 x 32 x 32 image: the exact eps (fp64, rounded to fp32), x_T, and the ODE's endpoint."""
    d = _diff()
    ah = d.alpha_hat.double()
    g = torch.Generator().manual_seed(0)
    mu = torch.rand(1, 4, 32, 32, generator=g, dtype=torch.float64) * 1.6 - 0.8

    def model(x, t):
        a = ah[t].view(-1, 1, 1, 1)
        return ((1 - a).sqrt() * (x.double() - a.sqrt() * mu) / (0.25 * a + 1 - a)).float()

    x_T = torch.randn((1, 4, 32, 32), generator=g, dtype=torch.float64)
    a0, aT = float(ah[0]), float(ah[999])
    exact = math.sqrt(a0) * mu + math.sqrt(0.25 * a0 + 1 - a0) * (x_T - math.sqrt(aT) * mu) / math.sqrt(0.25 * aT + 1 - aT)
    return d, model, x_T, exact


def _ddim_restated(d, model, x, pairs):
    ah = d.alpha_hat.tolist()
    x = x.clone()
    for t, tp in pairs:
        e = model(x, torch.full((x.shape[0],), t, dtype=torch.long)).double()
        x0 = (x - math.sqrt(1 - ah[t]) * e) / math.sqrt(ah[t])
        x = math.sqrt(ah[tp]) * x0 + math.sqrt(1 - ah[tp]) * e
    return x


def _dpmpp_restated(d, model, x, pairs):
    _, alpha, sigma, lam = _levels(d, pairs)
    S = len(pairs)
    x = x.clone()
    x0_prev = h_prev = None
    for k, (t, tp) in enumerate(pairs):
        e = model(x, torch.full((x.shape[0],), t, dtype=torch.long)).double()
        x0 = (x - sigma[k] * e) / alpha[k]
        h = lam[k + 1] - lam[k]
        B = -alpha[k + 1] * math.expm1(-h)
        x = sigma[k + 1] / sigma[k] * x
        if k == 0 or (k == S - 1 and S < 15):
            x = x + B * x0
        else:
            r = h_prev / h
            x = x + B * (1 + 1 / (2 * r)) * x0 - B / (2 * r) * x0_prev
        x0_prev, h_prev = x0, h
    return x


def _err(a, b):
    return float((a - b).norm() / b.norm())


def test_reference_beats_2m_on_the_exact_ode(gauss):
    import afdm
    d, model, x_T, exact = gauss
    e2m = {S: _err(_dpmpp_restated(d, model, x_T, d.dpmpp_pairs(S)), exact) for S in (20, 40)}
    u2 = {S: _err(afdm.unipc_reference(model, x_T, d.dpmpp_pairs(S), 2, d), exact) for S in (20, 40)}
    u3 = {S: _err(afdm.unipc_reference(model, x_T, d.dpmpp_pairs(S), 3, d), exact) for S in (16, 20, 40)}
    print(f"exact ODE: 2M {e2m}, UniPC-2 {u2}, UniPC-3 {u3}")
    assert e2m[20] / u3[20] >= 10
    assert e2m[40] / u3[40] >= 10
    assert e2m[20] / u2[20] >= 1.3
    assert e2m[40] / u2[40] >= 2
    assert u3[16] <= e2m[40]


@pytest.mark.parametrize("steps", [12, 20, [999, 640, 120, 40, 3]], ids=str)
def test_bare_predictors_are_ddim_and_2m(gauss, steps):
    import afdm
    d, model, x_T, _ = gauss
    pairs = d.dpmpp_pairs(steps)
    want = {1: _ddim_restated(d, model, x_T, pairs), 2: _dpmpp_restated(d, model, x_T, pairs)}
    for order in (1, 2):
        assert _err(afdm.unipc_reference(model, x_T, pairs, order, d, corrector=False), want[order]) <= 1e-12
        # the folded table with its corrector columns set aside: the corrected state is the predicted one
        tab = d.unipc_coefficients(pairs, order, dtype=torch.float64).tolist()
        x, h1 = x_T.clone(), torch.zeros_like(x_T)
        for k, (t, _) in enumerate(pairs):
            r = tab[k]
            m = (x - r[1] * model(x, torch.full((1,), t, dtype=torch.long)).double()) / r[0]
            x, h1 = r[7] * x + r[8] * m + r[9] * h1, m
            assert r[10] == 0.0
        assert _err(x, want[order]) <= 1e-12
        # with the corrector, the same chain moves away from the bare predictor (the corrector is not a no-op)
        assert _err(afdm.unipc_reference(model, x_T, pairs, order, d), want[order]) > 1e-6


def test_reference_follows_the_folded_table(gauss):
    """The oracle and the table are two codes of one method: the table, applied as the kernel applies it (ring included)."""
    import afdm
    d, model, x_T, _ = gauss
    for steps, order in ((12, 3), (16, 3), (16, 2), (5, 1)):
        pairs = d.dpmpp_pairs(steps)
        tab = d.unipc_coefficients(pairs, order, dtype=torch.float64).tolist()
        xs, xc, hist = x_T.clone(), x_T.clone(), [torch.zeros_like(x_T) for _ in range(3)]
        for k, (t, _) in enumerate(pairs):
            r = tab[k]
            slot = int(r[11])
            h1, h2, h3 = (hist[(slot - j) % 3] for j in (1, 2, 3))
            m = (xs - r[1] * model(xs, torch.full((1,), t, dtype=torch.long)).double()) / r[0]
            xc = r[2] * xc + r[3] * m + r[4] * h1 + r[5] * h2 + r[6] * h3
            xs = r[7] * xc + r[8] * m + r[9] * h1 + r[10] * h2
            hist[slot] = m
        assert _err(xs, afdm.unipc_reference(model, x_T, pairs, order, d)) <= 1e-12, (steps, order)


def test_reference_guidance_and_argument_errors(gauss):
    import afdm
    d, model, x_T, _ = gauss
    pairs = d.dpmpp_pairs(6)
    seen = []

    def labelled(x, t, y):
        seen.append((x.shape[0], y.tolist()))
        return model(x, t).double() * (1.0 + 0.1 * (y != afdm.NULL_LABEL).double().view(-1, 1, 1, 1))

    def lerped(x, t):
        return model(x, t).double() * (1.0 + 0.1 * 3.0)                 # e_u + s (e_c - e_u) with e_c = 1.1 e_u

    got = afdm.unipc_reference(labelled, x_T, pairs, 3, d, labels=[4], cfg_scale=3.0)
    assert seen == [(2, [4, afdm.NULL_LABEL])] * 6
    assert _err(got, afdm.unipc_reference(lerped, x_T, pairs, 3, d)) <= 1e-12
    for bad in (0, 4):
        with pytest.raises(ValueError, match="order"):
            afdm.unipc_reference(model, x_T, pairs, bad, d)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_header_declares_and_types_the_unipc_entry_points():
    from afdm._lib import parse_header
    sigs = parse_header()
    assert sigs["afd_unipc_step"] == (I, [P, P, P, P, P, P, L, P])
    assert sigs["afd_unipc_step_cfg"] == (I, [P, P, P, P, P, F, P, P, L, P])


def test_unipc_entry_points_reject_bad_arguments_without_a_gpu():
    import afdm
    lib = afdm.lib()
    with pytest.raises(afdm.AfdError, match="afd_unipc_step: .*NULL"):
        lib.afd_unipc_step(None, None, None, None, None, None, 8, None)
    with pytest.raises(afdm.AfdError, match="afd_unipc_step_cfg: .*NULL"):
        lib.afd_unipc_step_cfg(None, None, None, None, None, 3.0, None, None, 8, None)
    # non-NULL but never dereferenced: each check returns before a launch
    buf = (ctypes.c_float * 256)()
    base = ctypes.addressof(buf)
    at = lambda i: base + 4 * i                               # element i of the buffer
    n = 8
    x, e, c, o, o2, xc, hist = at(0), at(16), at(48), at(64), at(80), at(96), at(112)      # e: 2n values, hist: 3n
    good = [x, e, xc, hist, c, o]
    for j in range(6):                                        # each required pointer in turn
        args = list(good)
        args[j] = None
        with pytest.raises(afdm.AfdError, match="afd_unipc_step: .*NULL"):
            lib.afd_unipc_step(*args, n, None)
        args.insert(5, 3.0)
        with pytest.raises(afdm.AfdError, match="afd_unipc_step_cfg: .*NULL"):
            lib.afd_unipc_step_cfg(*args, o2, n, None)
    for bad_n in (0, -4):
        with pytest.raises(afdm.AfdError, match="afd_unipc_step: n must be positive"):
            lib.afd_unipc_step(x, e, xc, hist, c, o, bad_n, None)
        with pytest.raises(afdm.AfdError, match="afd_unipc_step_cfg: n must be positive"):
            lib.afd_unipc_step_cfg(x, e, xc, hist, c, 3.0, o, o2, bad_n, None)
    # xc overlapping x, eps, x_out or hist
    for bad in (x, at(4), e, at(20), o, at(60), hist, at(108), at(112 + 3 * n - 1)):
        with pytest.raises(afdm.AfdError, match="afd_unipc_step: xc and hist must not overlap"):
            lib.afd_unipc_step(x, e, bad, hist, c, o, n, None)
    # hist (3n values) overlapping x, eps, x_out or xc: a start 3n - 1 values before a buffer still reaches its first value
    for bad in (x, e, at(64 - 3 * n + 1), o, at(96 - 3 * n + 1), at(100)):
        with pytest.raises(afdm.AfdError, match="afd_unipc_step: xc and hist must not overlap"):
            lib.afd_unipc_step(x, e, xc, bad, c, o, n, None)
    # eps2 of the guided form holds 2n values: xc inside its second half overlaps it; x_out2 too
    for bad in (at(16 + n + 2), o2, at(84)):
        with pytest.raises(afdm.AfdError, match="afd_unipc_step_cfg: xc and hist must not overlap"):
            lib.afd_unipc_step_cfg(x, e, bad, hist, c, 3.0, o, o2, n, None)
    with pytest.raises(afdm.AfdError, match="afd_unipc_step_cfg: xc and hist must not overlap"):
        lib.afd_unipc_step_cfg(x, e, xc, at(80 - 3 * n + 1), c, 3.0, o, o2, n, None)          # hist reaching into x_out2


# ---- the public interface ------------------------------------------------------------------------------------------------------
def test_unipc_requests_that_are_refused_before_touching_a_device():
    import afdm
    d = _diff()
    m = afdm.UNet(c_in=1, c_out=1, image_size=32, f_settings=dict(F_SET), device="cpu", variant=3)
    for name in ("unipc", "unipc_1", "unipc_2", "unipc_3"):
        with pytest.raises(ValueError, match="needs steps"):
            d.sample(m, n=2, image_channels=1, sampler=name)
        with pytest.raises(ValueError, match="eta"):
            d.sample(m, n=2, image_channels=1, steps=10, eta=0.5, sampler=name)
        with pytest.raises(NotImplementedError, match="theta"):
            d.sample(m, n=2, image_channels=1, theta=30, steps=10, sampler=name)
        with pytest.raises(ValueError):
            d.sample(m, n=2, image_channels=1, steps=1000, sampler=name)              # steps = T
        with pytest.raises(ValueError, match="decreasing"):
            d.revert(m, n=1, image_channels=1, steps=[10, 20], sampler=name)
        with pytest.raises(ValueError, match="needs steps"):
            d.revert(m, n=1, image_channels=1, sampler=name)
    for bad in ("unipc_4", "unipc_0", "UniPC", 3):
        with pytest.raises(ValueError, match="unknown sampler") as ei:
            d.sample(m, n=2, image_channels=1, steps=10, sampler=bad)
        assert all(name in str(ei.value) for name in ("'unipc'", "'unipc_1'", "'unipc_2'", "'unipc_3'", "'dpmpp_2m'", "'ddim'"))
    with pytest.raises(ValueError, match="unknown sampler"):
        d.revert(m, n=2, image_channels=1, steps=10, sampler="unipc_4")
    assert m.training and m._t_range is None
    assert afdm.Diffusion.UNIPC_SAMPLERS == {"unipc": 2, "unipc_1": 1, "unipc_2": 2, "unipc_3": 3}
