"""GPU tests of class-conditional sampling with classifier-free guidance (CFG): the null-label embedding add, the UNet with
mixed labelled / unlabelled rows against the CPU oracle, the fused guided denoise update, the conditional and guided
samplers (eager and graph replay), conditional train steps under graph replay and label dropout."""
import math

import pytest
import torch

from conftest import check, note, rel_l2

pytestmark = pytest.mark.gpu
F_SET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}
K = 10


@pytest.fixture(scope="module")
def A(gpu):
    import afdm
    return afdm, gpu


def _cond_model(afdm, dev, seed=42):
    afdm.set_seed(seed)
    return afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(F_SET), device=dev, variant=3, num_classes=K).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sd_cpu(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


def _oracle_mixed(R, sd, x, t, y):
    """UNet forward of the CPU oracle over rows with labels (y >= 0) and rows without (y < 0), in the original row order."""
    lab, null = (y >= 0).nonzero().flatten(), (y < 0).nonzero().flatten()
    out = torch.empty(x.shape[0], 3, *x.shape[2:], dtype=x.dtype)
    out[lab] = R.unet_forward(sd, x[lab], t[lab], 3, F_SET, y=y[lab])
    out[null] = R.unet_forward(sd, x[null], t[null], 3, F_SET)
    return out


# ---- 1. kernels: null-label embedding add --------------------------------------------------------------------------------
def test_null_label_embed_add_forward_and_backward(A):
    afdm, dev = A
    from afdm import ops
    L, p, st = afdm.lib(), ops._p, ops._stream()
    g = torch.Generator().manual_seed(1)
    B, D = 7, 256
    temb = torch.randn(B, D, generator=g).to(dev)
    table = torch.randn(K, D, generator=g).to(dev)
    y_full = torch.tensor([3, 4, 0, 12, 4, 9, 1], device=dev)          # 12: over range (clamps to K - 1)
    drop = torch.tensor([False, True, False, False, True, False, True], device=dev)
    y = y_full.masked_fill(drop, afdm.NULL_LABEL)                       # classes 1 and 4 now appear only as null labels
    y[6] = -5                                                           # any negative label is the null label
    out, ref = torch.empty_like(temb), torch.empty_like(temb)
    L.afd_label_embed_add_fwd(p(temb), p(table), p(y), p(out), B, D, K, st)
    L.afd_embed_add_fwd(p(temb), p(table), p(y), p(ref), B, D, K, st)
    assert _same_bits(out[drop], temb[drop])                            # null rows: a bit copy of temb
    assert _same_bits(out[~drop], ref[~drop])                           # labelled rows: exactly the old entry point
    assert torch.equal(ref[1], temb[1] + table[0])                      # (which clamps a negative label to class 0)
    inplace = temb.clone()
    L.afd_label_embed_add_fwd(p(inplace), p(table), p(y), p(inplace), B, D, K, st)
    assert _same_bits(inplace, out)

    # backward: over the mixed batch == over the labelled rows alone; a null row contributes to no class
    dout = torch.randn(B, D, generator=g).to(dev)
    d_mixed, d_lab = torch.empty(K, D, device=dev), torch.empty(K, D, device=dev)
    L.afd_embed_add_bwd(p(dout), p(y), p(d_mixed), B, D, K, 0, st)
    lab = (~drop).nonzero().flatten()
    dl, yl = dout[lab].contiguous(), y[lab].contiguous()
    L.afd_embed_add_bwd(p(dl), p(yl), p(d_lab), int(lab.numel()), D, K, 0, st)
    assert _same_bits(d_mixed, d_lab)
    assert float(d_mixed[[1, 4]].abs().max()) == 0.0
    # and through autograd (ops.EmbedAdd on the new forward, the old backward)
    tp = table.clone().requires_grad_(True)
    res = ops.EmbedAdd.apply(temb, tp, y)
    assert _same_bits(res.detach(), out)
    (gt,) = torch.autograd.grad(res, [tp], dout)
    assert _same_bits(gt, d_mixed)
    torch.cuda.synchronize()


# ---- 2 / 3. UNet with mixed labels vs the CPU oracle -----------------------------------------------------------------------
def _mixed_batch(dev):
    g = torch.Generator().manual_seed(4)
    x = torch.rand(6, 3, 32, 32, generator=g) * 2 - 1
    t = torch.tensor([500, 37, 999, 1, 250, 700])
    y = torch.tensor([2, -1, 7, -1, 0, -1])
    return x, t, y


def test_unet_forward_with_mixed_labels_vs_oracle(A):
    afdm, dev = A
    from oracle import ref_ops as R
    model = _cond_model(afdm, dev)
    x, t, y = _mixed_batch(dev)
    lab, null = y >= 0, y < 0
    with torch.no_grad():
        got = model(x.to(dev), t.to(dev), y.to(dev)).cpu()
        sep_lab = model(x[lab].to(dev), t[lab].to(dev), y[lab].to(dev)).cpu()
        sep_null = model(x[null].to(dev), t[null].to(dev)).cpu()
    ref = _oracle_mixed(R, _sd_cpu(model), x, t, y)
    e_lab = check("CFG: mixed-label UNet forward vs CPU oracle (labelled rows)", got[lab], ref[lab], 1e-5)
    e_null = check("CFG: mixed-label UNet forward vs CPU oracle (null rows)", got[null], ref[null], 1e-5)
    # measured on MI355X: the 6-row forward equals the two 3-row calls bit for bit (no kernel of this shape family splits its
    # work by the batch size), so the check is exact; a size whose convolutions split differently may only agree to ~1e-6
    assert torch.equal(got[lab], sep_lab) and torch.equal(got[null], sep_null)
    print(f"mixed labels: vs oracle {e_lab:.2e} / {e_null:.2e}; equal to the separate labelled / unlabelled calls bit for bit")


def test_unet_backward_with_mixed_labels_vs_oracle(A):
    afdm, dev = A
    from oracle import ref_ops as R
    model = _cond_model(afdm, dev)
    x, t, y = _mixed_batch(dev)
    dy = torch.randn(6, 3, 32, 32, generator=torch.Generator().manual_seed(8))
    names = ["label_emb.weight", "outc.weight", "outc.bias", "down1.emb_layer.1.weight", "up3.emb_layer.1.bias"]
    params = dict(model.named_parameters())
    pred = model(x.to(dev), t.to(dev), y.to(dev))
    got = torch.autograd.grad(pred, [params[k] for k in names], dy.to(dev))
    sd = _sd_cpu(model)
    for k in names:
        sd[k] = sd[k].clone().requires_grad_(True)
    ref = torch.autograd.grad(_oracle_mixed(R, sd, x, t, y), [sd[k] for k in names], dy)
    worst = max(check("CFG: mixed-label UNet backward vs CPU oracle autograd", a.cpu(), b, 1e-5, k)
                for k, a, b in zip(names, got, ref))
    assert float(got[0][[1, 3, 4, 5, 6, 8, 9]].abs().max()) == 0.0      # only classes 0, 2, 7 carry labels
    print(f"mixed labels backward: worst parameter-gradient rel-L2 {worst:.2e}")


# ---- 4. the fused guided update ----------------------------------------------------------------------------------------
def _lerp_restated(u, c, s):
    """ATen's scalar lerp (aten/src/ATen/native/Lerp.h), one device op per step."""
    d = c - u
    if abs(s) < 0.5:
        return u + d * s
    oms = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(s, dtype=torch.float32))
    return c - d * oms


@pytest.mark.parametrize("form", ["host", "dev"])
@pytest.mark.parametrize("i", [999, 500, 2, 1])
@pytest.mark.parametrize("s", [0.3, 0.5, 3.0])
def test_fused_cfg_update_equals_lerp_then_denoise_step(A, s, i, form):
    afdm, dev = A
    from afdm import ops
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    g = torch.Generator().manual_seed(100 + i)
    for shape in ((3, 3, 32, 32), (3, 3, 5, 7)):                         # 16-byte path and scalar path (n % 4 != 0)
        n = shape[0]
        x = torch.randn(shape, generator=g).to(dev)
        eps2 = torch.randn((2 * n,) + shape[1:], generator=g).to(dev)
        noise = torch.randn(shape, generator=g).to(dev) if i > 1 else None
        c, u = eps2[:n], eps2[n:]
        e = _lerp_restated(u, c, s)
        e_lerp = torch.lerp(u, c, s)
        note("CFG: restated lerp vs torch.lerp", rel_l2(e, e_lerp), (s, i))
        assert rel_l2(e, e_lerp) < 1e-6
        want = ops.denoise_step(x, e, noise, diff.alpha, diff.alpha_hat, diff.beta, i)
        out2 = torch.full_like(x, float("nan"))
        if form == "host":
            got = ops.denoise_step_cfg(x, eps2, noise, diff.alpha, diff.alpha_hat, diff.beta, i, s, out2=out2)
        else:
            t_dev = torch.full((2 * n,), i, device=dev, dtype=torch.long)
            got = x.clone()                                              # in place, as the captured sampler step runs it
            ops.denoise_step_cfg_dev(got, eps2, noise, diff.alpha, diff.alpha_hat, diff.beta, t_dev, s, got, out2)
        assert _same_bits(got, want), (shape, s, i, form)
        assert _same_bits(out2, got)
    torch.cuda.synchronize()


# ---- 5-7. sampling -----------------------------------------------------------------------------------------------------
def test_conditional_sample_equals_hand_loop(A):
    afdm, dev = A
    from afdm import ops
    model = _cond_model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=12, img_size=32, device=dev)
    labels = torch.tensor([3, afdm.NULL_LABEL, 7], device=dev)
    afdm.set_seed(5)
    xq, rq, xf = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True, labels=labels)
    assert model.training
    afdm.set_seed(5)
    model.eval()
    with torch.no_grad():
        x = torch.randn((3, 3, 32, 32), device=dev)
        for i in reversed(range(1, diff.noise_steps)):
            eps = model(x, torch.full((3,), i, device=dev, dtype=torch.long), labels)
            noise = torch.randn_like(x) if i > 1 else None
            x = ops.denoise_step(x, eps, noise, diff.alpha, diff.alpha_hat, diff.beta, i)
    model.train()
    assert torch.equal(xf, x) and torch.equal(xq, ops.quantize_u8(x))
    afdm.set_seed(5)                                                    # the labels change the images, the noise is the same
    x_unc = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True)[2]
    assert not torch.equal(x_unc[0], xf[0])


def test_guided_sample_equals_batched_hand_loop(A):
    afdm, dev = A
    from afdm import ops
    model = _cond_model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=12, img_size=32, device=dev)
    labels = [3, afdm.NULL_LABEL, 7]
    afdm.set_seed(5)
    xq, rq, xf = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True, labels=labels, cfg_scale=3.0)
    afdm.set_seed(5)
    y2 = torch.tensor(labels + [afdm.NULL_LABEL] * 3, device=dev)
    model.eval()
    with torch.no_grad():
        x = torch.randn((3, 3, 32, 32), device=dev)
        for i in reversed(range(1, diff.noise_steps)):
            eps2 = model(torch.cat([x, x]), torch.full((6,), i, device=dev, dtype=torch.long), y2)
            noise = torch.randn_like(x) if i > 1 else None
            x = ops.denoise_step_cfg(x, eps2, noise, diff.alpha, diff.alpha_hat, diff.beta, i, 3.0)
    model.train()
    assert torch.equal(xf, x) and torch.equal(xq, ops.quantize_u8(x))


def test_guided_sample_vs_upstream_two_forward_oracle_loop(A):
    """Upstream's CFG loop on the CPU oracle (two forwards, torch.lerp, the reference's update) fed the same noise."""
    afdm, dev = A
    from oracle import ref_ops as R
    model = _cond_model(afdm, dev)
    T, n = 10, 2
    diff = afdm.Diffusion(noise_steps=T, img_size=32, device=dev)
    labels = torch.tensor([4, 9])
    afdm.set_seed(13)
    xf = diff.sample(model, n=n, image_channels=3, noise_source="cpu", return_float=True, labels=labels, cfg_scale=3.0)[2].cpu()
    sd = _sd_cpu(model)
    beta, alpha, alpha_hat = R.noise_schedule(T)
    afdm.set_seed(13)
    x = torch.randn((n, 3, 32, 32))
    with torch.no_grad():
        for i in reversed(range(1, T)):
            t = torch.full((n,), i, dtype=torch.long)
            ec = R.unet_forward(sd, x, t, 3, F_SET, y=labels)
            eu = R.unet_forward(sd, x, t, 3, F_SET)
            e = torch.lerp(eu, ec, 3.0)
            nz = torch.randn_like(x) if i > 1 else torch.zeros_like(x)
            x = R.denoise_step(beta, alpha, alpha_hat, x, e, i, nz)
    err = check("CFG: 9-step guided sample vs upstream's two-forward loop on the CPU oracle", xf, x, 1e-5)
    print(f"guided sample (T=10, n=2, s=3) vs oracle loop: rel-L2 {err:.2e}")


@pytest.mark.parametrize("cfg_scale", [0.0, 3.0])
def test_graph_conditional_sampling_equals_eager(A, cfg_scale):
    afdm, dev = A
    model = _cond_model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=31, img_size=32, device=dev)
    labels = torch.tensor([1, afdm.NULL_LABEL, 8], device=dev)
    outs = []
    for use_graph in (False, True):
        afdm.set_seed(5)
        xq, rq, xf = diff.sample(model, n=3, image_channels=3, noise_source="device", return_float=True, graph=use_graph,
                                 labels=labels, cfg_scale=cfg_scale)
        outs.append((xq.cpu(), rq.cpu(), xf.cpu()))
    assert model.training
    assert torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- 8 / 9. training ---------------------------------------------------------------------------------------------------
def _train_inputs(dev, B=8, steps=3):
    g = torch.Generator().manual_seed(17)
    images = (torch.rand(B, 3, 32, 32, generator=g) * 2 - 1).to(dev)
    ts = [torch.randint(1, 1000, (B,), generator=g) for _ in range(steps)]
    es = [torch.randn(B, 3, 32, 32, generator=g).to(dev) for _ in range(steps)]
    ys = [torch.randint(0, K, (B,), generator=g) for _ in range(steps)]
    for k, y in enumerate(ys):
        y[k::3] = -1                                                    # some rows of every batch carry no label
    return images, ts, es, [y.to(dev) for y in ys]


def test_conditional_train_step_graph_and_lanes_equal_eager(A):
    afdm, dev = A
    images, ts, es, ys = _train_inputs(dev)
    outs = {}
    for mode in (False, True, "lanes"):
        model = _cond_model(afdm, dev)
        diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
        step = afdm.TrainStep(model, diff, lr=3e-4, graph=mode, conditional=True)
        losses = [step(images, t=t, eps=e, y=y).item() for t, e, y in zip(ts, es, ys)]
        outs[mode] = (losses, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu())
        if mode is True:
            graph_step = step
    for mode in (True, "lanes"):
        dl = [abs(a - b) for a, b in zip(outs[False][0], outs[mode][0])]
        e = rel_l2(outs[mode][1], outs[False][1])
        note("CFG: conditional captured step vs eager (parameters after 3 steps)", e, mode)
        print(f"conditional step {mode} vs eager: loss diffs {dl}, param rel-L2 {e:.2e}")
        assert dl[0] < 1e-6 and max(dl[1:]) < 1e-5 and e < 1e-6
    assert torch.equal(outs["lanes"][1], outs[True][1]) and outs["lanes"][0] == outs[True][0]
    with pytest.raises(ValueError, match="class labels"):
        graph_step(images, t=ts[0], eps=es[0])                          # captured with labels: they are required
    model = _cond_model(afdm, dev)
    step = afdm.TrainStep(model, afdm.Diffusion(noise_steps=1000, img_size=32, device=dev), lr=3e-4, graph="lanes", conditional=True)
    assert math.isfinite(step(images, t=ts[0], eps=es[0]).item())      # captured without labels ...
    with pytest.raises(ValueError, match="class labels"):
        step(images, t=ts[1], eps=es[1], y=ys[1])                       # ... so they are refused


def test_label_dropout(A):
    afdm, dev = A
    from afdm.training import label_dropout_mask
    images, ts, es, ys = _train_inputs(dev, B=16)
    lr, wd = 3e-4, 0.01
    y_all = torch.arange(16, device=dev) % K

    # p_uncond = 1: every label dropped, label_emb gets a zero gradient: AdamW only decays its rows
    model = _cond_model(afdm, dev)
    before = model.label_emb.weight.detach().clone()
    step = afdm.TrainStep(model, afdm.Diffusion(noise_steps=1000, img_size=32, device=dev), lr=lr, conditional=True, p_uncond=1.0)
    step(images, t=ts[0], eps=es[0], y=y_all)
    assert bool((step.last_labels == afdm.NULL_LABEL).all())
    assert float((model.label_emb.weight.detach() - before * (1 - lr * wd)).abs().max()) < 1e-6

    # p_uncond = 0: bit-identical to a step built without the argument, and no extra draw from the CPU generator
    runs = []
    for kw in ({}, {"p_uncond": 0.0}):
        model = _cond_model(afdm, dev)
        step = afdm.TrainStep(model, afdm.Diffusion(noise_steps=1000, img_size=32, device=dev), lr=lr, conditional=True, **kw)
        afdm.set_seed(9)
        losses = [step(images, eps=e, y=y).item() for e, y in zip(es, ys)]
        runs.append((losses, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu(), torch.get_rng_state()))
    assert runs[0][0] == runs[1][0] and _same_bits(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])

    # p_uncond = 0.3 under the two-lane replay: the dropped labels are exactly the CPU draw next to the timesteps
    model = _cond_model(afdm, dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev)
    step = afdm.TrainStep(model, diff, lr=lr, graph="lanes", conditional=True, p_uncond=0.3)
    afdm.set_seed(21)
    got = []
    for e in es:
        assert math.isfinite(step(images, eps=e, y=y_all).item())
        got.append((step.last_labels == afdm.NULL_LABEL).cpu())
    afdm.set_seed(21)
    want = []
    for _ in es:
        diff.sample_timesteps(16)
        want.append(label_dropout_mask(16, 0.3))
    for g_, w_ in zip(got, want):
        assert torch.equal(g_, w_)
    frac = float(torch.cat(got).float().mean())
    assert frac == float(torch.cat(want).float().mean()) and 0.0 < frac < 1.0
    print(f"label dropout p_uncond=0.3: dropped fraction {frac:.3f} over {len(got)} steps of 16")
