"""Thin counterpart of the reference's task orchestration (modules/ddpm_tasks.py) so `Train.ipynb`'s
`ddpm_run(params)` runs unmodified on the HIP engine.  Host-side glue only:
same `params` keys, run-directory layout, settings text and file names; the plotting / visual-check
cells of the reference are not reproduced (out of scope: visualisation)."""
import csv
import gc
import json
import logging
import os
from collections import namedtuple

import numpy as np
import torch

from .data import (DeviceDataset, get_data, get_data_MNIST, get_data_device, get_data_MNIST_device, make_collage,
                   normalisation_table, save_dataset_MNIST, save_gen_images)
from .diffusion import Diffusion
from .training import (argument, consistency_distill, diffusion_kwargs, ema_path, model_out_channels, progressive_distill, set_seed,
                       train)
from .unet import UNet


def _f_settings(params):
    if params["f_kernel"] is None:
        return None
    return {"kernel_size": params["f_kernel"], "kaiser_beta": params["f_beta"],
            "omega_c_down": params["f_down"], "omega_c_up": params["f_up"]}


DATA_KEYS = ("device_loader", "flip_prob", "dataset_cache")


def _loader(dataset_name, args, params=None):
    """(loader, dataset) of a run: the host loaders, or with params["device_loader"] the data set in device memory and a
    DeviceLoader over it (params["flip_prob"]: horizontal flips, seeded by the run's seed; params["dataset_cache"]: the .npz an
    image-folder data set is kept in between runs)."""
    params = params or {}
    if not params.get("device_loader"):
        for k in ("flip_prob", "dataset_cache"):
            if params.get(k):
                raise ValueError(f"ddpm_run: {k} needs device_loader: True (the host loaders have neither flips nor a cache)")
        return get_data_MNIST(args) if dataset_name == "MNIST" else get_data(args)
    kw = {"flip_prob": params.get("flip_prob") or 0.0, "seed": params.get("seed")}
    if dataset_name == "MNIST":
        return get_data_MNIST_device(args, **kw)
    return get_data_device(args, cache=params.get("dataset_cache"), **kw)


def _first_images(dataset, N):
    """The first N training images, in data set order: (N, C, H, W) float."""
    if isinstance(dataset, DeviceDataset):
        return dataset.batch(torch.arange(N))[0]
    return torch.stack([dataset[i][0] for i in range(N)])


def ddpm_run(params):
    v, name = params["unet_v"], params["dataset"]
    args = argument()
    args.run_name = f"DDPM_Uncondtional_{name}_{v}"           # (sic) spelling is part of the directory contract
    args.epochs, args.batch_size, args.image_size = params["epochs"], params["batchsize"], params["image_size"]
    args.image_channels, args.device, args.lr = params["image_channels"], params["device"], params["lr"]
    args.noise_steps, args.image_gen_n = params["noise_steps"], params["image_gen_per_epoch"]
    args.dataset_path = params["dataset_dir"]
    # optional EMA of the weights (EMA(ema_beta), step_start_ema = ema_start): train() keeps it and saves it beside the
    # checkpoint; the FID/KID image set is then drawn from it.  Without the keys nothing changes.
    use_ema = params.get("ema_beta") is not None
    if use_ema:
        args.ema_beta, args.ema_start = params["ema_beta"], params.get("ema_start", 2000)
    # optional gradient-norm clipping and learning-rate schedule (train() hands them to its TrainStep).  Without the keys nothing
    # changes, the settings file included.
    # optional training objective: "noise_schedule" ("linear" | "cosine") and "prediction" ("eps" | "v" | "x0") go to every
    # Diffusion of the run, "loss_weighting" ("min_snr" | "truncated_snr") and "snr_gamma" to train()'s TrainStep; same rule
    # "variance" ("fixed" | "learned": the UNet then emits 2 * image_channels) goes to every Diffusion and model of the run,
    # "vlb_lambda" to train()'s TrainStep; same rule
    # "t_sampler" ("loss_second_moment"), "t_sampler_history" and "t_sampler_uniform_prob" to train()'s timestep sampler; same rule
    opt_keys = [k for k in ("max_grad_norm", "lr_warmup", "lr_schedule", "lr_min_ratio", "noise_schedule", "prediction",
                            "loss_weighting", "snr_gamma", "variance", "vlb_lambda", "t_sampler", "t_sampler_history",
                            "t_sampler_uniform_prob") if params.get(k) is not None]
    for k in opt_keys:
        setattr(args, k, params[k])
    # optional device-resident data set: "device_loader": True keeps the training set in device memory and assembles every batch
    # there (data.DeviceLoader: the host loader's order and values), "flip_prob" mirrors rows left-right, "dataset_cache" names the
    # .npz an image-folder data set is kept in; same rule
    data_keys = [k for k in DATA_KEYS if params.get(k) is not None]
    if params.get("distill") is not None:
        _distill_cfg(params)                                   # a malformed key fails here, not after the training
    if params.get("consistency") is not None:
        _consistency_cfg(params)                               # (same rule)
    evals = _eval_cfgs(params)                                 # (and so does a malformed evaluation key: EVALS)
    cwd = os.getcwd()
    modelpath = os.path.join(cwd, f"models/DDPM_Uncondtional_{name}_{v}/ckpt_{name}_{v}.pt")
    f_settings = _f_settings(params)
    tr_dir = os.path.join(cwd, f"images/original/{name}")
    gen_dir = os.path.join(cwd, f"images/generated/{name}_{v}")
    logging.basicConfig(format="%(asctime)s - %(levelname)s: %(message)s", level=logging.INFO, datefmt="%I:%M:%S")
    seed = params["seed"]
    set_seed(seed)
    if torch.cuda.is_available():
        print("CUDA is available. Device:", torch.cuda.get_device_name(0))
    else:
        print("CUDA is not available.")

    settings = {
        "unet_v": v, "run_name": args.run_name, "epochs": args.epochs, "batch_size ": args.batch_size,
        "image_size": args.image_size, "image_channels": args.image_channels, "device": args.device, "lr": args.lr,
        "noise_steps": args.noise_steps, "image_gen_n": args.image_gen_n, "datapath": args.dataset_path,
        "modelpath": modelpath, "save_tr_data": params["save_trining"], "tr_save_path": tr_dir,
        "gen_savepath": gen_dir, "gen_per_batch": params["gen_per_batch"], "total_gen": params["gen_total"],
        "seed": seed, "collage_n_per_image": params["collage_n_per_image"], "collage_n": params["collage_n"],
        "dataset": name,
    }
    for k_out, k_in in (("kernel_size", "kernel_size"), ("kaiser_beta", "kaiser_beta"),
                        ("omega_c_down", "omega_c_down"), ("omega_c_up", "omega_c_up")):
        settings[k_out] = f_settings[k_in] if f_settings is not None else "None"
    for k in opt_keys + data_keys:
        settings[k] = params[k]
    text = "\n".join(f"{k}: {val}" for k, val in settings.items())
    print(text)
    run_dir = os.path.join(cwd, f"runs/DDPM_Uncondtional_{name}_{v}")
    os.makedirs(run_dir, exist_ok=True)
    with open(os.path.join(run_dir, f"settings_{name}_{v}.txt"), "w") as fh:
        fh.write(text)

    # smoke forward (the reference does this on the CPU; the HIP engine has no CPU path)
    net = UNet(c_in=args.image_channels, c_out=model_out_channels(args), image_size=args.image_size, f_settings=f_settings,
               device=args.device, variant=v).to(args.device)
    print(sum(p.numel() for p in net.parameters()))
    x = torch.randn(2, args.image_channels, args.image_size, args.image_size, device=args.device)
    with torch.no_grad():
        print(net(x, x.new_tensor([500] * x.shape[0]).long()).shape)
    del net

    # train
    set_seed(seed)
    dataloader, dataset = _loader(name, args, params)
    for e, cfg in evals.items():                               # an n beyond the training set fails here, not after the training
        if e.parse is not None:
            _check_n(f"{e.key} n", cfg["n"], e.n_min(cfg), dataset)
    model = UNet(c_in=args.image_channels, c_out=model_out_channels(args), image_size=args.image_size, f_settings=f_settings,
                 device=args.device, variant=v).to(args.device)
    diffusion = Diffusion(noise_steps=args.noise_steps, img_size=args.image_size, device=args.device, **diffusion_kwargs(args))
    loss_all = train(args, model_path=modelpath, dataloader=dataloader, model=model, diffusion=diffusion)
    with open(os.path.join(run_dir, f"trining_loss_MNIST_{v}.csv"), "w", newline="") as fh:     # (sic) reference file name
        csv.writer(fh).writerow(loss_all)
    torch.cuda.empty_cache()
    gc.collect()

    # reload, sample, revert
    set_seed(seed)
    model = UNet(c_in=args.image_channels, c_out=model_out_channels(args), image_size=args.image_size, f_settings=f_settings,
                 device=args.device, variant=v).to(args.device)
    model.load_state_dict(torch.load(modelpath, weights_only=True))
    diffusion = Diffusion(noise_steps=args.noise_steps, img_size=args.image_size, device=args.device, **diffusion_kwargs(args))
    x, _ = diffusion.sample(model, n=6, image_channels=args.image_channels)
    set_seed(seed)
    denoise_img = diffusion.revert(model, n=1, image_channels=args.image_channels)

    if params["save_trining"] and name == "MNIST":
        save_dataset_MNIST(tr_dir, _loader(name, args)[1])
    else:
        print("skipped saving training dataset")
    # optional DDIM for the FID/KID image set only: params["sample_steps"] (S, or an explicit list of timesteps) and
    # params["sample_eta"] (default 0, deterministic); params["sample_solver"]: None / "ddim", "dpmpp_2m" (DPM-Solver++(2M)) or
    # "unipc" / "unipc_1" / "unipc_2" / "unipc_3" (UniPC of that order; "unipc" = order 2), the last two kinds over the same
    # steps with eta 0; without them the full DDPM chain runs as before
    gen_kw = {}
    if params.get("sample_steps") is not None:
        gen_kw = {"steps": params["sample_steps"], "eta": params.get("sample_eta", 0.0)}
    if params.get("sample_solver") is not None:
        gen_kw["sampler"] = params["sample_solver"]
    gen_model = model
    if use_ema:
        gen_model = UNet(c_in=args.image_channels, c_out=model_out_channels(args), image_size=args.image_size, f_settings=f_settings,
                         device=args.device, variant=v).to(args.device)
        gen_model.load_state_dict(torch.load(ema_path(modelpath), weights_only=True))
    # optional progressive distillation: params["distill"] = {"start_steps", "end_steps", "iters", "lr"} halves the DDIM chain of
    # the model the image set is drawn from, round after round (training.progressive_distill; "iters" steps per round, "lr"
    # defaults to the run's), saves the student beside the checkpoint and draws the image set from it over its own chain, eta = 0
    distill = None
    if params.get("distill") is not None:
        distill, gen_model, gen_kw = _distill(params, args, diffusion, gen_model, modelpath, name, seed, dataloader)
    # optional consistency distillation: params["consistency"] = {"steps", "iters", "sample_steps", "lr", "target_beta"} distils the
    # model the image set is drawn from over its DDIM chain of "steps" steps in one run of "iters" iterations
    # (training.consistency_distill; "lr" defaults to the run's, "target_beta" to 0.95), saves the target network beside the
    # checkpoint and draws the image set from it with diffusion.consistency_sample(steps=sample_steps)
    consistency, draw = None, diffusion.sample
    if params.get("consistency") is not None:
        consistency, gen_model, gen_kw = _consistency(params, args, diffusion, gen_model, modelpath, name, seed, dataloader)
        draw = diffusion.consistency_sample
    keep_n = max([cfg["n"] for e, cfg in evals.items() if e.samples], default=0)
    generated = []                                             # the first images of the set that an evaluation asks for, uint8 as sampled
    for start in np.arange(0, params["gen_total"], params["gen_per_batch"]):
        fileno = np.arange(start, start + params["gen_per_batch"], 1)
        xg, _ = draw(gen_model, n=params["gen_per_batch"], image_channels=args.image_channels, **gen_kw)
        save_gen_images(gen_dir, xg, fileno)
        if start < keep_n:
            generated.append(xg[:keep_n - start])
    make_collage(gen_dir, gen_dir, params["collage_n_per_image"], params["collage_n"], args.image_size)
    torch.cuda.empty_cache()
    gc.collect()
    out = {"loss_all": loss_all, "sample": x, "revert": denoise_img, "modelpath": modelpath, "gen_dir": gen_dir}
    if use_ema:
        out["ema_modelpath"] = ema_path(modelpath)
    if distill is not None:
        out["distill"] = distill
    if consistency is not None:
        out["consistency"] = consistency
    dev_set = dataset if isinstance(dataset, DeviceDataset) else None      # (the host path loads its data set again, as before)
    ctx = EvalContext(params, args, diffusion, gen_model, run_dir, name, v, seed, dev_set, torch.cat(generated) if generated else None)
    for e, cfg in evals.items():
        out[e.out] = e.run(ctx, cfg)
    return out


def distill_path(model_path, end_steps):
    """Where `ddpm_run` writes a distilled student beside a checkpoint: ckpt_X.pt -> ckpt_X_distill{end_steps}.pt."""
    root, ext = os.path.splitext(model_path)
    return f"{root}_distill{int(end_steps)}{ext}"


def _distill_cfg(params):
    cfg = dict(params["distill"])
    unknown = sorted(set(cfg) - {"start_steps", "end_steps", "iters", "lr"})
    if unknown or not {"start_steps", "end_steps", "iters"} <= set(cfg):
        raise ValueError(f"ddpm_run: distill needs start_steps, end_steps and iters (and optionally lr); got {sorted(cfg)}")
    return cfg


def consistency_path(model_path, steps):
    """Where `ddpm_run` writes a consistency model beside a checkpoint: ckpt_X.pt -> ckpt_X_consistency{steps}.pt."""
    root, ext = os.path.splitext(model_path)
    return f"{root}_consistency{int(steps)}{ext}"


def _consistency_cfg(params):
    cfg = params["consistency"]
    if not isinstance(cfg, dict):
        raise ValueError(f"ddpm_run: consistency must be a dict with steps, iters and sample_steps (got {type(cfg).__name__})")
    cfg = dict(cfg)
    unknown = sorted(set(cfg) - {"steps", "iters", "sample_steps", "lr", "target_beta"})
    if unknown or not {"steps", "iters", "sample_steps"} <= set(cfg):
        raise ValueError(f"ddpm_run: consistency needs steps, iters and sample_steps (and optionally lr, target_beta); got {sorted(cfg)}")
    if params.get("distill") is not None:
        raise ValueError("ddpm_run: distill and consistency both replace the model the image set is drawn from: pass one of them")
    return cfg


def _consistency(params, args, diffusion, model, modelpath, name, seed, device_loader=None):
    """-> (out["consistency"], the target network, the sampler arguments of the image set).  device_loader: as for `_distill`."""
    cfg = _consistency_cfg(params)
    set_seed(seed)
    loader = device_loader if params.get("device_loader") else _loader(name, args)[0]
    kw = {} if cfg.get("target_beta") is None else {"target_beta": cfg["target_beta"]}
    net, info = consistency_distill(model, diffusion, loader, cfg["steps"], cfg["iters"], args.lr if cfg.get("lr") is None else cfg["lr"],
                                    args.device, **kw)
    path = consistency_path(modelpath, cfg["steps"])
    torch.save(net.state_dict(), path)
    return dict(info, modelpath=path, sample_steps=cfg["sample_steps"]), net, {"steps": cfg["sample_steps"]}


def _distill(params, args, diffusion, model, modelpath, name, seed, device_loader=None):
    """-> (out["distill"], the student, the sampler arguments of the image set).  device_loader: the run's DeviceLoader, if any."""
    cfg = _distill_cfg(params)
    set_seed(seed)
    loader = device_loader if params.get("device_loader") else _loader(name, args)[0]
    student, rounds = progressive_distill(model, diffusion, loader, cfg["start_steps"], cfg["end_steps"], cfg["iters"],
                                          args.lr if cfg.get("lr") is None else cfg["lr"], args.device)
    path = distill_path(modelpath, cfg["end_steps"])
    torch.save(student.state_dict(), path)
    return {"rounds": rounds, "modelpath": path}, student, {"steps": rounds[-1]["chain"], "eta": 0.0}


def _int_in(val, lo, hi, message):
    """val as a plain int if it is an int (numpy's count, a bool does not) with lo <= val <= hi (hi None: no upper end); else
    ValueError(message)."""
    if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < lo or (hi is not None and val > hi):
        raise ValueError(message)
    return int(val)


def _extractor_cfg(what, extractor):
    if not callable(extractor) and not isinstance(extractor, str):
        raise ValueError(f"ddpm_run: {what} extractor must be a callable, the path of a TorchScript file or 'pixels' (got "
                         f"{type(extractor).__name__})")
    if isinstance(extractor, str) and extractor != "pixels" and not os.path.isfile(extractor):
        raise ValueError(f"ddpm_run: {what} extractor {extractor!r} is neither 'pixels' nor an existing TorchScript file")


def _check_n(what, n, lo, dataset):
    """An evaluation's number of training images against the training set's size."""
    if not lo <= n <= len(dataset):
        raise ValueError(f"ddpm_run: {what} must lie in [{lo}, {len(dataset)}] (the training set's size; got {n})")


def _write_json(ctx, stem, table, line):
    """An evaluation's json beside the run's other files, and its one printed line."""
    with open(os.path.join(ctx.run_dir, f"{stem}_{ctx.name}_{ctx.v}.json"), "w") as fh:
        json.dump(table, fh, indent=1)
    print(line)


def _nearest_cfg(params):
    cfg = params["eval_nearest"]
    if not isinstance(cfg, dict) or set(cfg) - {"n", "k"} or "n" not in cfg:
        raise ValueError(f"ddpm_run: eval_nearest needs n (and optionally k); got "
                         f"{sorted(cfg) if isinstance(cfg, dict) else type(cfg).__name__}")
    cfg = {"n": cfg["n"], "k": cfg.get("k", 5)}
    for key, hi, why in (("n", params["gen_total"], "gen_total, the size of the generated set"), ("k", 16, "16")):
        cfg[key] = _int_in(cfg[key], 1, hi, f"ddpm_run: eval_nearest {key} must be an int in [1, {why}] (got {cfg[key]!r})")
    return cfg


def _training_store(name, args, dataset=None):
    """The run's DeviceDataset, or the host loaders' data set moved to the device once."""
    if dataset is not None:
        return dataset
    host = _loader(name, args)[1]
    return (DeviceDataset.from_tensor_dataset(host, device=args.device) if name == "MNIST" else
            DeviceDataset.from_folder(args.dataset_path, args.image_size, device=args.device))


def _eval_nearest(ctx, cfg):
    from .imageio_utils import save_images
    n, k, generated, run_dir, name, v = cfg["n"], cfg["k"], ctx.generated, ctx.run_dir, ctx.name, ctx.v
    dataset = _training_store(name, ctx.args, ctx.dataset)
    _check_n("eval_nearest n", n, 1, dataset)
    C = dataset.images.shape[1]
    queries = generated[:n].to(dataset.device)
    if dataset.images.dtype != torch.uint8:                    # a float store: the samples on its scale, as the loader maps pixels
        queries = normalisation_table(C).to(dataset.device)[torch.arange(C, device=dataset.device).view(1, C, 1, 1), queries.long()]
    dist, idx = dataset.nearest(queries, k)
    own = torch.arange(n, device=dataset.device)
    base_dist, base_idx = dataset.nearest(dataset.images[:n], k, exclude=own)
    res = {"dist": dist.cpu().numpy(), "idx": idx.cpu().numpy(), "baseline_dist": base_dist.cpu().numpy(),
           "baseline_idx": base_idx.cpu().numpy()}
    np.savez(os.path.join(run_dir, f"nearest_{name}_{v}.npz"), **res)
    # one row per sample: the sample, then its k neighbours (a slot with no neighbour left is black)
    rows = torch.where(idx < 0, torch.arange(n, device=idx.device).view(n, 1) - n, idx)
    pool = torch.cat([dataset.images, dataset.images.new_zeros((n,) + tuple(dataset.images.shape[1:]))])
    neigh = pool[rows.reshape(-1)]
    if neigh.dtype != torch.uint8:                             # back to pixels, as the samplers do: (x clamped to [-1, 1] + 1) / 2 * 255
        neigh = ((neigh.clamp(-1, 1) + 1) / 2 * 255).to(torch.uint8)
    neigh = neigh.view(n, k, *neigh.shape[1:])
    grid = torch.cat([generated[:n].to(neigh.device).unsqueeze(1), neigh], dim=1).reshape(n * (k + 1), *neigh.shape[2:])
    save_images(grid.cpu(), os.path.join(run_dir, f"nearest_{name}_{v}.jpg"), nrow=k + 1)
    print(f"nearest: median distance {np.median(res['dist'][:, 0]):.6g} (samples), {np.median(res['baseline_dist'][:, 0]):.6g} "
          f"(training images, leave-one-out)")
    return res


def _spectrum_cfg(params):
    cfg = params["eval_spectrum"]
    if not isinstance(cfg, dict) or set(cfg) - {"n", "window"} or "n" not in cfg:
        raise ValueError(f"ddpm_run: eval_spectrum needs n (and optionally window); got "
                         f"{sorted(cfg) if isinstance(cfg, dict) else type(cfg).__name__}")
    window = cfg.get("window", "hann")
    n = _int_in(cfg["n"], 1, params["gen_total"],
                f"ddpm_run: eval_spectrum n must be an int in [1, gen_total, the size of the generated set] (got {cfg['n']!r})")
    if window is not None and window != "hann":
        raise ValueError(f"ddpm_run: eval_spectrum window must be 'hann' or None (got {window!r})")
    if params.get("image_size") is not None and not 1 <= params["image_size"] <= 64:
        raise ValueError(f"ddpm_run: eval_spectrum takes images of at most 64 x 64 (image_size is {params['image_size']})")
    return {"n": n, "window": window}


def _spectrum_pair(train, generated, window, remove_mean=True):
    """The spectra of a DeviceDataset's first images and of as many generated uint8 images, and their comparison, as numpy arrays.
    A uint8 store and the samples go through the store's table; beside a float store the samples go through normalisation_table,
    as the loader maps pixels."""
    from .spectrum import compare_spectra, power_spectrum
    n, C = generated.shape[0], generated.shape[1]
    ref = train.power_spectrum(window=window, remove_mean=remove_mean, n=n)
    table = train.table if train.table is not None else normalisation_table(C)
    gen = power_spectrum(generated.to(train.device), table, window=window, remove_mean=remove_mean)
    db, lsd, hf_ratio = compare_spectra(ref, gen)
    return {"power_train": ref["power"].cpu().numpy(), "power_gen": gen["power"].cpu().numpy(), "radial_train": ref["radial"].cpu().numpy(),
            "radial_gen": gen["radial"].cpu().numpy(), "counts": ref["counts"].cpu().numpy(), "db": db.numpy(), "lsd": np.float64(lsd),
            "hf_ratio": np.float64(hf_ratio)}


def _eval_spectrum(ctx, cfg):
    n = cfg["n"]
    dataset = _training_store(ctx.name, ctx.args, ctx.dataset)
    _check_n("eval_spectrum n", n, 1, dataset)
    res = _spectrum_pair(dataset, ctx.generated[:n], cfg["window"])
    np.savez(os.path.join(ctx.run_dir, f"spectrum_{ctx.name}_{ctx.v}.npz"), **res)
    print(f"spectrum: log-spectral distance {res['lsd']:.4f} dB, high-frequency energy ratio {res['hf_ratio']:.4f} "
          f"({n} samples against {n} training images)")
    return res


def _fidelity_cfg(params):
    cfg = params["eval_fidelity"]
    if not isinstance(cfg, dict) or set(cfg) - {"n", "extractor", "kid_subsets", "kid_subset_size"} or not {"n", "extractor"} <= set(cfg):
        raise ValueError(f"ddpm_run: eval_fidelity needs n and extractor (and optionally kid_subsets, kid_subset_size); got "
                         f"{sorted(cfg) if isinstance(cfg, dict) else type(cfg).__name__}")
    n = _int_in(cfg["n"], 2, params["gen_total"],
                f"ddpm_run: eval_fidelity n must be an int in [2, gen_total, the size of the generated set] (got {cfg['n']!r})")
    _extractor_cfg("eval_fidelity", cfg["extractor"])
    out = {"n": n, "extractor": cfg["extractor"], "kid_subsets": cfg.get("kid_subsets", 100), "kid_subset_size": cfg.get("kid_subset_size", min(1000, n))}
    for key, lo, hi in (("kid_subsets", 1, None), ("kid_subset_size", 2, n)):
        out[key] = _int_in(out[key], lo, hi, f"ddpm_run: eval_fidelity {key} must be an int in [{lo}, {'...' if hi is None else 'n = ' + str(hi)}] "
                                             f"(got {out[key]!r})")
    return out


def _fidelity_pair(train, generated, cfg):
    """fidelity.fidelity of generated uint8 images against as many of a DeviceDataset's first images, read as pixels."""
    from .fidelity import fidelity
    n = generated.shape[0]
    return fidelity(generated.to(train.device), train.pixels(n), cfg["extractor"], kid_subsets=cfg["kid_subsets"],
                    kid_subset_size=cfg["kid_subset_size"])


def _eval_fidelity(ctx, cfg):
    n = cfg["n"]
    dataset = _training_store(ctx.name, ctx.args, ctx.dataset)
    _check_n("eval_fidelity n", n, 2, dataset)
    res = _fidelity_pair(dataset, ctx.generated[:n], cfg)
    _write_json(ctx, "fidelity", dict(res, n=n, kid_subsets=cfg["kid_subsets"], kid_subset_size=cfg["kid_subset_size"]),
                "fidelity: " + ", ".join(f"{k} {val:.6g}" for k, val in res.items()) + f" ({n} samples against {n} training images)")
    return res


def _manifold_cfg(params):
    cfg = params["eval_manifold"]
    if not isinstance(cfg, dict) or set(cfg) - {"n", "extractor", "k"} or not {"n", "extractor"} <= set(cfg):
        raise ValueError(f"ddpm_run: eval_manifold needs n and extractor (and optionally k); got "
                         f"{sorted(cfg) if isinstance(cfg, dict) else type(cfg).__name__}")
    k = _int_in(cfg.get("k", 3), 1, 16, f"ddpm_run: eval_manifold k must be an int in [1, 16] (got {cfg.get('k', 3)!r})")
    n = _int_in(cfg["n"], k + 1, params["gen_total"], f"ddpm_run: eval_manifold n must be an int in [k + 1 = {k + 1}, gen_total, the size of the "
                                                      f"generated set] (got {cfg['n']!r})")
    _extractor_cfg("eval_manifold", cfg["extractor"])
    return {"n": n, "extractor": cfg["extractor"], "k": k}


def _manifold_pair(train, generated, cfg):
    """manifold.manifold of generated uint8 images against as many of a DeviceDataset's first images, read as pixels."""
    from .manifold import manifold
    return manifold(generated.to(train.device), train.pixels(generated.shape[0]), cfg["extractor"], k=cfg["k"])


def _eval_manifold(ctx, cfg):
    n = cfg["n"]
    dataset = _training_store(ctx.name, ctx.args, ctx.dataset)
    _check_n("eval_manifold n", n, cfg["k"] + 1, dataset)
    res = _manifold_pair(dataset, ctx.generated[:n], cfg)
    _write_json(ctx, "manifold", dict(res, n=n, k=cfg["k"]), "manifold: " + ", ".join(f"{key} {val:.6g}" for key, val in res.items())
                + f" ({n} samples against {n} training images, k = {cfg['k']})")
    return res


RESTORATION_TASKS = ("inpaint", "superres")


def _restoration_mask(mask, S):
    """The (S, S) uint8 mask of `Diffusion.inpaint`, 1 = known: "center" (the hole is the central S/2 x S/2 square), "half" (the
    hole is the right half), or an (S, S) array of 0 / 1 taken as it is."""
    if isinstance(mask, str):
        if mask not in ("center", "half"):
            raise ValueError(f"restoration: mask must be 'center', 'half' or an ({S}, {S}) array of 0 / 1 (got {mask!r})")
        m = np.ones((S, S), dtype=np.uint8)
        if mask == "center":
            m[S // 4:S // 4 + S // 2, S // 4:S // 4 + S // 2] = 0
        else:
            m[:, S // 2:] = 0
        return m
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if m.shape != (S, S) or m.dtype.kind not in "biuf" or not np.isin(m, (0, 1)).all():
        raise ValueError(f"restoration: mask must be 'center', 'half' or an ({S}, {S}) array of 0 / 1 (got shape {m.shape}, {m.dtype})")
    return m.astype(np.uint8)


def _restoration_cfg(params):
    from .quality import gaussian_window
    cfg = params["eval_restoration"]
    keys = {"n", "mask", "factor", "tasks", "steps", "eta", "window", "sigma"}
    if not isinstance(cfg, dict) or set(cfg) - keys or "n" not in cfg:
        raise ValueError(f"ddpm_run: eval_restoration needs n (and optionally {', '.join(sorted(keys - {'n'}))}); got "
                         f"{sorted(cfg) if isinstance(cfg, dict) else type(cfg).__name__}")
    out = {"n": cfg["n"], "mask": cfg.get("mask", "center"), "factor": cfg.get("factor", 4), "tasks": cfg.get("tasks", RESTORATION_TASKS),
           "steps": cfg.get("steps"), "eta": cfg.get("eta", 0.0), "window": cfg.get("window", 11), "sigma": cfg.get("sigma", 1.5)}
    S = params.get("image_size")
    out["n"] = _int_in(out["n"], 1, None, f"ddpm_run: eval_restoration n must be an int >= 1 (got {out['n']!r})")
    tasks = (out["tasks"],) if isinstance(out["tasks"], str) else tuple(out["tasks"])
    if not tasks or any(t not in RESTORATION_TASKS for t in tasks) or len(set(tasks)) != len(tasks):
        raise ValueError(f"ddpm_run: eval_restoration tasks must be some of {RESTORATION_TASKS} (got {out['tasks']!r})")
    out["tasks"] = tasks
    factor, bad_factor = out["factor"], f"ddpm_run: eval_restoration factor must be a power of two >= 2 (got {out['factor']!r})"
    out["factor"] = _int_in(factor, 2, None, bad_factor)
    if factor & (factor - 1):
        raise ValueError(bad_factor)
    try:
        gaussian_window(out["window"], out["sigma"])
    except ValueError as e:
        raise ValueError(f"ddpm_run: eval_restoration {e}") from None
    if S is not None:
        if not 1 <= S <= 64 or out["window"] > S:
            raise ValueError(f"ddpm_run: eval_restoration takes images of at most 64 x 64 and no smaller than its window of "
                             f"{out['window']} taps (image_size is {S})")
        if "superres" in tasks and 2 * out["factor"] > S:
            raise ValueError(f"ddpm_run: eval_restoration factor must be at most image_size / 2 = {S // 2} (got {factor!r})")
        if "inpaint" in tasks:
            _restoration_mask(out["mask"], S)
    return out


def _spread(values):
    """A per-image fp64 tensor as {"mean", "std" (population), "values"}: plain floats, ready for json."""
    v = values.double().cpu()
    return {"mean": float(v.mean()), "std": float(v.std(unbiased=False)), "values": v.tolist()}


def _restoration_scores(diffusion, model, originals, cfg, seed, kw):
    """Inpaints and / or super-resolves the uint8 images `originals` (n, C, S, S), on the sampler's device, from their own
    degraded versions and scores the results against them; set_seed(seed) before each task."""
    from . import ops
    from .quality import gaussian_window, image_quality
    n, C, S = originals.shape[0], originals.shape[1], originals.shape[2]
    dev = originals.device
    win = gaussian_window(cfg["window"], cfg["sigma"])
    x0 = normalisation_table(C).to(dev)[torch.arange(C, device=dev).view(1, C, 1, 1), originals.long()]      # as the loader maps pixels
    skw = dict(kw, steps=cfg["steps"], eta=cfg["eta"])
    res = {"n": int(n), "window": int(cfg["window"]), "sigma": cfg["sigma"]}
    if "inpaint" in cfg["tasks"]:
        mask = _restoration_mask(cfg["mask"], S)
        set_seed(seed)
        filled = diffusion.inpaint(model, x0, torch.from_numpy(mask), **skw)[0]
        whole = image_quality(filled, originals, window=win)
        hole = image_quality(filled, originals, window=win, region=torch.from_numpy(1 - mask))
        res["inpaint"] = {"mask": cfg["mask"] if isinstance(cfg["mask"], str) else "custom", "hole_pixels": int((1 - mask).sum()),
                          "psnr": _spread(whole["psnr"]), "ssim": _spread(whole["ssim"]), "psnr_hole": _spread(hole["psnr"]),
                          "ssim_hole": _spread(hole["ssim"])}
    if "superres" in cfg["tasks"]:
        factor = cfg["factor"]
        taps, levels = diffusion._ilvr_operator("restoration", factor, None)
        with torch.no_grad():
            low = x0
            for _ in range(levels):
                low = ops.FiltDown2.apply(low, taps)
        reference = diffusion.reference_from_lowres(low, factor)
        set_seed(seed)
        sample, _, sample_float = diffusion.ilvr(model, reference, factor=factor, return_float=True, **skw)
        got, base = image_quality(sample, originals, window=win), image_quality(ops.quantize_u8(reference), originals, window=win)
        kept = image_quality(ops.lowpass_project(sample_float, taps, levels), ops.lowpass_project(x0, taps, levels), data_range=2.0, window=win)
        res["superres"] = {"factor": int(factor), "psnr": _spread(got["psnr"]), "ssim": _spread(got["ssim"]),
                           "psnr_reference": _spread(base["psnr"]), "ssim_reference": _spread(base["ssim"]),
                           "consistency_psnr": _spread(kept["psnr"])}
    return res


def _eval_restoration(ctx, cfg):
    n = cfg["n"]
    dataset = _training_store(ctx.name, ctx.args, ctx.dataset)
    _check_n("eval_restoration n", n, 1, dataset)
    res = _restoration_scores(ctx.diffusion, ctx.gen_model, dataset.pixels(n).to(ctx.args.device), cfg, ctx.seed, {})
    _write_json(ctx, "restoration", res, "\n".join(
        f"restoration {task}: " + ", ".join(f"{k} {val['mean']:.6g}" for k, val in res[task].items() if isinstance(val, dict))
        + f" (means over {n} training images)" for task in cfg["tasks"]))
    return res


def _eval_bpd(ctx, cfg=None):
    params, diffusion, run_dir, name, v = ctx.params, ctx.diffusion, ctx.run_dir, ctx.name, ctx.v
    N, K, sigma = int(params["eval_bpd"]), params.get("eval_bpd_t_samples"), params.get("eval_bpd_sigma", "beta")
    dataset = ctx.dataset if ctx.dataset is not None else _loader(name, ctx.args)[1]
    _check_n("eval_bpd", N, 1, dataset)
    images = _first_images(dataset, N)
    set_seed(ctx.seed)
    r = diffusion.calc_bpd(ctx.gen_model, images, sigma=sigma, t_samples=K)
    bpd = r["bpd"].numpy()
    se = float(bpd.std(ddof=1) / np.sqrt(N)) if N > 1 else float("nan")
    lines = [f"bpd: {bpd.mean():.6f}", f"bpd_stderr: {se:.6f}"]
    lines += [f"{k}: {float(r[k].mean()):.6f}" for k in ("prior_bpd", "vb_bpd", "decoder_bpd")]
    lines += [f"N: {N}", f"t_samples: {diffusion.noise_steps - 1 if K is None else int(K)}", f"sigma: {sigma}"]
    with open(os.path.join(run_dir, f"bpd_{name}_{v}.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return float(bpd.mean())


def _eval_equivariance(ctx, cfg=None):
    kw = dict(ctx.params["eval_equivariance"])
    N = int(kw.pop("N", 16))
    dataset = ctx.dataset if ctx.dataset is not None else _loader(ctx.name, ctx.args)[1]
    _check_n("eval_equivariance N", N, 1, dataset)
    images = _first_images(dataset, N).float()
    set_seed(ctx.seed)
    r = ctx.diffusion.equivariance(ctx.gen_model, images, **kw)
    t = kw["t"]
    table = {"t": [int(t)] if isinstance(t, (int, np.integer)) else [int(a) for a in t],
             "transforms": [list(sp) for sp in kw["transforms"]], "N": N, "margin": float(kw.get("margin", 4.0)),
             "peak": float(kw.get("peak", 2.0)), "count": r["count"].tolist(), "eq_db": r["eq_db"].tolist(),
             "snr_db": r["snr_db"].tolist()}
    _write_json(ctx, "equivariance", table, json.dumps(table))
    return table


# What a runner gets: the run's params and args, the sampler and the model the image set came from, where and under which names
# the run writes, the run's DeviceDataset (None on the host loaders: a runner loads the data set again, as before) and the first
# generated images that the evaluations asked to keep, uint8 as sampled (None if none did).
EvalContext = namedtuple("EvalContext", "params args diffusion gen_model run_dir name v seed dataset generated")

# One optional evaluation of ddpm_run: params[key] asks for it, parse(params) -> its config (None: the key is no dict and counts
# when it is truthy), samples: the first cfg["n"] generated images are kept for it, n_min(cfg): the smallest n it takes,
# run(ctx, cfg) -> out[out].  All of them score the model the FID/KID image set came from.
Eval = namedtuple("Eval", "key out parse samples n_min run")

EVALS = (                                                      # in the order they run and appear in ddpm_run's result
    # likelihood: params["eval_bpd"] = N scores the first N training images, in dataset order (Diffusion.calc_bpd;
    # "eval_bpd_t_samples": K timesteps per image, "eval_bpd_sigma": "beta", "posterior" or, with "variance": "learned", "learned")
    Eval("eval_bpd", "bpd", None, False, None, _eval_bpd),
    # equivariance scores: params["eval_equivariance"] = the keyword arguments of Diffusion.equivariance (t, transforms, margin,
    # peak, batch, ...) plus "N" (default 16), the number of training images scored, in dataset order
    Eval("eval_equivariance", "equivariance", None, False, None, _eval_equivariance),
    # nearest training images: params["eval_nearest"] = {"n": ..., "k": ...} (k defaults to 5) searches the training set for the
    # k nearest neighbours of the first n generated images, and of the first n training images (leave-one-out) as the baseline
    # the distances are read against (DeviceDataset.nearest)
    Eval("eval_nearest", "nearest", _nearest_cfg, True, lambda cfg: 1, _eval_nearest),
    # power spectra: params["eval_spectrum"] = {"n": ..., "window": "hann" | None} sets the mean power spectrum of the first n
    # generated images against that of the first n training images (spectrum.power_spectrum / compare_spectra)
    Eval("eval_spectrum", "spectrum", _spectrum_cfg, True, lambda cfg: 1, _eval_spectrum),
    # FID / KID / Inception Score: params["eval_fidelity"] = {"n": ..., "extractor": a callable, the path of a TorchScript file or
    # "pixels", "kid_subsets": ..., "kid_subset_size": ...} scores the first n generated images against the first n training
    # images through the extractor (fidelity.fidelity)
    Eval("eval_fidelity", "fidelity", _fidelity_cfg, True, lambda cfg: 2, _eval_fidelity),
    # precision / recall / density / coverage: params["eval_manifold"] = {"n": ..., "extractor": as for eval_fidelity, "k": ...}
    # (k defaults to 3) scores the first n generated images against the first n training images through the extractor
    # (manifold.manifold)
    Eval("eval_manifold", "manifold", _manifold_cfg, True, lambda cfg: cfg["k"] + 1, _eval_manifold),
    # restoration scores: params["eval_restoration"] = {"n": ..., "mask": "center" | "half" | an (S, S) array of 0 / 1, "factor":
    # ..., "tasks": ("inpaint", "superres"), "steps": ..., "eta": ..., "window": ..., "sigma": ...} inpaints and super-resolves the
    # first n training images and scores the results against them in PSNR and SSIM (quality.image_quality)
    Eval("eval_restoration", "restoration", _restoration_cfg, False, lambda cfg: 1, _eval_restoration),
)


def _eval_cfgs(params):
    """{entry of EVALS: its parsed config} of the evaluations that params asks for, in table order."""
    asked = [e for e in EVALS if (params.get(e.key) if e.parse is None else params.get(e.key) is not None)]
    return {e: e.parse(params) if e.parse is not None else None for e in asked}


def _load(model_data):
    args, v = model_data["args"], model_data["unet_v"]
    set_seed(model_data["seed"])
    model = UNet(c_in=args.image_channels, c_out=model_out_channels(args), image_size=args.image_size,
                 f_settings=model_data["f_settings"], device=args.device, variant=v).to(args.device)
    model.load_state_dict(torch.load(model_data["modelpath"], weights_only=True))
    # (a checkpoint trained with another noise schedule or parametrisation is evaluated as such: args.noise_schedule / .prediction)
    return model, Diffusion(noise_steps=args.noise_steps, img_size=args.image_size, device=args.device, **diffusion_kwargs(args)), args


def rotation_results(model_data, thatas):
    """Config E sweep (ddpm_tasks.py:346-369): the same seed for every angle, so only the rotation differs.
    One batched trajectory for all angles (identical noise for every angle, as the reference's per-angle re-seeding gives);
    under torch.distributed the angles are partitioned over the ranks and rank 0 gets the gathered lists (the other ranks
    get (None, None)) -- BASELINE config 5."""
    model, diffusion, args = _load(model_data)
    set_seed(model_data["seed"])
    return diffusion.sample_rotation_sweep_sharded(model, 4, args.image_channels, list(thatas))


def inpaint_results(model_data, images, mask, **kw):
    """Load the checkpoint as rotation_results does, seed, and fill the region of `images` where `mask` is 0
    (Diffusion.inpaint; **kw: steps, eta, labels, cfg_scale, jump_length, jump_n_sample, noise_source, graph, return_float)."""
    model, diffusion, _ = _load(model_data)
    set_seed(model_data["seed"])
    return diffusion.inpaint(model, images, mask, **kw)


def ilvr_results(model_data, reference, **kw):
    """Load the checkpoint as rotation_results does, seed, and draw samples that keep the coarse content of `reference`
    (Diffusion.ilvr; **kw: factor, t_stop, taps, steps, eta, labels, cfg_scale, noise_source, graph, return_float)."""
    model, diffusion, _ = _load(model_data)
    set_seed(model_data["seed"])
    return diffusion.ilvr(model, reference, **kw)


def analytic_results(model_data, images, out_dir=None, **kw):
    """Load the checkpoint as rotation_results does, seed, and estimate the Analytic-DPM table of the model over `images` (a
    DeviceDataset, or (N, C, H, W) uint8 pixels or float values: Diffusion.estimate_analytic_variance; **kw: timesteps,
    rows_per_step, batch, labels, cfg_scale, noise_source, noise_fn).  Writes analytic_<name>_<v>.npz (name =
    model_data["dataset"] when given, else the checkpoint's file stem; v = model_data["unet_v"]) into out_dir, by default the
    checkpoint's directory, and returns the AnalyticVariance with the file's path as `.path`: what
    `Diffusion.sample_analytic(steps=, eta=)` and `calc_bpd(sigma=)` take, and AnalyticVariance.load reads back."""
    model, diffusion, _ = _load(model_data)
    set_seed(model_data["seed"])
    av = diffusion.estimate_analytic_variance(model, images, **kw)
    name = model_data.get("dataset") or os.path.splitext(os.path.basename(model_data["modelpath"]))[0]
    out_dir = os.path.dirname(os.path.abspath(model_data["modelpath"])) if out_dir is None else out_dir
    os.makedirs(out_dir, exist_ok=True)
    av.path = os.path.join(out_dir, f"analytic_{name}_{model_data['unet_v']}.npz")
    av.save(av.path)
    return av


def bpd_results(model_data, images, **kw):
    """Load the checkpoint as rotation_results does, seed, and score `images` in bits/dim (Diffusion.calc_bpd; **kw: labels,
    sigma, t_samples, batch, noise_source, noise_fn, return_terms).  Returns calc_bpd's dict."""
    model, diffusion, _ = _load(model_data)
    set_seed(model_data["seed"])
    return diffusion.calc_bpd(model, images, **kw)


def _sample_against(who, model_data, images, n, lo, kw, parse=lambda n: None):
    """What spectrum_results, fidelity_results and manifold_results share: check n, parse the caller's options (they fail before
    the checkpoint is loaded), load, wrap the images, seed and draw n samples.  -> (the training store, the samples, parse(n))."""
    n = _int_in(n, lo, len(images), f"{who}: n must be an int in [{lo}, {len(images)}] (the number of images; got {n!r})")
    cfg = parse(n)
    model, diffusion, args = _load(model_data)
    train = images if isinstance(images, DeviceDataset) else DeviceDataset(images[:n], device=args.device)
    set_seed(model_data["seed"])
    x, _ = diffusion.sample(model, n=n, image_channels=args.image_channels, **kw)
    return train, x, cfg


def spectrum_results(model_data, images, n, window="hann", remove_mean=True, **kw):
    """Load the checkpoint as rotation_results does, seed, draw n samples (Diffusion.sample; **kw: steps, eta, sampler, ...) and set
    their mean power spectrum against that of the first n of `images`: a DeviceDataset, or (N, C, H, W) uint8 pixels or float32
    values on the loader's scale.  Returns the arrays ddpm_run writes for params["eval_spectrum"]: power_train, power_gen,
    radial_train, radial_gen, counts, db, lsd, hf_ratio."""
    train, x, _ = _sample_against("spectrum_results", model_data, images, n, 1, kw)
    return _spectrum_pair(train, x, window, remove_mean)


def fidelity_results(model_data, images, n, extractor, **kw):
    """Load the checkpoint as rotation_results does, seed, draw n samples (Diffusion.sample; **kw: steps, eta, sampler, ..., and
    kid_subsets / kid_subset_size, which are taken out first) and score them against the first n of `images`: a DeviceDataset, or
    (N, C, H, W) uint8 pixels or float32 values on the loader's scale.  Returns fidelity.fidelity's dict, as ddpm_run does for
    params["eval_fidelity"]."""
    kw = dict(kw)
    opt = {k: kw.pop(k) for k in ("kid_subsets", "kid_subset_size") if k in kw}
    train, x, cfg = _sample_against("fidelity_results", model_data, images, n, 2, kw,
                                    lambda n: _fidelity_cfg({"eval_fidelity": dict(opt, n=n, extractor=extractor), "gen_total": n}))
    return _fidelity_pair(train, x, cfg)


def manifold_results(model_data, images, n, extractor, k=3, **kw):
    """Load the checkpoint as rotation_results does, seed, draw n samples (Diffusion.sample; **kw: steps, eta, sampler, ...) and
    score them against the first n of `images`: a DeviceDataset, or (N, C, H, W) uint8 pixels or float32 values on the loader's
    scale.  Returns manifold.manifold_scores' dict, as ddpm_run does for params["eval_manifold"]."""
    train, x, cfg = _sample_against("manifold_results", model_data, images, n, 2, kw,
                                    lambda n: _manifold_cfg({"eval_manifold": {"n": n, "extractor": extractor, "k": k}, "gen_total": n}))
    return _manifold_pair(train, x, cfg)


def restoration_results(model_data, images, n, mask="center", factor=4, tasks=RESTORATION_TASKS, window=11, sigma=1.5, **kw):
    """Load the checkpoint as rotation_results does and score the model's restorations of the first n of `images` (a
    DeviceDataset, or (N, C, H, W) uint8 pixels) against the images themselves, in PSNR and SSIM (quality.image_quality with a
    Gaussian window of `window` taps and `sigma`); the seed is set before each task.  **kw: steps, eta, labels, cfg_scale, graph.
    "inpaint": `Diffusion.inpaint` with `mask`, 1 = known: "center" (the hole is the central S/2 x S/2 square), "half" (the right
    half) or an (S, S) array of 0 / 1; psnr and ssim over the whole image, psnr_hole and ssim_hole over the hole (region =
    1 - mask; SSIM over the windows centred in it).
    "superres": low = down2^L(images) with factor = 2^L, `Diffusion.ilvr` on `reference_from_lowres(low, factor)`; psnr and ssim
    of the sample, psnr_reference and ssim_reference of the quantised reference alone (the baseline to read them against), and
    consistency_psnr of ops.lowpass_project(sample) against ops.lowpass_project(image) in fp32 at data range 2: how far the sample
    left the measurement.
    Returns what ddpm_run writes for params["eval_restoration"]: {"n", "window", "sigma", task: {score: {"mean", "std" (population),
    "values": one per image}, ...}}."""
    n = _int_in(n, 1, len(images), f"restoration_results: n must be an int in [1, {len(images)}] (the number of images; got {n!r})")
    kw = dict(kw)
    cfg = {"n": n, "mask": mask, "factor": factor, "tasks": tasks, "window": window, "sigma": sigma}
    cfg.update({k: kw.pop(k) for k in ("steps", "eta") if k in kw})
    if isinstance(images, DeviceDataset):
        originals = images.pixels(n)
    else:
        originals = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
        if not isinstance(originals, torch.Tensor) or originals.dtype != torch.uint8 or originals.dim() != 4:
            raise ValueError("restoration_results: images must be a DeviceDataset or (N, C, H, W) uint8 pixels")
        originals = originals[:n]
    cfg = _restoration_cfg({"eval_restoration": cfg, "image_size": int(originals.shape[-1])})
    model, diffusion, args = _load(model_data)
    return _restoration_scores(diffusion, model, originals.to(args.device).contiguous(), cfg, model_data["seed"], kw)


def reconstruct_results(model_data, images, n, steps=50, refine=0, **kw):
    """Load the checkpoint as rotation_results does, seed, invert the first n of `images` (a DeviceDataset, or (N, C, H, W) uint8
    pixels, as restoration_results takes them) with `Diffusion.invert(steps, refine)` and decode the latents again with
    `Diffusion.decode(steps)`, eta = 0.  **kw: labels, cfg_scale, graph, given to both.  Returns {"n", "steps", "refine", "psnr" and
    "ssim" of the reconstructions against the images ({"mean", "std" (population), "values": one per image}; quality.image_quality),
    "latent_std": each latent's standard deviation (1 for a latent that looks like the noise the sampler starts from)}."""
    from .quality import image_quality
    n = _int_in(n, 1, len(images), f"reconstruct_results: n must be an int in [1, {len(images)}] (the number of images; got {n!r})")
    if isinstance(images, DeviceDataset):
        originals = images.pixels(n)
    else:
        originals = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
        if not isinstance(originals, torch.Tensor) or originals.dtype != torch.uint8 or originals.dim() != 4:
            raise ValueError("reconstruct_results: images must be a DeviceDataset or (N, C, H, W) uint8 pixels")
        originals = originals[:n]
    model, diffusion, args = _load(model_data)
    set_seed(model_data["seed"])
    originals = originals.to(args.device).contiguous()
    C = originals.shape[1]
    x0 = normalisation_table(C).to(args.device)[torch.arange(C, device=args.device).view(1, C, 1, 1), originals.long()]      # as the loader maps pixels
    latents = diffusion.invert(model, x0, steps, refine=refine, **kw)
    score = image_quality(diffusion.decode(model, latents, steps, **kw)[0], originals)
    return {"n": n, "steps": int(steps) if isinstance(steps, (int, np.integer)) else [int(t) for t in steps], "refine": int(refine),
            "psnr": _spread(score["psnr"]), "ssim": _spread(score["ssim"]),
            "latent_std": latents.flatten(1).double().std(dim=1, unbiased=False).tolist()}


def likelihood_results(model_data, images, n=4, steps=100, **kw):
    """Load the checkpoint as rotation_results does and score the first n of `images` (a DeviceDataset, or (N, C, H, W) uint8 pixels,
    as restoration_results takes them) in bits per dimension two ways: the model's own log-density from the probability-flow ODE
    (`Diffusion.ode_likelihood(steps)`; **kw: method, probes, probe, labels, dequantize, noise_source) and, beside it, `calc_bpd`'s
    variational bound of the same images (labels and noise_source are passed on).  The seed is set before each.  Returns {"n",
    "steps", "method", "probes", "probe", "bpd": {"mean", "std" (population), "values": one per image}, "logp", "trace_sem" (the
    same three of the log-density in nats and of the trace's standard error), "bound_bpd": calc_bpd's, the same three}."""
    n = _int_in(n, 1, len(images), f"likelihood_results: n must be an int in [1, {len(images)}] (the number of images; got {n!r})")
    if isinstance(images, DeviceDataset):
        originals = images.pixels(n)
    else:
        originals = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
        if not isinstance(originals, torch.Tensor) or originals.dtype != torch.uint8 or originals.dim() != 4:
            raise ValueError("likelihood_results: images must be a DeviceDataset or (N, C, H, W) uint8 pixels")
        originals = originals[:n]
    model, diffusion, args = _load(model_data)
    originals = originals.to(args.device).contiguous()
    C = originals.shape[1]
    x0 = normalisation_table(C).to(args.device)[torch.arange(C, device=args.device).view(1, C, 1, 1), originals.long()]      # as the loader maps pixels
    set_seed(model_data["seed"])
    ode = diffusion.ode_likelihood(model, x0, steps=steps, **kw)
    set_seed(model_data["seed"])
    bound = diffusion.calc_bpd(model, originals, **{k: kw[k] for k in ("labels", "noise_source") if k in kw})
    return {"n": n, "steps": int(steps) if isinstance(steps, (int, np.integer)) else [int(t) for t in steps],
            "method": kw.get("method", "heun"), "probes": int(kw.get("probes", 1)), "probe": kw.get("probe", "rademacher"),
            "bpd": _spread(ode["bpd"]), "logp": _spread(ode["logp"]), "trace_sem": _spread(ode["trace_sem"]),
            "bound_bpd": _spread(bound["bpd"])}


def posterior_results(model_data, images, operator, sigma=0.05, zeta=1.0, n=4, steps=100, eta=1.0, **kw):
    """Load the checkpoint as rotation_results does, measure the first n of `images` (a DeviceDataset, or (N, C, H, W) uint8 pixels,
    as restoration_results takes them) with `operator.measure(x0, sigma)` (a posterior.LinearOperator; the seed is set first) and
    restore them with `Diffusion.posterior_sample(zeta, steps, eta)` (steps=None: the DDPM chain, eta is then unused); the seed is
    set again before each restoration.  **kw: labels, noise_source.  Returns {"n", "steps", "eta", "sigma", "zeta", "psnr" and "ssim" of the restorations against the images
    ({"mean", "std" (population), "values": one per image}; quality.image_quality), "consistency": |A x - y| / |y| per image, x the
    unquantised restoration, and "baseline": the same three scores at zeta = 0, the unguided sampler from the same noise, which
    the scores are to be read against}."""
    from .posterior import LinearOperator
    from .quality import image_quality
    if not isinstance(operator, LinearOperator):
        raise ValueError(f"posterior_results: operator must be a posterior.LinearOperator (got {type(operator).__name__})")
    n = _int_in(n, 1, len(images), f"posterior_results: n must be an int in [1, {len(images)}] (the number of images; got {n!r})")
    if isinstance(images, DeviceDataset):
        originals = images.pixels(n)
    else:
        originals = torch.from_numpy(images) if isinstance(images, np.ndarray) else images
        if not isinstance(originals, torch.Tensor) or originals.dtype != torch.uint8 or originals.dim() != 4:
            raise ValueError("posterior_results: images must be a DeviceDataset or (N, C, H, W) uint8 pixels")
        originals = originals[:n]
    model, diffusion, args = _load(model_data)
    originals = originals.to(args.device).contiguous()
    C = originals.shape[1]
    x0 = normalisation_table(C).to(args.device)[torch.arange(C, device=args.device).view(1, C, 1, 1), originals.long()]      # as the loader maps pixels
    set_seed(model_data["seed"])
    y = operator.measure(x0, sigma)
    y_norm = y.double().flatten(1).norm(dim=1)

    def restore(z):
        set_seed(model_data["seed"])
        xq, _, x = diffusion.posterior_sample(model, y, operator, zeta=z, steps=steps, eta=eta if steps is not None else 0.0,
                                                 return_float=True, **kw)
        score = image_quality(xq, originals)
        gap = (operator.apply(x) - y).double().flatten(1).norm(dim=1) / y_norm
        return {"psnr": _spread(score["psnr"]), "ssim": _spread(score["ssim"]), "consistency": _spread(gap)}

    res = {"n": n, "steps": None if steps is None else (int(steps) if isinstance(steps, (int, np.integer)) else [int(t) for t in steps]),
           "eta": float(eta), "sigma": float(sigma), "zeta": float(zeta)}
    res.update(restore(zeta))
    res["baseline"] = restore(0.0)
    return res


def edit_results(model_data, images, t0, **kw):
    """Load the checkpoint as rotation_results does, seed, and edit `images` from noise level t0 (Diffusion.sdedit; **kw: steps,
    eta, labels, cfg_scale, noise_source, graph, return_float)."""
    model, diffusion, _ = _load(model_data)
    set_seed(model_data["seed"])
    return diffusion.sdedit(model, images, t0, **kw)


def equivariance_results(model_data, images, **kw):
    """Load the checkpoint as rotation_results does, seed, and score the model's equivariance on `images`
    (Diffusion.equivariance; **kw: t, transforms, margin, peak, labels, batch, noise_source, noise_fn).  Returns its dict."""
    model, diffusion, _ = _load(model_data)
    set_seed(model_data["seed"])
    return diffusion.equivariance(model, images, **kw)


def shift_results(model_data, shift):
    model, diffusion, args = _load(model_data)
    x_all = []
    for sh in shift:
        set_seed(model_data["seed"])
        x_all.append(diffusion.sample_shift(model, n=4, image_channels=args.image_channels, shift=sh))
    return x_all
