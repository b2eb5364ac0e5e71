"""Worker for test_gpu_objective.test_two_rank_objective_step_equals_single_rank (launched by torch.distributed.run, gloo, every
rank on cuda:0): each rank trains its half of the golden batch for two steps with TrainStep(distributed=True,
loss_weighting="min_snr") on a cosine-schedule v-prediction Diffusion and saves its parameters and its losses."""
import argparse
import math
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FSET = {"kernel_size": 3, "kaiser_beta": 2, "omega_c_down": math.pi / 2, "omega_c_up": math.pi / 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import afdm
    g = np.load(os.path.join(ROOT, "tests", "golden", "train_step.npz"), allow_pickle=False)
    afdm.set_seed(42)
    model = afdm.UNet(c_in=3, c_out=3, image_size=32, f_settings=dict(FSET), device=dev, variant=3).to(dev)
    diff = afdm.Diffusion(noise_steps=1000, img_size=32, device=dev, schedule="cosine", prediction="v")
    step = afdm.TrainStep(model, diff, lr=3e-4, distributed=True, loss_weighting="min_snr")
    B = g["images"].shape[0] // world
    sl = slice(rank * B, (rank + 1) * B)
    T = lambda a: torch.from_numpy(np.asarray(a))
    losses = []
    for tk, ek in (("t0", "eps0"), ("t1", "eps1")):
        losses.append(float(step(T(g["images"][sl]).to(dev), t=T(g[tk][sl]), eps=T(g[ek][sl]).to(dev))))
    torch.cuda.synchronize()
    torch.save({"params": step.opt.fp.flat.cpu(), "losses": losses}, f"{args.out}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
