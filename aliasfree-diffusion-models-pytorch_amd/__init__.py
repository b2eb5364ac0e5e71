"""afdm -- MI355X-native alias-free DDPM engine (hot path of MDFahimAnjum/AliasFree-Diffusion-Models-PyTorch).

Public surface = the reference's Python API for the hot path:
UNet, Diffusion, train, custom_upsample, custom_downsample, circularLowpassKernel, argument,
set_seed, EMA, plus the engine-side helpers TrainStep / FusedAdamW / GradAllReduce / LRSchedule / DistillStep / progressive_distill /
ConsistencyStep / consistency_distill / LossSecondMomentSampler / DeviceDataset / DeviceLoader.
Device work runs in libafd_hip.so (hand-written gfx950 kernels, C ABI in include/afd.h).
"""
from ._lib import AfdError, lib  # noqa: F401
from .filters import circularLowpassKernel, custom_downsample, custom_upsample  # noqa: F401
from .blocks import (SelfAttention, DoubleConv, DoubleConv_F, DoubleConv_F4, Down, Down_F, Down_FF, Down_FFF,  # noqa: F401
                     Down_F4, Up, Up_F, Up_FF, Up_FFF, Up_F4)
from .ops import NULL_LABEL, nn_search  # noqa: F401
from .spectrum import compare_spectra, hann_window, power_spectrum, spectrum_bins  # noqa: F401
from .fidelity import (FeatureStats, extract_features, feature_stats, fidelity, frechet_distance, inception_score,  # noqa: F401
                       kernel_distance, mmd_indices, mmd_sums)
from .manifold import ball_membership, manifold, manifold_scores, neighbour_radii  # noqa: F401
from .quality import gaussian_window, image_quality, pair_sums, psnr, ssim  # noqa: F401
from .posterior import LinearOperator, gaussian_kernel  # noqa: F401
from .likelihood import ode_likelihood_reference  # noqa: F401
from .unipc import unipc_reference  # noqa: F401
from .unet import UNet  # noqa: F401
from .diffusion import Diffusion  # noqa: F401
from .analytic import AnalyticVariance  # noqa: F401
from .training import (argument, set_seed, setup_logging, train, TrainStep, FusedAdamW, FlatParams,  # noqa: F401
                       GradAllReduce, EMA, LRSchedule, clip_coefficient, DistillStep, progressive_distill,
                       ConsistencyStep, consistency_distill, LossSecondMomentSampler)

from .tasks import (analytic_results, bpd_results, ddpm_run, edit_results, equivariance_results, fidelity_results, ilvr_results,  # noqa: F401
                    inpaint_results, likelihood_results, manifold_results, posterior_results, reconstruct_results, restoration_results,
                    rotation_results, shift_results, spectrum_results)
from .data import (get_data, get_data_MNIST, save_gen_images, make_collage, DeviceDataset, DeviceLoader,  # noqa: F401
                   get_data_device, get_data_MNIST_device)

__version__ = "0.1.0"
