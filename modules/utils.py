from afdm.training import set_seed, setup_logging  # noqa: F401
from afdm.imageio_utils import save_images, make_grid  # noqa: F401
from afdm.data import (get_data, get_data_MNIST, save_gen_images, save_dataset_MNIST, make_collage,  # noqa: F401
                       DeviceDataset, DeviceLoader, get_data_device, get_data_MNIST_device)
from afdm.ops import nn_search  # noqa: F401
from afdm.spectrum import compare_spectra, hann_window, power_spectrum, spectrum_bins  # noqa: F401
