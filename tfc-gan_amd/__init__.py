"""tfc-gan_amd: MI355X-native (gfx950) engine for the PATCH-16 training hot path of nudro/TFC-GAN.

Import name: ``tfc_gan_amd`` (the directory name carries a hyphen; the one-file loader ``tfc_gan_amd.py`` at the repository
root registers this package under the importable name).

Reference surface mirrored here (TFC-GAN-FFT/TFCGAN_multigpu_patchFFT_16P.py): UNetDown, UNetUp, GeneratorUNet,
Discriminator1 (alias Discriminator), weights_init_normal, make_16_patches, the 16-patch triplet head (ContrastiveLoss),
make_4_patches and the 4-patch heads of TFCGAN_multigpu_patchFFT.py / TFCGAN_multigpu_globalFFT.py (patches=4),
the regional FFT loss of the ..._withregion_FFT(.py|_KL.py) scripts (TrainStep(region_fft=...)),
the label-conditioned step of ..._debiased(.py|_V2.py|_V3.py) (TrainStep(labels=...), GeneratorUNet(labels=3), Discriminator1(aux_classes=(2, 4, 3))),
the edge-mask step of ..._experiment.py (TrainStep(mask=True), GeneratorUNet(mask=True), mask_maker, mask_l1_loss),
FFT_Components / fft_components / calculate_ffts, and the fused TrainStep + data-parallel layer (batch_scope="global": the batch-coupled mask and
KL terms take their extrema / softmax over the batch of all ranks).
Of the CycleGAN baseline (cyclegan_og/models.py): ResidualBlock and GeneratorResNet, the residual trunk on the reflect-padded 3x3 convolution op.
"""
import os as _os

# The step runs on two HIP streams (nets.py) and, with several GPUs, beside RCCL's stream. ROCm maps a process's streams onto GPU_MAX_HW_QUEUES hardware
# queues (default 4): with a process group alive the side stream came to share a hardware queue with busy work and the two-stream step ran 1.0 ms (10 %)
# SLOWER than without collectives -- measured with a one-rank "nccl" group; 8 queues bring it back to +0.2 ms. The runtime reads the
# variable when it initialises (first GPU call), so it is set here, before anything of this package touches the GPU; an explicit setting wins.
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

from . import _lib, data, engine, inference, losses, lpips, metrics, models, nets, ops, parallel, stn, stn21, synthetic, vit  # noqa: F401
from ._lib import TfcError, build  # noqa: F401
from .engine import TrainStep  # noqa: F401
from .nets import set_wgrad_stream  # noqa: F401
from .parallel import all_gather_records  # noqa: F401
from .data import DeviceLoader, ImageDataset, LabelledImageDataset, TestImageDataset, pair_resize_normalize  # noqa: F401
from .lpips import LPIPS  # noqa: F401
from .stn21 import DarkVisibleStep, STN21Step  # noqa: F401
from .stn import Warp, affine_warp, morph_gradient, morph_triplet, triplet_margin_rows  # noqa: F401
from .synthetic import synthetic_pairs, synthetic_temperatures  # noqa: F401
from .inference import global_grid, load_clean_state, save_checkpoint, stitch_16_patches, stitch_patches  # noqa: F401
from .losses import (ContrastiveLoss, FFT_Components, calculate_ffts, color_jitter_params, color_jitter_thermal, debias_weights,  # noqa: F401
                     fft_components, global_fft_loss, make_4_patches, make_16_patches, mask_l1_loss, mask_maker, mask_weights, mse_spec, other_spec, patch_fft_loss, patch_first_flat_index,
                     patch_triplet_loss, region_weights, regional_fft_components, regional_fft_loss, sample_spectra, temperature_triplet_loss,
                     vectorize_temps)
from .metrics import EvalAccumulator, bhattacharyya, mutual_information, ncc, psnr, ssim, to_gray, to_uint8  # noqa: F401
from .models import (BlurPool, Discriminator, Discriminator1, GeneratorResNet, GeneratorUNet, Pix2PixDiscriminator, ResidualBlock, UNetDown, UNetUp,  # noqa: F401
                     get_batch_invariant,
                     get_compute_dtype, set_batch_invariant, set_compute_dtype, weights_init_normal)

__all__ = ["UNetDown", "UNetUp", "GeneratorUNet", "Discriminator1", "Discriminator", "BlurPool", "weights_init_normal",
           "make_16_patches", "make_4_patches", "patch_first_flat_index", "stitch_patches", "ContrastiveLoss", "patch_triplet_loss", "FFT_Components", "fft_components", "calculate_ffts",
           "patch_fft_loss", "global_fft_loss", "regional_fft_components", "regional_fft_loss", "region_weights", "debias_weights", "mask_weights", "mask_maker", "mask_l1_loss", "mse_spec", "other_spec", "psnr", "ssim", "bhattacharyya", "ncc", "mutual_information", "to_uint8", "to_gray",
           "EvalAccumulator", "sample_spectra", "vectorize_temps", "temperature_triplet_loss", "color_jitter_thermal",
           "color_jitter_params", "synthetic_pairs", "synthetic_temperatures", "load_clean_state", "save_checkpoint", "stitch_16_patches", "global_grid", "TrainStep", "STN21Step", "DarkVisibleStep", "Pix2PixDiscriminator", "GeneratorResNet", "ResidualBlock", "LPIPS", "ImageDataset", "LabelledImageDataset", "TestImageDataset", "DeviceLoader", "pair_resize_normalize", "Warp", "affine_warp", "morph_gradient", "morph_triplet", "triplet_margin_rows", "set_compute_dtype", "get_compute_dtype", "set_batch_invariant", "get_batch_invariant", "build", "TfcError", "all_gather_records"]
