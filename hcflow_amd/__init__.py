"""hcflow_amd -- MI355X-native HCFlow forward / inverse engine.

Host side (this package) mirrors the reference's arch-module interface; the compute lives in
hand-written HIP kernels behind the C ABI of include/hcflow.h (hcflow_amd/libhcflow_hip.so).
"""
from .config import NetConfig, preset, param_spec, eps_shapes  # noqa: F401
from .params import make_params  # noqa: F401
from .arch import HCFlowNet_SR, HCFlowNet_Rescaling  # noqa: F401
from . import latent  # noqa: F401
from . import data  # noqa: F401
from .data import ImageBank, BankLoader, draw_crops, prepare_batch, whole_image  # noqa: F401
from .data import PairedBank, PairedBankLoader, draw_paired_crops, center_crops, prepare_paired_batch, whole_pair  # noqa: F401
from . import resize  # noqa: F401
from .resize import imresize, lr_psnr  # noqa: F401
from . import losses  # noqa: F401
from .losses import (PixelLoss, ReconstructionLoss, CharbonnierLoss, GANLoss, Quantization, latent_l2,  # noqa: F401
                     finite_sum, ssim, SSIMLoss)

__all__ = ["NetConfig", "preset", "param_spec", "eps_shapes", "make_params", "HCFlowNet_SR", "HCFlowNet_Rescaling", "latent",
           "data", "ImageBank", "BankLoader", "draw_crops", "prepare_batch", "whole_image",
           "PairedBank", "PairedBankLoader", "draw_paired_crops", "center_crops", "prepare_paired_batch", "whole_pair",
           "resize", "imresize", "lr_psnr",
           "losses", "PixelLoss", "ReconstructionLoss", "CharbonnierLoss", "GANLoss", "Quantization", "latent_l2", "finite_sum",
           "ssim", "SSIMLoss"]
