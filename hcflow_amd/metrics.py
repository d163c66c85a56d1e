"""Validation metrics on the GPU: the per-image block of the reference's test loop (test_HCFlow.py:103-182) --
``tensor2img`` + ``calculate_psnr_ssim`` (utils/util.py:790-816, 898-982), optionally on MATLAB-style bicubic
down-scaled copies (utils/imresize.py), and the sample diversity (``std`` over samples, test_HCFlow.py:165) --
computed by HIP kernels in float64 (include/hcflow.h: hcf_metric_*). No CPU fallback."""
import ctypes as C
import math
from typing import Dict, List

import numpy as np
import torch

from . import _lib

KEYS = ["psnr", "ssim", "psnr_y", "ssim_y", "bic_psnr", "bic_ssim", "bic_psnr_y", "bic_ssim_y"]


def _prep(t):
    assert t.is_cuda and t.dim() == 4 and t.shape[1] == 3, "expected a CUDA tensor [B,3,H,W]"
    return t.detach().to(torch.float32).contiguous()


def psnr_ssim(gt: torch.Tensor, sr: torch.Tensor, crop_border: int = 0, scale: int = 0) -> List[Dict[str, float]]:
    """Per image: PSNR / SSIM / PSNR_Y / SSIM_Y of tensor2img(gt) vs tensor2img(sr) (borders cropped), and for
    ``scale > 1`` the same four on the bicubic down-scaled pair (the "bicHR" columns of the reference's log line)."""
    gt, sr = _prep(gt), _prep(sr)
    assert gt.shape == sr.shape
    B, _, H, W = gt.shape
    out = np.zeros((B, 8), dtype=np.float64)
    _lib.launch("hcf_metric_psnr_ssim", gt.device, gt, sr, B, H, W, int(crop_border), int(scale), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(KEYS, map(float, row))) for row in out]


def imresize_down(x: torch.Tensor, scale: int) -> np.ndarray:
    """imresize(tensor2img(x) / 255., 1 / scale) * 255 as a float64 array [B, h, w, 3] in BGR order (0..255 units)."""
    x = _prep(x)
    B, _, H, W = x.shape
    h, w = math.ceil(H / scale), math.ceil(W / scale)
    out = np.zeros((B, 3, h, w), dtype=np.float64)
    _lib.launch("hcf_metric_imresize_down", x.device, x, B, H, W, int(scale), out.ctypes.data_as(C.c_void_p))
    return np.transpose(out, (0, 2, 3, 1))


def diversity(samples: List[torch.Tensor]) -> float:
    """torch.cat([s.unsqueeze(0) * 255 for s in samples], 0).std([0]).mean() (test_HCFlow.py:127,165)."""
    return float((torch.stack([s.float() for s in samples], 0) * 255).std(0).mean())


class SampleStats:
    """Per-pixel mean and std of a set of samples WITHOUT holding the samples: ``add`` folds one ``[B,3,H,W]`` fp32 batch (values
    in [0, 1]) into a float64 (mean, M2) pair per element (Welford's recurrence, include/hcflow.h: hcf_metric_stats_*), so the
    state is 16 bytes per element however many samples arrive -- less than the samples themselves from the fifth on.

    ``result()`` -> {"mean": [B,3,H,W] fp32, the per-pixel mean (the MMSE estimate of a stochastic SR model); "std": [B,3,H,W]
    fp32, the unbiased (n - 1) per-pixel std in the samples' units (the uncertainty map); "diversity": [B] float64 on the device,
    the mean over (c, y, x) of 255 * std -- the reference's ``torch.cat(sr_img_list).std([0]).mean()`` (test_HCFlow.py:131,167)
    per image, summed in float64 in a fixed order}. One sample gives std = 0 and diversity = 0.

    ``add`` is one launch, ``result`` two; neither synchronises, and ``result`` leaves the state alone: it may be called, and
    ``add`` continued, any number of times. An image's values do not depend on the rest of the batch, and two runs agree bit for
    bit. No CPU fallback."""

    def __init__(self, B: int, H: int, W: int, device):
        device = torch.device(device)
        if device.type != "cuda" or not torch.cuda.is_available():
            raise _lib.HcfError("SampleStats needs a GPU device (got %s); hcflow_amd has no CPU/PyTorch fallback" % (device,))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.shape = (int(B), 3, int(H), int(W))
        self.device = device
        self.count = 0
        self._bytes = int(_lib.load().hcf_metric_stats_bytes(int(B), int(H), int(W)))
        if self._bytes == 0:
            raise _lib.HcfError("SampleStats: invalid shape B=%d H=%d W=%d" % (B, H, W))
        self._state = torch.empty(self._bytes // 8, dtype=torch.float64, device=device)      # defined by the first add

    @classmethod
    def like(cls, sr: torch.Tensor) -> "SampleStats":
        """An empty accumulator for samples shaped like ``sr`` ([B,3,H,W]) on its device."""
        if sr.dim() != 4 or sr.shape[1] != 3:
            raise ValueError("SampleStats.like: expected [B,3,H,W], got %s" % (tuple(sr.shape),))
        return cls(sr.shape[0], sr.shape[2], sr.shape[3], sr.device)

    def reset(self) -> "SampleStats":
        self.count = 0
        return self

    def add(self, sr: torch.Tensor) -> "SampleStats":
        if tuple(sr.shape) != self.shape or sr.device != self.device:
            raise ValueError("SampleStats.add: expected %s on %s, got %s on %s" % (self.shape, self.device, tuple(sr.shape), sr.device))
        B, _, H, W = self.shape
        _lib.launch("hcf_metric_stats_add", self.device, self._state, self._bytes, _prep(sr), B, H, W, self.count + 1)
        self.count += 1
        return self

    def result(self) -> Dict[str, torch.Tensor]:
        if self.count < 1:
            raise ValueError("SampleStats.result: no sample has been added")
        B, _, H, W = self.shape
        mean = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        std = torch.empty(self.shape, dtype=torch.float32, device=self.device)
        div = torch.empty(B, dtype=torch.float64, device=self.device)
        _lib.launch("hcf_metric_stats_finish", self.device, self._state, self._bytes, B, H, W, self.count, mean, std, div)
        return {"mean": mean, "std": std, "diversity": div}
