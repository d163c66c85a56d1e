"""Validation metrics on the GPU: the per-image block of the reference's test loop (test_HCFlow.py:103-182) --
``tensor2img`` + ``calculate_psnr_ssim`` (utils/util.py:790-816, 898-982), optionally on MATLAB-style bicubic
down-scaled copies (utils/imresize.py), and the sample diversity (``std`` over samples, test_HCFlow.py:165) --
computed by HIP kernels in float64 (include/hcflow.h: hcf_metric_*). No CPU fallback."""
import ctypes as C
import math
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

KEYS = ["psnr", "ssim", "psnr_y", "ssim_y", "bic_psnr", "bic_ssim", "bic_psnr_y", "bic_ssim_y"]


def _prep(t):
    assert t.is_cuda and t.dim() == 4 and t.shape[1] == 3, "expected a CUDA tensor [B,3,H,W]"
    return t.detach().to(torch.float32).contiguous()


def psnr_ssim(gt: torch.Tensor, sr: torch.Tensor, crop_border: int = 0, scale: int = 0) -> List[Dict[str, float]]:
    """Per image: PSNR / SSIM / PSNR_Y / SSIM_Y of tensor2img(gt) vs tensor2img(sr) (borders cropped), and for
    ``scale > 1`` the same four on the bicubic down-scaled pair (the "bicHR" columns of the reference's log line).

    A one-shot ``PairMetrics.embed`` + ``compare`` inside the library (it allocates, prepares the GT, compares, reads back and
    synchronises per call): the numbers equal ``PairMetrics.compare``'s bit for bit, two calls agree bit for bit, and an
    image's numbers do not depend on the rest of the batch. For many samples of one GT use ``PairMetrics``."""
    gt, sr = _prep(gt), _prep(sr)
    assert gt.shape == sr.shape
    B, _, H, W = gt.shape
    out = np.zeros((B, 8), dtype=np.float64)
    _lib.launch("hcf_metric_psnr_ssim", gt.device, gt, sr, B, H, W, int(crop_border), int(scale), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(KEYS, map(float, row))) for row in out]


def imresize_down(x: torch.Tensor, scale: int) -> np.ndarray:
    """imresize(tensor2img(x) / 255., 1 / scale) * 255 as a float64 array [B, h, w, 3] in BGR order (0..255 units), ``scale >= 2``:
    the down-scaled planes ``PairMetrics.embed`` keeps of a GT (rows first, not re-quantised), i.e. the ones ``psnr_ssim`` and
    ``PairMetrics.compare`` measure against. Reproducible bit for bit; an image's planes do not depend on the rest of the batch."""
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


class MetricRef:
    """What ``PairMetrics.embed`` returns: one GT batch prepared for comparison in a device buffer (private layout), the shape,
    ``crop_border`` and ``scale`` it was prepared for, and the scratch its ``compare`` calls run in (they share it: issue the
    compares of one reference on one stream)."""

    def __init__(self, store, shape, crop_border, scale, work):
        self.store, self.shape, self.crop_border, self.scale, self.work = store, tuple(shape), int(crop_border), int(scale), work


class PairMetrics:
    """``psnr_ssim``'s eight numbers for many samples against ONE GT, kept on the device (include/hcflow.h: hcf_metric_pair_*):

        pm = PairMetrics()
        ref = pm.embed(gt, crop_border=4, scale=4)      # GT quantised, down-scaled and its tables uploaded once
        m = pm.compare(ref, sr)                         # [B,8] float64 CUDA tensor in KEYS order; no host sync
        m, u8 = pm.compare(ref, sr, image=True)         # + [B,H,W,3] uint8 BGR = util.tensor2img(sr) per image
        acc = pm.sample_set(gt, crop_border=4, scale=4)
        for sr in samples: acc.add(sr)                  # one compare into row M of a [capacity,B,8] buffer
        r = acc.result()                                # per_sample [M,B,8], mean [B,8], best_psnr / best_psnr_index [B]

    ``out=`` / ``image_out=`` write into the caller's tensors; with them ``compare`` allocates nothing (the scratch belongs to the
    reference). Two runs agree bit for bit and an image's row does not depend on the rest of the batch. ``rows_to_dicts`` turns a
    result into ``psnr_ssim``'s list of dicts. No CPU fallback."""

    def embed(self, gt: torch.Tensor, crop_border: int = 0, scale: int = 0) -> MetricRef:
        if not torch.is_tensor(gt) or not gt.is_cuda:
            raise _lib.HcfError("PairMetrics needs a GPU tensor (got %s); hcflow_amd has no CPU fallback"
                                % (gt.device if torch.is_tensor(gt) else type(gt).__name__,))
        if gt.dim() != 4 or gt.shape[1] != 3:
            raise _lib.HcfError("PairMetrics.embed: expected [B,3,H,W], got %s" % (tuple(gt.shape),))
        B, _, H, W = gt.shape
        lib = _lib.load()
        need = int(lib.hcf_metric_pair_ref_bytes(B, H, W, int(scale)))
        wneed = int(lib.hcf_metric_pair_workspace(B, H, W, int(scale)))
        if need == 0 or wneed == 0:
            raise _lib.HcfError("PairMetrics.embed: invalid shape %s or scale %d" % (tuple(gt.shape), scale))
        store = torch.empty(need, dtype=torch.uint8, device=gt.device)
        work = torch.empty(wneed, dtype=torch.uint8, device=gt.device)
        _lib.launch("hcf_metric_pair_embed", gt.device, _prep(gt), B, H, W, int(crop_border), int(scale), store, need)
        return MetricRef(store, gt.shape, crop_border, scale, work)

    def _check(self, ref: MetricRef, sr: torch.Tensor):
        if not isinstance(ref, MetricRef):
            raise TypeError("PairMetrics: ref must come from PairMetrics.embed, got %s" % type(ref).__name__)
        if not torch.is_tensor(sr) or tuple(sr.shape) != ref.shape or sr.device != ref.store.device:
            raise _lib.HcfError("PairMetrics: the reference was embedded for %s on %s, got %s on %s"
                                % (ref.shape, ref.store.device, tuple(getattr(sr, "shape", ())), getattr(sr, "device", None)))

    def _call(self, ref: MetricRef, sr: torch.Tensor, out: torch.Tensor, image_out: Optional[torch.Tensor]):
        self._check(ref, sr)
        B, _, H, W = ref.shape
        if out.dtype != torch.float64 or tuple(out.shape) != (B, 8):
            raise _lib.HcfError("PairMetrics.compare: out must be float64 [%d,8], got %s %s" % (B, out.dtype, tuple(out.shape)))
        if image_out is not None and (image_out.dtype != torch.uint8 or tuple(image_out.shape) != (B, H, W, 3)):
            raise _lib.HcfError("PairMetrics.compare: image_out must be uint8 [%d,%d,%d,3], got %s %s"
                                % (B, H, W, image_out.dtype, tuple(image_out.shape)))
        _lib.launch("hcf_metric_pair_compare", sr.device, ref.store, ref.store.numel(), _prep(sr), B, H, W, ref.crop_border, ref.scale,
                    out, image_out, ref.work, ref.work.numel())

    def compare(self, ref: MetricRef, sr: torch.Tensor, image: bool = False, out: Optional[torch.Tensor] = None,
                image_out: Optional[torch.Tensor] = None):
        """The ``[B,8]`` float64 rows of ``sr`` against the embedded GT; with ``image=True`` (or an ``image_out``) the pair
        ``(rows, [B,H,W,3] uint8 BGR)``."""
        self._check(ref, sr)
        B, _, H, W = ref.shape
        if out is None:
            out = torch.empty(B, 8, dtype=torch.float64, device=sr.device)
        if image_out is None and image:
            image_out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=sr.device)
        self._call(ref, sr, out, image_out)
        return (out, image_out) if image_out is not None else out

    def sample_set(self, gt: torch.Tensor, crop_border: int = 0, scale: int = 0, capacity: int = 64) -> "PairSampleSet":
        return PairSampleSet(self, self.embed(gt, crop_border, scale), capacity)


class PairSampleSet:
    """The accumulator of ``PairMetrics.sample_set``: ``add`` is one ``compare`` into row M of a ``[capacity,B,8]`` device buffer
    allocated with the set (beyond ``capacity`` samples it doubles: the one allocation after the first add); nothing synchronises
    until the caller reads ``result()``: {"per_sample": [M,B,8], "mean": [B,8] (float64 mean over the samples), "best_psnr" [B],
    "best_psnr_index" [B]: the sample with the highest PSNR per image}."""

    def __init__(self, owner: PairMetrics, ref: MetricRef, capacity: int = 64):
        self.owner, self.ref, self.M = owner, ref, 0
        self._rows = torch.empty(max(1, int(capacity)), ref.shape[0], 8, dtype=torch.float64, device=ref.store.device)

    def __len__(self):
        return self.M

    def add(self, sr: torch.Tensor) -> "PairSampleSet":
        self.owner._check(self.ref, sr)                              # a refused sample does not count (and grows nothing)
        if self.M == self._rows.shape[0]:
            self._rows = torch.cat([self._rows, torch.empty_like(self._rows)], 0)
        self.owner._call(self.ref, sr, self._rows[self.M], None)
        self.M += 1
        return self

    def result(self) -> Dict[str, torch.Tensor]:
        if self.M == 0:
            raise _lib.HcfError("PairSampleSet.result: no sample was added")
        rows = self._rows[:self.M].clone()
        best, idx = rows[:, :, 0].max(dim=0)
        return {"per_sample": rows, "mean": rows.mean(dim=0), "best_psnr": best, "best_psnr_index": idx}


def _gpu_tensor(what: str, t, dtype, shape_ok, expected: str) -> torch.Tensor:
    """The argument checks of ``quantize`` / ``from_image``: a CUDA tensor of ``dtype`` whose shape ``shape_ok`` accepts, contiguous."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.HcfError("%s needs a GPU tensor (got %s); hcflow_amd has no CPU fallback"
                            % (what, t.device if torch.is_tensor(t) else type(t).__name__))
    if t.dtype != dtype or not shape_ok(t.shape) or t.numel() == 0:
        raise _lib.HcfError("%s: expected %s, got %s %s" % (what, expected, t.dtype, tuple(t.shape)))
    return t.detach().contiguous()


def _out_tensor(what: str, name: str, given: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    if given is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if not torch.is_tensor(given) or given.dtype != dtype or tuple(given.shape) != tuple(shape) or given.device != device \
            or not given.is_contiguous():
        raise _lib.HcfError("%s: %s must be a contiguous %s %s on %s, got %s %s on %s"
                            % (what, name, dtype, list(shape), device, getattr(given, "dtype", None),
                               tuple(getattr(given, "shape", ())), getattr(given, "device", None)))
    return given


def quantize(x: torch.Tensor, out: Optional[torch.Tensor] = None, image: bool = False, image_out: Optional[torch.Tensor] = None):
    """``(torch.clamp(x, 0, 1) * 255.).round() / 255.`` of a CUDA fp32 ``[B,3,H,W]`` tensor, bit for bit: the forward value of the
    reference's ``Quantization`` (Basic.py:186-202), which its rescaling test applies to LR^ before every inverse
    (HCFlow_Rescaling_model.py:306-324). With ``image=True`` (or an ``image_out``) the pair ``(q, [B,H,W,3] uint8 BGR)``: the same
    integers as the image ``util.tensor2img`` makes of ``x``, i.e. what ``PairMetrics.compare(image=True)`` stores -- the LR as it
    is written to disk; ``from_image`` is the way back. One launch writes both (include/hcflow.h: hcf_metric_quantize); ``out=`` /
    ``image_out=`` are filled in place and nothing is allocated. Not differentiable: a training step keeps its own straight-through
    ``Quantization``. No CPU fallback."""
    x = _gpu_tensor("metrics.quantize", x, torch.float32, lambda s: len(s) == 4 and s[1] == 3, "float32 [B,3,H,W]")
    B, _, H, W = x.shape
    q = _out_tensor("metrics.quantize", "out", out, (B, 3, H, W), torch.float32, x.device)
    img = None
    if image or image_out is not None:
        img = _out_tensor("metrics.quantize", "image_out", image_out, (B, H, W, 3), torch.uint8, x.device)
    _lib.launch("hcf_metric_quantize", x.device, x, B, H, W, q, img)
    return (q, img) if img is not None else q


def from_image(u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A stored image back as the tensor a net takes: CUDA uint8 ``[B,H,W,3]`` BGR (``quantize``'s image, ``util.tensor2img``'s
    layout) -> fp32 ``[B,3,H,W]`` RGB = ``u8.astype(np.float32) / 255.`` transposed, bit for bit what the reference's datasets
    produce from an image file (data/util.py:72-79). ``quantize(from_image(u8), image=True)`` returns ``(from_image(u8), u8)``
    exactly: stored images are fixed points (include/hcflow.h: hcf_metric_from_image). No CPU fallback."""
    u8 = _gpu_tensor("metrics.from_image", u8, torch.uint8, lambda s: len(s) == 4 and s[3] == 3, "uint8 [B,H,W,3]")
    B, H, W, _ = u8.shape
    o = _out_tensor("metrics.from_image", "out", out, (B, 3, H, W), torch.float32, u8.device)
    _lib.launch("hcf_metric_from_image", u8.device, u8, B, H, W, o)
    return o


def rows_to_dicts(m: torch.Tensor) -> List[Dict[str, float]]:
    """A ``[B,8]`` result of ``PairMetrics.compare`` as ``psnr_ssim``'s list of dicts (one readback)."""
    return [dict(zip(KEYS, row)) for row in m.detach().double().cpu().tolist()]
