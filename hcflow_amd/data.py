"""Device-side training batches: what the reference's GT_dataset (codes/data/GT_dataset.py) makes per sample on the CPU --
whole-image bicubic LR, random crop, flip / flip / transpose, BGR -> RGB, HWC -> CHW -- as ONE launch per batch over images that
are decoded once and kept in device memory as uint8 (hcf_data_prepare_batch, include/hcflow.h; kernel: csrc/hcf_data.hip).

    bank = ImageBank(list_of_uint8_hwc_bgr_arrays, "cuda:0")            # decode once (cv2.imread order = "bgr")
    for batch in BankLoader(bank, batch_size=16, gt_size=160, scale=4, generator=g):
        model.feed_data(batch)                                           # {'LQ', 'GT', 'LQ_path', 'GT_path'}

There is no CPU fallback: prepare_batch on a bank that is not on a GPU raises.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["ImageBank", "draw_crops", "prepare_batch", "prepare_crops", "whole_image", "BankLoader"]


class ImageBank:
    """uint8 HWC 3-channel images packed into one device tensor, each on a 16-byte boundary, plus the host table
    int64 [N, 3] = (byte offset, H, W) the kernel's launcher validates every crop against.
    order: "bgr" (cv2.imread, the reference's read_img) or "rgb" -- the batches are RGB either way."""

    def __init__(self, images: Sequence, device, order: str = "bgr", paths: Optional[Sequence[str]] = None):
        if order not in ("bgr", "rgb"):
            raise ValueError("order must be 'bgr' or 'rgb', got %r" % (order,))
        arrs = []
        for i, im in enumerate(images):
            a = im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("image %d: need uint8 [H, W, 3], got %s %s" % (i, a.dtype, tuple(a.shape)))
            arrs.append(np.ascontiguousarray(a))
        if not arrs:
            raise ValueError("an ImageBank needs at least one image")
        if paths is not None and len(paths) != len(arrs):
            raise ValueError("paths: %d entries for %d images" % (len(paths), len(arrs)))
        table = torch.zeros(len(arrs), 3, dtype=torch.int64)
        off = 0
        for i, a in enumerate(arrs):
            table[i, 0], table[i, 1], table[i, 2] = off, a.shape[0], a.shape[1]
            off = (off + a.size + 15) // 16 * 16
        host = torch.zeros(off, dtype=torch.uint8)
        for i, a in enumerate(arrs):
            o = int(table[i, 0])
            host[o:o + a.size] = torch.from_numpy(a.reshape(-1))
        self.table = table.contiguous()
        self.data = host.to(device)
        self.bgr = order == "bgr"
        self.paths = list(paths) if paths is not None else ["bank:%d" % i for i in range(len(arrs))]

    def __len__(self) -> int:
        return int(self.table.shape[0])

    @property
    def nbytes(self) -> int:
        return int(self.data.numel())

    @property
    def device(self):
        return self.data.device

    def shape(self, index: int):
        return int(self.table[index, 1]), int(self.table[index, 2])


def _lr_size(gt_size: int, scale: int) -> int:
    if not 2 <= int(scale) <= 8:
        raise ValueError("scale must be an integer in 2 .. 8, got %r" % (scale,))
    if gt_size < scale or gt_size % scale:
        raise ValueError("gt_size %d is not a positive multiple of scale %d" % (gt_size, scale))
    return gt_size // scale


def draw_crops(bank: ImageBank, indices, gt_size: int, scale: int, use_flip: bool = True, use_rot: bool = True,
               generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """CPU int32 [B, 6] = (image, top_lr, left_lr, hflip, vflip, rot90) as GT_dataset.__getitem__ and augment draw them:
    top_lr uniform in [0, H // scale - lr_size], left_lr likewise, hflip = use_flip and p < 1/2, vflip and rot90 = use_rot and
    p < 1/2 each. Deterministic under `generator`."""
    n = _lr_size(gt_size, scale)
    idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(bank)):
        raise ValueError("image index outside the bank")
    hw = bank.table[idx, 1:3] // scale - n                       # largest top / left
    if idx.numel() and int(hw.min()) < 0:
        raise ValueError("an image is smaller than the %d x %d crop" % (gt_size, gt_size))
    r = torch.rand(idx.numel(), 5, generator=generator, dtype=torch.float64)
    pos = torch.minimum((r[:, :2] * (hw + 1)).floor().to(torch.int64), hw)
    gate = torch.tensor([bool(use_flip), bool(use_rot), bool(use_rot)])
    flags = (r[:, 2:] < 0.5) & gate
    return torch.cat([idx[:, None], pos, flags.to(torch.int64)], dim=1).to(torch.int32).contiguous()


def _launch(bank: ImageBank, crops: torch.Tensor, lr_h: int, lr_w: int, scale: int, gt: torch.Tensor, lq: torch.Tensor):
    dev = bank.data.device
    if dev.type != "cuda":
        raise _lib.HcfError("hcflow_amd.data has no CPU path: the bank lives on %s" % dev)
    _lib.launch("hcf_data_prepare_batch", dev, bank.data, bank.nbytes, bank.table, len(bank), crops, int(crops.shape[0]), lr_h, lr_w,
                int(scale), int(bank.bgr), gt, lq)


def _outputs(bank, out, B, gh, gw, lh, lw) -> Dict[str, torch.Tensor]:
    shapes = {"GT": (B, 3, gh, gw), "LQ": (B, 3, lh, lw)}
    if out is None:
        return {k: torch.empty(s, dtype=torch.float32, device=bank.device) for k, s in shapes.items()}
    for k, s in shapes.items():
        t = out[k]
        if tuple(t.shape) != s or t.dtype != torch.float32 or t.device != bank.device or not t.is_contiguous():
            raise ValueError("out[%r]: need a contiguous float32 %s on %s" % (k, s, bank.device))
    return out


def _crop_table(crops) -> torch.Tensor:
    c = torch.as_tensor(crops)
    if c.device.type != "cpu" or c.dim() != 2 or c.shape[1] != 6:
        raise ValueError("crops: need a CPU [B, 6] table (draw_crops)")
    return c.to(torch.int32).contiguous()


def prepare_crops(bank: ImageBank, crops, lr_h: int, lr_w: int, scale: int, out: Optional[Dict[str, torch.Tensor]] = None):
    """prepare_batch for rectangular crops of lr_h x lr_w LR pixels (rot90 rows need lr_h == lr_w)."""
    _lr_size(scale, scale)
    c = _crop_table(crops)
    o = _outputs(bank, out, int(c.shape[0]), lr_h * scale, lr_w * scale, lr_h, lr_w)
    _launch(bank, c, int(lr_h), int(lr_w), scale, o["GT"], o["LQ"])
    return o


def prepare_batch(bank: ImageBank, crops, gt_size: int, scale: int, out: Optional[Dict[str, torch.Tensor]] = None):
    """{'GT': [B, 3, gt_size, gt_size], 'LQ': [B, 3, gt_size / scale, ...]} float32 RGB on the bank's device, enqueued on the
    current stream: no copy, no synchronisation, and with `out` (a dict of those two tensors, returned) no allocation."""
    n = _lr_size(gt_size, scale)
    return prepare_crops(bank, crops, n, n, scale, out)


def whole_image(bank: ImageBank, index: int, scale: int, out: Optional[Dict[str, torch.Tensor]] = None):
    """The validation pair of one image: {'GT': [1, 3, H, W], 'LQ': [1, 3, H / scale, W / scale]}, no crop, no augment (the same
    kernel, B = 1). H and W must be multiples of scale (the reference mod-crops its validation images beforehand)."""
    _lr_size(scale, scale)
    if not 0 <= int(index) < len(bank):
        raise ValueError("image index outside the bank")
    H, W = bank.shape(index)
    if H % scale or W % scale:
        raise ValueError("image %d is %d x %d: not a multiple of scale %d" % (index, H, W, scale))
    c = torch.tensor([[int(index), 0, 0, 0, 0, 0]], dtype=torch.int32)
    o = _outputs(bank, out, 1, H, W, H // scale, W // scale)
    _launch(bank, c, H // scale, W // scale, scale, o["GT"], o["LQ"])
    return o


class BankLoader:
    """One epoch of training batches per iteration: a random permutation of the bank's images (under `generator`), the last partial
    batch dropped, every batch {'LQ', 'GT', 'LQ_path', 'GT_path'} as the reference's models take in feed_data. reuse_out=True
    writes every batch into the same two tensors (no allocation; the consumer must be done with a batch before asking for the next)."""

    def __init__(self, bank: ImageBank, batch_size: int, gt_size: int, scale: int, use_flip: bool = True, use_rot: bool = True,
                 generator: Optional[torch.Generator] = None, reuse_out: bool = False):
        _lr_size(gt_size, scale)
        if batch_size < 1 or batch_size > len(bank):
            raise ValueError("batch_size %d for a bank of %d images" % (batch_size, len(bank)))
        self.bank, self.batch_size, self.gt_size, self.scale = bank, int(batch_size), int(gt_size), int(scale)
        self.use_flip, self.use_rot, self.generator = use_flip, use_rot, generator
        self._out = _outputs(bank, None, self.batch_size, gt_size, gt_size, gt_size // scale, gt_size // scale) if reuse_out else None

    def __len__(self) -> int:
        return len(self.bank) // self.batch_size

    def __iter__(self):
        perm = torch.randperm(len(self.bank), generator=self.generator)
        for i in range(len(self)):
            idx = perm[i * self.batch_size:(i + 1) * self.batch_size]
            crops = draw_crops(self.bank, idx, self.gt_size, self.scale, self.use_flip, self.use_rot, self.generator)
            o = prepare_batch(self.bank, crops, self.gt_size, self.scale, out=self._out)
            paths = [self.bank.paths[int(j)] for j in idx]
            yield {"LQ": o["LQ"], "GT": o["GT"], "LQ_path": paths, "GT_path": paths}
