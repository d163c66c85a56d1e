"""Device-side training batches: what the reference's GT_dataset (codes/data/GT_dataset.py) makes per sample on the CPU --
whole-image bicubic LR, random crop, flip / flip / transpose, BGR -> RGB, HWC -> CHW -- as ONE launch per batch over images that
are decoded once and kept in device memory as uint8 (hcf_data_prepare_batch, include/hcflow.h; kernel: csrc/hcf_data.hip).

    bank = ImageBank(list_of_uint8_hwc_bgr_arrays, "cuda:0")            # decode once (cv2.imread order = "bgr")
    for batch in BankLoader(bank, batch_size=16, gt_size=160, scale=4, generator=g):
        model.feed_data(batch)                                           # {'LQ', 'GT', 'LQ_path', 'GT_path'}

The paired dataset modes (LRHR_PKL_dataset.py, GTLQnpy_dataset.py, GTLQx_dataset.py), where the LQ image is stored data and not
a function of the HR image, keep two banks (hcf_data_prepare_paired):

    bank = PairedBank.from_pkl(hr_pkl, lr_pkl, "cuda:0")                 # mode: LRHR_PKL
    for batch in PairedBankLoader(bank, 16, 160, rule="pkl", use_flip=True, use_rot=True, generator=g):
        model.feed_data(batch)

There is no CPU fallback: prepare_batch on a bank that is not on a GPU raises.
"""
from __future__ import annotations

import pickle
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

__all__ = ["ImageBank", "draw_crops", "prepare_batch", "prepare_crops", "whole_image", "BankLoader",
           "PairedBank", "PKL_FLAGS", "draw_paired_crops", "center_crops", "prepare_paired_crops", "prepare_paired_batch",
           "whole_pair", "PairedBankLoader"]


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


def _bank_indices(bank, indices) -> torch.Tensor:
    idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= len(bank)):
        raise ValueError("image index outside the bank")
    return idx


def _draw(idx: torch.Tensor, hw: torch.Tensor, n: int, rule: str, use_flip, use_rot, generator) -> torch.Tensor:
    """The crop table of both banks: idx = validated image indices [B], hw = their (H, W) in LR pixels (each >= n, the caller's
    check). One torch.rand(B, 5) per call: columns 0-1 the positions, 2-4 the three coins of "augment", or 2 = f and 3 = k of "pkl"
    (draw_paired_crops states both rules)."""
    room = hw - n                                                   # largest top / left
    r = torch.rand(idx.numel(), 5, generator=generator, dtype=torch.float64)
    pos = torch.minimum((r[:, :2] * (room + 1)).floor().to(torch.int64), room)
    if rule == "augment":
        flags = ((r[:, 2:] < 0.5) & torch.tensor([bool(use_flip), bool(use_rot), bool(use_rot)])).to(torch.int64)
    else:
        f = ((r[:, 2] < 0.5) & bool(use_flip)).to(torch.int64)
        k = (r[:, 3] * 3).floor().to(torch.int64).clamp_(max=2) * int(bool(use_rot))      # 0, 1, 2 stand for k = 0, 1, 3
        table = torch.tensor([PKL_FLAGS[(fi, ki)] for ki in (0, 1, 3) for fi in (0, 1)], dtype=torch.int64)
        flags = table[k * 2 + f]
    return torch.cat([idx[:, None], pos, flags], dim=1).to(torch.int32).contiguous()


def draw_crops(bank: ImageBank, indices, gt_size: int, scale: int, use_flip: bool = True, use_rot: bool = True,
               generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """CPU int32 [B, 6] = (image, top_lr, left_lr, hflip, vflip, rot90) as GT_dataset.__getitem__ and augment draw them:
    top_lr uniform in [0, H // scale - lr_size], left_lr likewise, hflip = use_flip and p < 1/2, vflip and rot90 = use_rot and
    p < 1/2 each. Deterministic under `generator`."""
    n = _lr_size(gt_size, scale)
    idx = _bank_indices(bank, indices)
    hw = bank.table[idx, 1:3] // scale
    if idx.numel() and int(hw.min()) < n:
        raise ValueError("an image is smaller than the %d x %d crop" % (gt_size, gt_size))
    return _draw(idx, hw, n, "augment", use_flip, use_rot, generator)


def _device(bank):
    """The bank's GPU; the one place that refuses a bank that is not on one."""
    dev = bank.device
    if dev.type != "cuda":
        raise _lib.HcfError("hcflow_amd.data has no CPU path: the bank lives on %s" % dev)
    return dev


def _launch(bank: ImageBank, crops: torch.Tensor, lr_h: int, lr_w: int, scale: int, gt: torch.Tensor, lq: torch.Tensor):
    _lib.launch("hcf_data_prepare_batch", _device(bank), bank.data, bank.nbytes, bank.table, len(bank), crops, int(crops.shape[0]),
                lr_h, lr_w, int(scale), int(bank.bgr), gt, lq)


def _outputs(bank, out, B, lh, lw, scale, partial=False) -> Dict[str, Optional[torch.Tensor]]:
    """out=None: both tensors, new. Otherwise the caller's dict, checked; with `partial` (the paired calls) one of its two entries
    may be None (that half is not made)."""
    shapes = {"GT": (B, 3, lh * scale, lw * scale), "LQ": (B, 3, lh, lw)}
    if out is None:
        return {k: torch.empty(s, dtype=torch.float32, device=bank.device) for k, s in shapes.items()}
    if partial and out.get("GT") is None and out.get("LQ") is None:
        raise ValueError("out: need at least one of 'GT' and 'LQ'")
    for k, s in shapes.items():
        t = out.get(k) if partial else out[k]
        if partial and t is None:
            continue
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
    o = _outputs(bank, out, int(c.shape[0]), lr_h, lr_w, scale)
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
    o = _outputs(bank, out, 1, H // scale, W // scale, scale)
    _launch(bank, c, H // scale, W // scale, scale, o["GT"], o["LQ"])
    return o


def _epoch(loader, order, lq_paths, batch):
    """The batch loop of both loaders: slices of the epoch's index order, the last partial batch dropped; batch(idx) draws the
    crops of one slice and prepares them."""
    for i in range(len(loader)):
        idx = order[i * loader.batch_size:(i + 1) * loader.batch_size]
        o = batch(idx)
        yield {"LQ": o["LQ"], "GT": o["GT"], "LQ_path": [lq_paths[int(j)] for j in idx],
               "GT_path": [loader.bank.paths[int(j)] for j in idx]}


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
        self._out = _outputs(bank, None, self.batch_size, gt_size // scale, gt_size // scale, scale) if reuse_out else None

    def __len__(self) -> int:
        return len(self.bank) // self.batch_size

    def __iter__(self):
        perm = torch.randperm(len(self.bank), generator=self.generator)         # from the same generator, before the crops
        yield from _epoch(self, perm, self.bank.paths, lambda idx: prepare_batch(
            self.bank, draw_crops(self.bank, idx, self.gt_size, self.scale, self.use_flip, self.use_rot, self.generator),
            self.gt_size, self.scale, out=self._out))


# ---- paired banks: LRHR_PKL and GTLQ / GTLQnpy / GTLQx, the LQ image is data ----

# LRHR_PKL_dataset.py:146-157 on CHW arrays: np.flip(axis=2) when f, then np.rot90(k, axes=(1, 2)), k in {0, 1, 3}, as the
# kernel's (hflip, vflip, rot90) = [:, ::-1], [::-1], transpose applied in that order (tests/paired_data_oracle.py checks all six)
PKL_FLAGS = {(0, 0): (0, 0, 0), (1, 0): (1, 0, 0), (0, 1): (1, 0, 1), (1, 1): (0, 0, 1), (0, 3): (0, 1, 1), (1, 3): (1, 1, 1)}


class PairedBank:
    """HR / LQ pairs of uint8 HWC 3-channel images as two packings like ImageBank's (16-byte alignment), pair i = row i of both
    host tables. scale = H_gt // H_lq of the first pair, as the reference infers it; every pair must have H_gt >= scale * H_lq and
    W_gt >= scale * W_lq (ValueError naming the pair): a larger HR image is the reference's validation mod-crop, its extra rows and
    columns are never read. order: "bgr" (cv2 / npy files) or "rgb" (the PKL lists) -- the batches are RGB either way.
    paths: one entry per pair, a string (both images) or (GT path, LQ path); default str(i), the PKL dataset's."""

    def __init__(self, gt_images: Sequence, lq_images: Sequence, device, order: str = "bgr", paths: Optional[Sequence] = None):
        gt_images, lq_images = list(gt_images), list(lq_images)
        if len(gt_images) != len(lq_images):
            raise ValueError("GT and LQ have different numbers of images: %d, %d" % (len(gt_images), len(lq_images)))
        if paths is not None and len(paths) != len(gt_images):
            raise ValueError("paths: %d entries for %d pairs" % (len(paths), len(gt_images)))
        self.gt = ImageBank(gt_images, "cpu", order)
        self.lq = ImageBank(lq_images, "cpu", order)
        scale = int(self.gt.table[0, 1]) // int(self.lq.table[0, 1])
        if not 2 <= scale <= 8:
            raise ValueError("pair 0: HR %s over LQ %s is scale %d, need 2 .. 8" % (self.gt.shape(0), self.lq.shape(0), scale))
        for i in range(len(self.gt)):
            (gh, gw), (lh, lw) = self.gt.shape(i), self.lq.shape(i)
            if gh < scale * lh or gw < scale * lw:
                raise ValueError("pair %d: HR %d x %d is smaller than %d times LQ %d x %d" % (i, gh, gw, scale, lh, lw))
        self.scale = scale
        self.gt.data, self.lq.data = self.gt.data.to(device), self.lq.data.to(device)
        self.bgr = order == "bgr"
        pairs = [(str(i), str(i)) for i in range(len(self.gt))] if paths is None else \
            [(p, p) if isinstance(p, str) else tuple(p) for p in paths]
        self.paths, self.lq_paths = [p[0] for p in pairs], [p[1] for p in pairs]

    @classmethod
    def from_pkl(cls, gt_path: str, lq_path: str, device, n_max: Optional[int] = None):
        """The reference's LRHR_PKL files: each a pickled list of HWC uint8 RGB arrays (load_pkls, before its transpose)."""
        lists = []
        for path in (gt_path, lq_path):
            with open(path, "rb") as f:
                images = pickle.load(f)
            if not isinstance(images, (list, tuple)) or len(images) == 0:
                raise ValueError("%s: need a pickled non-empty list of images" % path)
            lists.append(list(images)[:n_max])
        return cls(lists[0], lists[1], device, order="rgb")

    def __len__(self) -> int:
        return len(self.lq)

    @property
    def nbytes(self) -> int:
        return self.gt.nbytes + self.lq.nbytes

    @property
    def device(self):
        return self.lq.data.device

    def shape(self, index: int):
        """(H, W) of LQ image `index`: crops are drawn on its grid."""
        return self.lq.shape(index)


def draw_paired_crops(bank: PairedBank, indices, gt_size: int, rule: str, use_flip: bool = True, use_rot: bool = True,
                      generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """CPU int32 [B, 6] = (image, top_lr, left_lr, hflip, vflip, rot90): top_lr uniform in [0, H_lq - n], left_lr likewise,
    n = gt_size / scale (LRHR_PKL_dataset.py:160-177, GTLQnpy_dataset.py:52-59), and the flags by
      rule="augment"  data/util.py:116-120: hflip = use_flip and p < 1/2, vflip and rot90 = use_rot and p < 1/2 each;
      rule="pkl"      LRHR_PKL_dataset.py:146-157: f = use_flip and p < 1/2, k uniform in {0, 1, 3} when use_rot, through PKL_FLAGS.
    Deterministic under `generator`. An LQ image smaller than the crop raises ValueError: the reference would return a short patch
    there (its slices stop at the image border), which no batch can hold."""
    if rule not in ("augment", "pkl"):
        raise ValueError("rule must be 'augment' or 'pkl', got %r" % (rule,))
    n = _lr_size(gt_size, bank.scale)
    idx = _bank_indices(bank, indices)
    hw = bank.lq.table[idx, 1:3]
    if idx.numel() and int(hw.min()) < n:
        raise ValueError("an LQ image is smaller than the %d x %d crop" % (n, n))
    return _draw(idx, hw, n, rule, use_flip, use_rot, generator)


def center_crops(bank: PairedBank, indices, hr_size: int) -> torch.Tensor:
    """Crop rows of the PKL mode's validation option center_crop_hr_size (LRHR_PKL_dataset.py:108-109, 180-185): a border of
    (H - size) / 2 on all sides of both images, no augment; feed them to prepare_paired_batch(bank, rows, hr_size). The
    reference's asserts (square images, an even border) raise ValueError, and so does an HR image that is not exactly scale times
    its LQ image, whose two borders would not be the same window. A border of 0 gives the whole pair."""
    s = bank.scale
    n = _lr_size(hr_size, s)
    idx = _bank_indices(bank, indices)
    rows = []
    for i in idx.tolist():
        (gh, gw), (lh, lw) = bank.gt.shape(i), bank.lq.shape(i)
        if gh != gw or lh != lw:
            raise ValueError("pair %d: center crop needs square images, got HR %d x %d, LQ %d x %d" % (i, gh, gw, lh, lw))
        if gh != s * lh:
            raise ValueError("pair %d: HR %d is not %d times LQ %d" % (i, gh, s, lh))
        if lh < n or (lh - n) % 2 or (gh - hr_size) % 2:
            raise ValueError("pair %d: no even border around %d of %d (LQ %d of %d)" % (i, hr_size, gh, n, lh))
        rows.append([i, (lh - n) // 2, (lh - n) // 2, 0, 0, 0])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 6)


def prepare_paired_crops(bank: PairedBank, crops, lr_h: int, lr_w: int, out: Optional[Dict[str, torch.Tensor]] = None):
    """prepare_paired_batch for rectangular crops of lr_h x lr_w LQ pixels (rot90 rows need lr_h == lr_w)."""
    c = _crop_table(crops)
    o = _outputs(bank, out, int(c.shape[0]), int(lr_h), int(lr_w), bank.scale, partial=True)
    _lib.launch("hcf_data_prepare_paired", _device(bank), bank.gt.data, bank.gt.nbytes, bank.gt.table, bank.lq.data, bank.lq.nbytes,
                bank.lq.table, len(bank), c, int(c.shape[0]), int(lr_h), int(lr_w), bank.scale, int(bank.bgr), o.get("GT"),
                o.get("LQ"))
    return o


def prepare_paired_batch(bank: PairedBank, crops, gt_size: int, out: Optional[Dict[str, torch.Tensor]] = None):
    """{'GT': [B, 3, gt_size, gt_size], 'LQ': [B, 3, gt_size / scale, ...]} float32 RGB on the bank's device: the stored windows
    as uint8 / 255, augmented, enqueued on the current stream: no copy, no synchronisation, and with `out` (a dict of those two
    tensors, returned; one may be None and is then not made) no allocation."""
    n = _lr_size(gt_size, bank.scale)
    return prepare_paired_crops(bank, crops, n, n, out)


def whole_pair(bank: PairedBank, index: int, out: Optional[Dict[str, torch.Tensor]] = None):
    """The validation pair of the GTLQ modes: {'GT': [1, 3, H_lq * scale, W_lq * scale], 'LQ': [1, 3, H_lq, W_lq]}, no crop, no
    augment, GT mod-cropped to scale times the LQ size (GTLQx_dataset.py:118-120). The same kernel, B = 1."""
    if not 0 <= int(index) < len(bank):
        raise ValueError("image index outside the bank")
    H, W = bank.shape(index)
    return prepare_paired_crops(bank, torch.tensor([[int(index), 0, 0, 0, 0, 0]], dtype=torch.int32), H, W, out)


class PairedBankLoader:
    """One epoch of a rank's training batches per iteration, every batch {'LQ', 'GT', 'LQ_path', 'GT_path'} as feed_data takes.
    The epoch's permutation of the bank comes from torch.Generator().manual_seed(seed + epoch) and is common to all ranks; rank r
    takes perm[r::world] cut to len(bank) // world (the idea of the reference's DistIterSampler, data_sampler.py:46-59, without its
    `ratio` enlargement), the last partial batch dropped. set_epoch(e) before each epoch, as with a DistributedSampler. The crops
    come from `generator`, which is the rank's own. reuse_out=True writes every batch into the same two tensors (no allocation;
    the consumer must be done with a batch before asking for the next)."""

    def __init__(self, bank: PairedBank, batch_size: int, gt_size: int, rule: str, use_flip: bool = True, use_rot: bool = True,
                 generator: Optional[torch.Generator] = None, reuse_out: bool = False, rank: int = 0, world: int = 1, seed: int = 0):
        n = _lr_size(gt_size, bank.scale)
        if rule not in ("augment", "pkl"):
            raise ValueError("rule must be 'augment' or 'pkl', got %r" % (rule,))
        if world < 1 or not 0 <= rank < world:
            raise ValueError("rank %d of world %d" % (rank, world))
        if batch_size < 1 or batch_size > len(bank) // world:
            raise ValueError("batch_size %d for %d images per rank" % (batch_size, len(bank) // world))
        self.bank, self.batch_size, self.gt_size, self.rule = bank, int(batch_size), int(gt_size), rule
        self.use_flip, self.use_rot, self.generator = use_flip, use_rot, generator
        self.rank, self.world, self.seed, self.epoch = int(rank), int(world), int(seed), 0
        self._out = _outputs(bank, None, self.batch_size, n, n, bank.scale) if reuse_out else None

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)

    def shard(self) -> torch.Tensor:
        """This rank's image indices of the current epoch, in order."""
        perm = torch.randperm(len(self.bank), generator=torch.Generator().manual_seed(self.seed + self.epoch))
        return perm[self.rank::self.world][:len(self.bank) // self.world]

    def __len__(self) -> int:
        return len(self.bank) // self.world // self.batch_size

    def __iter__(self):
        yield from _epoch(self, self.shard(), self.bank.lq_paths, lambda idx: prepare_paired_batch(
            self.bank, draw_paired_crops(self.bank, idx, self.gt_size, self.rule, self.use_flip, self.use_rot, self.generator),
            self.gt_size, out=self._out))
