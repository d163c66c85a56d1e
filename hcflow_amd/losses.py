"""The training criteria of the reference's callers on the device (``hcf_loss.hip``; ``include/hcflow.h`` has the contract).

``models/modules/loss.py`` and the expressions around it in ``HCFlow_SR_model.py:207-287`` / ``HCFlow_Rescaling_model.py:214-232``
are strings of small torch ops with host synchronisations in between (``torch.isnan(fake_H).any()``, ``torch.isfinite(l)``,
``.item()``). Here every criterion a shipped training yml selects is ONE autograd node on the project's kernels:

* the terms are evaluated in fp64 from the fp32 inputs and summed in fp64 in a fixed order, rounded to fp32 once: a value is
  bit-reproducible and does not depend on the alignment of its inputs; row ``b`` of a per-sample result does not depend on the
  batch around it;
* a node saves nothing but its inputs: the backward recomputes, one launch;
* nothing synchronises with the host: the upstream gradient is read on the device, and a sum over every element is non-finite as
  soon as one element is, so ``finite_sum`` replaces the callers' ``isnan`` / ``isfinite`` gates without a pass of its own.

GPU and fp32 only; anything else raises ``HcfError`` -- there is no fallback. A non-contiguous input is made contiguous (its
autograd link is kept); when nothing requires grad no graph is built. ``ssim`` / ``SSIMLoss`` (``hcf_ssim.hip``) add the
structural measure the validation log reports (``utils/util.py:914-955``) under the same rules. ``GradientPenaltyLoss`` (``loss.py:54-74``) needs a double
backward through the discriminator, no shipped yml uses it: it stays the reference's.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import metrics

__all__ = ["PixelLoss", "ReconstructionLoss", "CharbonnierLoss", "GANLoss", "Quantization", "latent_l2", "finite_sum", "ssim",
           "SSIMLoss"]

_L1, _L2, _CHARB = 0, 1, 2
_MAX_TENSORS = 8
_WORK = {}


def _workspace(tag, device, need):
    """The scratch buffer of criterion `tag` on (device, current stream), as gan._workspace: calls on a stream run in order and a
    buffer holds state of the call in flight only."""
    key = (tag, device.index, _lib.current_stream(device))
    wk = _WORK.get(key)
    if wk is None or wk.numel() < need:
        wk = torch.empty(max(int(need), 4096), dtype=torch.uint8, device=device)
        _WORK[key] = wk
    return wk


def _typed(name, x, what):
    if not isinstance(x, torch.Tensor):
        raise _lib.HcfError("%s: %s is not a tensor" % (name, what))
    if x.dtype != torch.float32:
        raise _lib.HcfError("%s: %s is %s; float32 only" % (name, what, x.dtype))
    if x.numel() < 1:
        raise _lib.HcfError("%s: %s is empty" % (name, what))


def _on_gpu(name, x, what):
    if not x.is_cuda:
        raise _lib.HcfError("%s: %s is on %s; the criterion runs on the GPU only (no fallback)" % (name, what, x.device))
    return x.contiguous()


def _checked(name, x, what):
    _typed(name, x, what)
    return _on_gpu(name, x, what)


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---- pair criterion -------------------------------------------------------------------------------------------------------------

def _pair_forward(x, y, B, n, kind, eps, scale, row_scale, rows):
    dev = x.device
    need = int(_lib.load().hcf_loss_pair_workspace(B, n))
    if need == 0:
        raise _lib.HcfError("pair criterion: shape [%d, %d] is refused by hcf_loss_pair_workspace" % (B, n))
    wk = _workspace("pair", dev, need)
    out = torch.empty((B,) if rows else (), dtype=torch.float32, device=dev)
    _lib.launch("hcf_loss_pair", dev, x, y, B, n, kind, float(eps), float(scale), float(row_scale), None if rows else out,
                out if rows else None, wk, wk.numel())
    return out


class _PairFn(torch.autograd.Function):
    """One node: the inputs are saved, nothing else; backward is one hcf_loss_pair_backward launch for both gradients."""

    @staticmethod
    def forward(ctx, x, y, B, n, kind, eps, scale, row_scale, rows):
        ctx.save_for_backward(x, y)
        ctx.meta = (B, n, kind, eps, row_scale if rows else scale, 1 if rows else 0)
        return _pair_forward(x, y, B, n, kind, eps, scale, row_scale, rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B, n, kind, eps, scale, g_stride = ctx.meta
        g = g.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        _lib.launch("hcf_loss_pair_backward", x.device, x, y, B, n, kind, float(eps), float(scale), g, g_stride, gx, gy)
        return (gx, gy) + (None,) * 7


def _pair(name, x, y, kind, eps, mode):
    """mode 'sum' / 'mean' / 'batchmean': fp32(scale * sum over every element), scale = 1, 1 / numel, 1 / B;
    'rowsum' / 'rowmean': [B], fp32(row_scale * sum of row b), row_scale = 1, 1 / n."""
    _typed(name, x, "input")
    _typed(name, y, "target")
    if x.shape != y.shape:
        raise _lib.HcfError("%s: input is %s, target is %s" % (name, tuple(x.shape), tuple(y.shape)))
    x, y = _on_gpu(name, x, "input"), _on_gpu(name, y, "target")
    if x.device != y.device:
        raise _lib.HcfError("%s: input is on %s, target on %s" % (name, x.device, y.device))
    rows = mode in ("rowsum", "rowmean")
    if x.dim() < 1 or (rows and x.dim() < 2):
        raise _lib.HcfError("%s: the input must be [B, ...], got %s" % (name, tuple(x.shape)))
    B = int(x.shape[0]) if rows else 1              # a scalar is one flat sum: the grid follows the element count alone
    n = x.numel() // B
    s = {"sum": 1.0, "mean": 1.0 / x.numel(), "batchmean": 1.0 / int(x.shape[0]), "rowsum": 1.0, "rowmean": 1.0 / n}[mode]
    args = (B, n, kind, eps, 0.0 if rows else s, s if rows else 0.0, rows)
    if _wants_grad(x, y):
        return _PairFn.apply(x, y, *args)
    return _pair_forward(x.detach(), y.detach(), *args)


class PixelLoss(nn.Module):
    """``nn.L1Loss()`` / ``nn.MSELoss()`` (criterion 'l1' / 'l2'), the ``cri_pix_hr`` of ``HCFlow_SR_model.py:47-52``. reduction
    'mean' (the reference's), 'sum', or 'none': the per-sample means ``[B]``."""

    def __init__(self, criterion="l1", reduction="mean"):
        super().__init__()
        if criterion not in ("l1", "l2"):
            raise NotImplementedError("Loss type [{}] is not recognized.".format(criterion))
        if reduction not in ("mean", "sum", "none"):
            raise ValueError("PixelLoss: reduction is 'mean', 'sum' or 'none', got %r" % (reduction,))
        self.criterion, self.reduction = criterion, reduction

    def forward(self, input, target):
        kind = _L1 if self.criterion == "l1" else _L2
        return _pair("PixelLoss", input, target, kind, 0.0, "rowmean" if self.reduction == "none" else self.reduction)


class ReconstructionLoss(nn.Module):
    """The reference's class (``loss.py:76-90``): 'l2' ``mean_b sum_chw (x - t)^2``, 'l1' ``mean_b sum_chw sqrt((x - t)^2 + eps)``.
    reduction 'none': the per-sample sums ``[B]``."""

    def __init__(self, losstype="l2", eps=1e-6, reduction="mean"):
        super().__init__()
        if losstype not in ("l2", "l1"):
            raise ValueError("ReconstructionLoss: losstype is 'l2' or 'l1', got %r" % (losstype,))
        if reduction not in ("mean", "none"):
            raise ValueError("ReconstructionLoss: reduction is 'mean' or 'none', got %r" % (reduction,))
        self.losstype, self.eps, self.reduction = losstype, float(eps), reduction

    def forward(self, x, target):
        kind, eps = (_L2, 0.0) if self.losstype == "l2" else (_CHARB, self.eps)
        return _pair("ReconstructionLoss", x, target, kind, eps, "rowsum" if self.reduction == "none" else "batchmean")


class CharbonnierLoss(nn.Module):
    """``torch.sum(torch.sqrt(diff * diff + eps))`` (``loss.py:5-15``)."""

    def __init__(self, eps=1e-6):
        super().__init__()
        self.eps = float(eps)

    def forward(self, x, y):
        return _pair("CharbonnierLoss", x, y, _CHARB, self.eps, "sum")


# ---- mean square of several tensors ----------------------------------------------------------------------------------------------

def _tables(tensors, grads=None):
    k = len(tensors)
    z = (C.c_void_p * _MAX_TENSORS)(*[t.data_ptr() for t in tensors])
    ln = (C.c_int64 * _MAX_TENSORS)(*[t.numel() for t in tensors])
    gz = None
    if grads is not None:
        gz = (C.c_void_p * _MAX_TENSORS)(*[None if g is None else g.data_ptr() for g in grads])
    return z, ln, k, gz


def _sumsq_forward(tensors):
    dev = tensors[0].device
    z, ln, k, _ = _tables(tensors)
    need = int(_lib.load().hcf_loss_sumsq_workspace(ln, k))
    if need == 0:
        raise _lib.HcfError("latent_l2: the tensor lengths are refused by hcf_loss_sumsq_workspace")
    wk = _workspace("sumsq", dev, need)
    out = torch.empty((), dtype=torch.float32, device=dev)
    _lib.launch("hcf_loss_sumsq", dev, z, ln, k, out, wk, wk.numel())
    return out


class _SumsqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *tensors):
        ctx.save_for_backward(*tensors)
        return _sumsq_forward(tensors)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        tensors = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) if need else None for t, need in zip(tensors, ctx.needs_input_grad)]
        z, ln, k, gz = _tables(tensors, grads)
        _lib.launch("hcf_loss_sumsq_backward", tensors[0].device, z, ln, k, g, gz)
        return tuple(grads)


def latent_l2(*tensors):
    """``(torch.cat([t.flatten() for t in tensors]) ** 2).mean()`` (``HCFlow_Rescaling_model.py:216``: the rescaling net's z1, z2)
    of 1 .. 8 tensors of any shapes, without the concatenation: one node, two launches forward, one backward."""
    if not 1 <= len(tensors) <= _MAX_TENSORS:
        raise _lib.HcfError("latent_l2: 1 .. %d tensors, got %d" % (_MAX_TENSORS, len(tensors)))
    ts = [_checked("latent_l2", t, "tensor %d" % i) for i, t in enumerate(tensors)]
    if any(t.device != ts[0].device for t in ts):
        raise _lib.HcfError("latent_l2: the tensors are on different devices")
    if _wants_grad(*ts):
        return _SumsqFn.apply(*ts)
    return _sumsq_forward([t.detach() for t in ts])


# ---- GAN criteria ----------------------------------------------------------------------------------------------------------------

_GAN_TYPES = {"gan": 0, "ragan": 0, "lsgan": 1, "wgan-gp": 2}
_GAN_MAX = 1 << 20


def _gan_forward(a, b, ta, tb, typ, rel, halve):
    out = torch.empty(5, dtype=torch.float32, device=a.device)
    _lib.launch("hcf_loss_gan", a.device, a, a.numel(), float(ta), b, 0 if b is None else b.numel(), float(tb), typ, rel, halve, out)
    return out


class _GanFn(torch.autograd.Function):
    """(total, logs): logs = [term_a, term_b, total, mean(a), mean(b)] is not differentiable, total is logs[2]."""

    @staticmethod
    def forward(ctx, a, b, ta, tb, typ, rel, halve):
        ctx.save_for_backward(a, b)
        ctx.meta = (ta, tb, typ, rel, halve)
        logs = _gan_forward(a, b, ta, tb, typ, rel, halve)
        ctx.mark_non_differentiable(logs)
        return logs[2], logs

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _glogs):
        a, b = ctx.saved_tensors
        ta, tb, typ, rel, halve = ctx.meta
        g = g.to(torch.float32).contiguous()
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if b is not None and ctx.needs_input_grad[1] else None
        _lib.launch("hcf_loss_gan_backward", a.device, a, a.numel(), float(ta), b, 0 if b is None else b.numel(), float(tb), typ, rel,
                    halve, g, ga, gb)
        return (ga, gb) + (None,) * 5


def _gan(a, b, ta, tb, typ, rel, halve):
    a = _checked("GANLoss", a, "the logits")
    if b is not None:
        b = _checked("GANLoss", b, "the second logits")
        if b.device != a.device:
            raise _lib.HcfError("GANLoss: the logits are on %s and %s" % (a.device, b.device))
    if a.numel() > _GAN_MAX or (b is not None and b.numel() > _GAN_MAX):
        raise _lib.HcfError("GANLoss: more than 2^20 logits (discriminator outputs are [B,1] or [B,1,h,w])")
    if _wants_grad(a, b):
        return _GanFn.apply(a, b, ta, tb, typ, rel, halve)
    logs = _gan_forward(a.detach(), None if b is None else b.detach(), ta, tb, typ, rel, halve)
    return logs[2], logs


class GANLoss(nn.Module):
    """The reference's ``GANLoss`` (``loss.py:19-51``), same constructor and ``forward(input, target_is_real)``, plus the two
    sequences its caller builds from it, each as one node (one launch forward, one backward):

    * ``generator_loss(pred_fake, pred_real=None)``: ``HCFlow_SR_model.py:242-247`` -- ``cri(pred_fake, True)``, or for 'ragan'
      ``(cri(pred_real - mean(pred_fake), False) + cri(pred_fake - mean(pred_real), True)) / 2`` with ``pred_real`` detached;
    * ``discriminator_loss(pred_real, pred_fake)``: ``:271-278`` -- returns ``(total, logs)``, ``logs`` a detached ``[5]`` device
      tensor of ``l_d_real, l_d_fake, l_d_total, D_real, D_fake`` (one ``.tolist()`` instead of four ``.item()``).
    """

    def __init__(self, gan_type, real_label_val=1.0, fake_label_val=0.0):
        super().__init__()
        self.gan_type = gan_type.lower()
        self.real_label_val = real_label_val
        self.fake_label_val = fake_label_val
        if self.gan_type not in _GAN_TYPES:
            raise NotImplementedError('GAN type [{:s}] is not found'.format(self.gan_type))
        self._type = _GAN_TYPES[self.gan_type]

    def _target(self, target_is_real):
        if self._type == 2:                      # wgan_loss takes the boolean itself
            return 1.0 if target_is_real else 0.0
        return float(self.real_label_val if target_is_real else self.fake_label_val)

    def forward(self, input, target_is_real):
        return _gan(input, None, self._target(bool(target_is_real)), 0.0, self._type, 0, 0)[0]

    def generator_loss(self, pred_fake, pred_real=None):
        if self.gan_type != "ragan":
            return self.forward(pred_fake, True)
        if pred_real is None:
            raise _lib.HcfError("GANLoss('ragan').generator_loss needs pred_real")
        return _gan(pred_real.detach() if isinstance(pred_real, torch.Tensor) else pred_real, pred_fake, self._target(False),
                    self._target(True), self._type, 1, 1)[0]

    def discriminator_loss(self, pred_real, pred_fake):
        rel = 1 if self.gan_type == "ragan" else 0
        total, logs = _gan(pred_real, pred_fake, self._target(True), self._target(False), self._type, rel, rel)
        return total, logs.detach()


# ---- SSIM ------------------------------------------------------------------------------------------------------------------------

def _ssim_args(name, x, y, y_channel, data_range):
    """The checked, contiguous pair and (B, C, H, W, y_channel, data_range). What the kernels would refuse as a status code
    (a side under 11, y_channel without three channels) is worded here, before any launch."""
    _typed(name, x, "input")
    _typed(name, y, "target")
    if x.shape != y.shape:
        raise _lib.HcfError("%s: input is %s, target is %s" % (name, tuple(x.shape), tuple(y.shape)))
    if x.dim() != 4:
        raise ValueError("%s: the inputs must be [B, C, H, W], got %s" % (name, tuple(x.shape)))
    B, Cn, H, W = (int(s) for s in x.shape)
    if H < 11 or W < 11:
        raise ValueError("%s: the 11 x 11 window does not fit into %d x %d images" % (name, H, W))
    if y_channel and Cn != 3:
        raise ValueError("%s: y_channel needs RGB inputs [B, 3, H, W], got %d channels" % (name, Cn))
    data_range = float(data_range)
    if not 0.0 < data_range < float("inf"):
        raise ValueError("%s: data_range must be positive and finite, got %r" % (name, data_range))
    x, y = _on_gpu(name, x, "input"), _on_gpu(name, y, "target")
    if x.device != y.device:
        raise _lib.HcfError("%s: input is on %s, target on %s" % (name, x.device, y.device))
    return x, y, (B, Cn, H, W, 1 if y_channel else 0, data_range)


def _ssim_forward(x, y, meta, loss):
    """(rows [B], 1 - mean or None): two launches."""
    dev = x.device
    B, Cn, H, W, ych, R = meta
    need = int(_lib.load().hcf_loss_ssim_workspace(B, Cn, H, W, ych))
    if need == 0:
        raise _lib.HcfError("ssim: shape %s is refused by hcf_loss_ssim_workspace" % (tuple(x.shape),))
    wk = _workspace("ssim", dev, need)
    rows = torch.empty(B, dtype=torch.float32, device=dev)
    out = torch.empty((), dtype=torch.float32, device=dev) if loss else None
    _lib.launch("hcf_loss_ssim", dev, x, y, B, Cn, H, W, ych, R, rows, out, wk, wk.numel())
    return rows, out


class _SsimFn(torch.autograd.Function):
    """One node: the inputs are saved, nothing else; backward is one hcf_loss_ssim_backward launch for both gradients. `loss`:
    the output is the scalar 1 - mean_b (upstream: one scalar), else the rows [B] (upstream: one value per sample)."""

    @staticmethod
    def forward(ctx, x, y, meta, loss):
        ctx.save_for_backward(x, y)
        ctx.meta, ctx.loss = meta, loss
        rows, out = _ssim_forward(x, y, meta, loss)
        return out if loss else rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        B, Cn, H, W, ych, R = ctx.meta
        g = g.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        _lib.launch("hcf_loss_ssim_backward", x.device, x, y, B, Cn, H, W, ych, R, g, 0 if ctx.loss else 1,
                    -1.0 / B if ctx.loss else 1.0, gx, gy)
        return gx, gy, None, None


def _ssim(name, x, y, y_channel, data_range, loss):
    x, y, meta = _ssim_args(name, x, y, y_channel, data_range)
    if _wants_grad(x, y):
        return _SsimFn.apply(x, y, meta, loss)
    rows, out = _ssim_forward(x.detach(), y.detach(), meta, loss)
    return out if loss else rows


def ssim(x, y, y_channel=False, data_range=1.0):
    """The reference's SSIM (``utils/util.py:914-955``: 11 x 11 Gaussian window, sigma 1.5, "valid" map, mean over the channels
    of the map means) of fp32 ``[B, C, H, W]`` tensors in ``[0, data_range]``, per sample: ``[B]``, differentiable with respect to
    either input or both. On ``[0, 1]`` data with ``data_range=1`` it is the reference's number on the same data times 255.
    ``y_channel=True`` (RGB, C = 3): on ``Y = (65.481 R + 128.553 G + 24.966 B + 16 data_range) / 255`` (``bgr2ycbcr(only_y=True)``),
    the SSIM_Y the rescaling nets are ranked by. Unlike ``PairMetrics`` nothing is quantised and nothing is cropped: slice the
    inputs for a ``crop_border``. Images under 11 pixels a side and ``y_channel`` without three channels raise ``ValueError``."""
    return _ssim("ssim", x, y, y_channel, data_range, False)


class SSIMLoss(nn.Module):
    """``1 - ssim(x, y, y_channel, data_range).mean()`` as one node (two launches forward, one backward): a structural term for
    the places that take a loss -- ``latent.refine_image(data_loss=...)``, ``latent.optimise(loss_fn=...)``, the HR term of the
    HCFlow+ reverse step and of the rescaling objective. Identical inputs give exactly 0."""

    def __init__(self, y_channel=False, data_range=1.0):
        super().__init__()
        data_range = float(data_range)
        if not 0.0 < data_range < float("inf"):
            raise ValueError("SSIMLoss: data_range must be positive and finite, got %r" % (data_range,))
        self.y_channel, self.data_range = bool(y_channel), data_range

    def forward(self, x, y):
        return _ssim("SSIMLoss", x, y, self.y_channel, self.data_range, True)


# ---- straight-through quantisation and the finite gate ---------------------------------------------------------------------------

class _QuantFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return metrics.quantize(x)

    @staticmethod
    def backward(ctx, g):
        return g


class Quantization(nn.Module):
    """``Basic.py:186-202``: ``(clamp(x, 0, 1) * 255).round() / 255`` forward (``metrics.quantize``, bit for bit), the identity
    backward -- the step between the two passes of ``HCFlow_Rescaling_model.py:218``."""

    def forward(self, x):
        x = _checked("Quantization", x, "input")
        if _wants_grad(x):
            return _QuantFn.apply(x)
        return metrics.quantize(x.detach())


def finite_sum(*terms):
    """``(total, values)``: ``total`` = the sum of the FINITE terms (scalars on one device), ``values`` = the detached stack of all of
    them for one readback. The callers' gates -- ``if torch.isfinite(l): total += l`` (``HCFlow_Rescaling_model.py:222-228``),
    ``if not torch.isnan(l)`` (``HCFlow_SR_model.py:251,285``) and, since one NaN in ``fake_H`` makes its pixel loss NaN, the
    ``torch.isnan(fake_H).any()`` pass of ``:210`` -- without their host synchronisations: plain torch ops on the device. A dropped
    term receives the upstream gradient 0, which the criteria's backward turns into exact zeros for its inputs."""
    if not terms:
        raise _lib.HcfError("finite_sum: no terms")
    for i, t in enumerate(terms):
        if not isinstance(t, torch.Tensor) or t.numel() != 1:
            raise _lib.HcfError("finite_sum: term %d is not a one-element tensor" % i)
    vals = torch.stack([t.reshape(()) for t in terms])
    keep = torch.isfinite(vals.detach())
    total = torch.where(keep, vals, torch.zeros_like(vals)).sum()
    return total, vals.detach()
