"""MATLAB-style bicubic resize on the device, differentiable, down and up (``hcf_resize_bicubic`` / ``_backward``).

``imresize(x, scale)`` is the reference's ``utils/imresize.py::imresize`` of a float image with ``method='bicubic'`` -- the rule
every shipped configuration defines its LR image by -- for fp32 ``[B, C, H, W]`` tensors on the GPU: ``scale`` an integer 2 .. 8
(up-scaling) or the reciprocal of one (antialiased down-scaling), output ``[B, C, ceil(H * scale), ceil(W * scale)]``, nothing
clipped (up-scaling overshoots [0, 1] as the reference's float path does). Per axis it is the matrix ``A`` of ``contributions()``
(mirror padding through ``aux``, each row normalised), ``y = A_h x A_w^T``; the backward is the exact transpose
``A_h^T g A_w``. Weights are float64 on the host, rounded once to fp32; every element is one fp32 fma chain in a fixed order: a
result is bit-reproducible and does not depend on the batch around the image. ``F.interpolate(mode="bicubic", antialias=True)``
is a different function (another kernel and another border rule), not a substitute.

``metrics.imresize_down`` is the LOG-LINE form of the same rule: it quantises the image to uint8 first (tensor2img), works in
float64, handles 3-channel images and down-scaling only and returns numpy. This module is the tensor-to-tensor form: no
quantisation, fp32, any channel count, both directions, a gradient.

The device tables of a (length, factor, direction) are uploaded at their first use (one allocation, one host copy, one
synchronisation); later calls of that shape do none of these, so a graph capture needs one warm-up call of the same shape first.
"""
from __future__ import annotations

import math
from fractions import Fraction

import torch
from torch.autograd.function import once_differentiable

from . import _lib

__all__ = ["imresize", "lr_psnr", "parse_scale", "out_size"]


def parse_scale(scale):
    """``scale`` -> ``(s, up)``: an ``int`` 2 .. 8 is up-scaling by it; a float or ``Fraction`` whose reciprocal is such an integer
    within 1e-9 is down-scaling by that integer. Anything else: ``ValueError``."""
    if isinstance(scale, bool):
        raise ValueError("imresize: scale must be an int 2..8 or the reciprocal of one, got %r" % (scale,))
    if isinstance(scale, int):
        if 2 <= scale <= 8:
            return scale, 1
        raise ValueError("imresize: an integer scale (up-scaling) must be in 2..8, got %r" % (scale,))
    if isinstance(scale, (float, Fraction)):
        v = float(scale)
        if math.isfinite(v) and v > 0:
            r = 1.0 / v
            s = int(round(r))
            if 2 <= s <= 8 and abs(r - s) <= 1e-9:
                return s, 0
    raise ValueError("imresize: scale must be an int 2..8 (up) or a float / Fraction 1/2..1/8 (down), got %r" % (scale,))


def out_size(n, s, up):
    """ceil(n * scale) (utils/imresize.py: deriveSizeFromScale)."""
    return n * s if up else (n + s - 1) // s


def _checked(x, what):
    if not isinstance(x, torch.Tensor):
        raise _lib.HcfError("imresize: %s is not a tensor" % what)
    if not x.is_cuda:
        raise _lib.HcfError("imresize: %s is on %s; the op runs on the GPU only (no fallback)" % (what, x.device))
    if x.dtype != torch.float32:
        raise _lib.HcfError("imresize: %s is %s; float32 only" % (what, x.dtype))
    if x.dim() != 4 or min(x.shape) < 1:
        raise _lib.HcfError("imresize: %s must be [B, C, H, W] with every side >= 1, got %s" % (what, tuple(x.shape)))


def _work(x, B, C, H, W, s, up):
    need = int(_lib.load().hcf_resize_workspace(B, C, H, W, s, up))
    if need == 0:
        raise _lib.HcfError("imresize: shape %s at s = %d is refused by hcf_resize_workspace" % ((B, C, H, W), s))
    return torch.empty(need, dtype=torch.uint8, device=x.device), need


def _forward(x, s, up, out):
    B, C, H, W = (int(v) for v in x.shape)
    y = out if out is not None else torch.empty(B, C, out_size(H, s, up), out_size(W, s, up), dtype=torch.float32, device=x.device)
    work, need = _work(x, B, C, H, W, s, up)
    _lib.launch("hcf_resize_bicubic", x.device, x, B, C, H, W, s, up, y, work, need)
    return y


class _ImresizeFn(torch.autograd.Function):
    """``imresize`` as ONE node: the op is linear, so nothing is saved but the shape; backward is one
    ``hcf_resize_bicubic_backward`` call."""

    @staticmethod
    def forward(ctx, x, s, up, out):
        ctx.meta = (tuple(int(v) for v in x.shape), s, up)
        if out is not None:
            ctx.mark_dirty(out)
        return _forward(x, s, up, out)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (B, C, H, W), s, up = ctx.meta
        gy = gy.to(torch.float32).contiguous()
        gx = torch.empty(B, C, H, W, dtype=torch.float32, device=gy.device)
        work, need = _work(gy, B, C, H, W, s, up)
        _lib.launch("hcf_resize_bicubic_backward", gy.device, gy, B, C, H, W, s, up, gx, work, need)
        return gx, None, None, None


def imresize(x, scale, out=None):
    """``x`` [B, C, H, W] fp32 on the GPU resized by ``scale`` (module docstring). ``out``: an optional contiguous fp32 tensor of
    the output's shape on ``x``'s device to write into. ``ValueError`` for an illegal scale (before any engine call); ``HcfError``
    for a CPU tensor, another dtype or a wrong ``out`` -- there is no fallback. A non-contiguous ``x`` is made contiguous (its
    autograd link is kept). When ``x`` requires grad and grad mode is on, the result is one autograd node; otherwise no graph
    is built."""
    s, up = parse_scale(scale)
    _checked(x, "x")
    if out is not None:
        _checked(out, "out")
        want = (x.shape[0], x.shape[1], out_size(int(x.shape[2]), s, up), out_size(int(x.shape[3]), s, up))
        if tuple(out.shape) != want or out.device != x.device or not out.is_contiguous():
            raise _lib.HcfError("imresize: out must be a contiguous %s tensor on %s, got %s on %s"
                                % (want, x.device, tuple(out.shape), out.device))
    x = x.contiguous()
    if x.requires_grad and torch.is_grad_enabled():
        return _ImresizeFn.apply(x, s, up, out)
    return _forward(x.detach(), s, up, out)


def lr_psnr(sr, lq, scale):
    """[B] float64 device tensor: the LR-PSNR consistency number of the flow-SR literature,

        ``10 log10(1 / mean_{c,y,x} (imresize(sr, 1 / scale) - lq)^2)``   (peak 1, per sample),

    i.e. how well the bicubic down-scale of a super-resolved image reproduces the LR input it was sampled from. ``scale`` is the
    SR factor (an int 2 .. 8); ``inf`` for an exact match. The mean is taken in float64. Not differentiable (use
    ``latent.lr_consistency`` for a loss)."""
    if isinstance(scale, bool) or not isinstance(scale, int) or not 2 <= scale <= 8:
        raise ValueError("lr_psnr: scale is the integer SR factor 2..8, got %r" % (scale,))
    with torch.no_grad():
        low = imresize(sr, Fraction(1, scale))
        if tuple(lq.shape) != tuple(low.shape):
            raise _lib.HcfError("lr_psnr: lq is %s, imresize(sr, 1/%d) is %s" % (tuple(lq.shape), scale, tuple(low.shape)))
        mse = ((low.double() - lq.to(low.device).double()) ** 2).mean(dim=[1, 2, 3])
        return -10.0 * torch.log10(mse)
