"""The auxiliary nets of the HCFlow+ / HCFlow++ recipes on the MI355X conv kernels.

``HCFlow_SR_model.py:75-95`` builds, beside netG, a VGG19 feature extractor (``networks.define_F`` -> ``VGGFeatureExtractor``,
``discriminator_vgg_arch.py:110-137``) for the perceptual loss and a ``Discriminator_VGG_160`` (``:68-107``; ``networks.define_D``
also builds ``Discriminator_VGG_128`` and ``PatchGANDiscriminator``, ``networks.py:44-56``) trained with the
reference's own ``GANLoss`` (``loss.py:19-51``: stock PyTorch criteria -- it stays the reference's file; the same criteria as one
node each on the device are ``hcflow_amd.losses``); ``optimize_parameters`` (``HCFlow_SR_model.py:219-285``) runs them forward and backward every
step on ``fake_H`` / ``real_H`` batches. The classes here keep the reference's constructor signatures, ``state_dict`` keys /
shapes (the parameter holders ARE ``nn.Conv2d`` / ``nn.BatchNorm2d`` / ``nn.Linear`` modules, so checkpoints of the reference
load strictly, ``load_network(..., netD)``) and call surface, and run EVERY CONVOLUTION -- > 99 % of their FLOPs -- through the
flow's own kernels on device tensors (``hcf_aux_conv2d`` / ``hcf_aux_conv2d_backward`` in ``include/hcflow.h``: fp32-MFMA or
f16x3 / Winograd forward, fp32-MFMA data gradient, fixed-order weight gradient):

* activations travel as NHWC fp32 (the engine's layout), 3-channel inputs padded to 4;
* the discriminator's 4x4 stride-2 convs are a ``squeeze2d`` (space-to-depth) followed by a 3x3 conv on 4C channels whose
  weight is the 4x4 kernel re-indexed (``_w4s2_as_3x3``; exact, differentiable);
* bias + LeakyReLU / ReLU are fused into the conv epilogue where no BatchNorm sits in between;
* ``Discriminator_VGG_128`` and ``PatchGANDiscriminator`` (``:6-65``, ``:159-189``) run every BatchNorm + LeakyReLU through the
  fused NHWC kernels ``hcf_aux_bn_act`` / ``hcf_aux_bn_act_backward`` (batch statistics in train(), running statistics in
  eval(), the module's own buffers updated on the device); PatchGAN's padding-0 convs are the interior window of the
  same-padded conv, which those kernels read (forward) and zero-border (backward);
* in ``Discriminator_VGG_160`` and ``VGGFeatureExtractor``, BatchNorm stays on stock PyTorch ops; the Linear layers,
  max-pooling and the losses are a few elementwise / reduction ops per layer and stay on stock PyTorch ops in these modules;
* ``PerceptualLoss`` is the generator step's whole feature loss ``cri_fea(netF(fake_H), netF(real_H).detach())`` as one autograd
  node: netF's convs, with input normalisation, max-pooling, the fused max-pool + ReLU backward and the L1 / MSE criterion on the
  kernels of ``hcf_vgg.hip`` (``hcf_aux_input_norm``, ``hcf_aux_maxpool2``, ``hcf_aux_maxpool2_act_backward``,
  ``hcf_aux_act_backward``, ``hcf_aux_feature_loss``).

``VGGFeatureExtractor`` needs torchvision's pretrained VGG19 weights, which cannot be downloaded here: the layer stack is
rebuilt from the VGG19 configuration with the same ``features.N`` keys, so a torchvision ``vgg19().features`` state dict loads
strictly; without one the weights are random. No CPU fallback: ``forward`` raises ``HcfError`` off-GPU.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

_PREC = {"exact": 0, "f16x3": 1}


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    """NCHW -> dense NHWC fp32 with the channel count padded to a multiple of 4."""
    B, Cc, H, W = x.shape
    y = x.permute(0, 2, 3, 1).to(torch.float32)
    if Cc % 4:
        y = F.pad(y, (0, 4 - Cc % 4))
    return y.contiguous()


def _nchw(y: torch.Tensor, Cc: int) -> torch.Tensor:
    return y[..., :Cc].permute(0, 3, 1, 2)


def squeeze2d_nhwc(x: torch.Tensor) -> torch.Tensor:
    """[B,H,W,C] -> [B,H/2,W/2,4C], channel order c*4 + a*2 + b (Basic.squeeze2d, Basic.py:127-141)."""
    B, H, W, Cc = x.shape
    return x.view(B, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, 4 * Cc).contiguous()


def _w4s2_as_3x3(w: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d(C, O, 4, 2, 1) weight [O,C,4,4] -> the 3x3 stride-1 weight [O,4C,3,3] acting on squeeze2d(x):
    out[y,x] = sum_ij w[i,j] in[2y-1+i, 2x-1+j]; input row 2y-1+i = squeezed row y+dy, sub-row a with
    (i -> dy, a) = 0 -> (-1, 1), 1 -> (0, 0), 2 -> (0, 1), 3 -> (+1, 0); same for columns."""
    O, Cc = w.shape[0], w.shape[1]
    w3 = w.new_zeros(O, Cc, 2, 2, 3, 3)
    m = ((0, -1, 1), (1, 0, 0), (2, 0, 1), (3, 1, 0))
    for i, dy, a in m:
        for j, dx, b in m:
            w3[:, :, a, b, dy + 1, dx + 1] = w[:, :, i, j]
    return w3.reshape(O, 4 * Cc, 3, 3)


def _workspace(work, key, need, device, zeroed):
    """The scratch buffer work[key] of at least `need` bytes on `device` (re)allocated when missing or too small. Every key names
    its DEVICE and STREAM: nn.DataParallel replicas share the dict (replicate() shallow-copies __dict__), one replica thread per
    device (HCFlow_SR_model.py:76,94 wrap netD / netF); calls on a stream run in order, and a buffer holds state of the call in
    flight only."""
    wk = work.get(key)
    if wk is None or wk.numel() < need or wk.device != device:
        wk = (torch.zeros if zeroed else torch.empty)(need, dtype=torch.uint8, device=device)
        work[key] = wk
    return wk


def _conv_forward(x, w, bias, act, prec, work, flags):
    """y = act(conv_k(x, w) + bias): NHWC x, contiguous w [cout,cin,k,k]; y has cout rounded up to 4 channels (the padding zero).
    Returns (y, wk); wk, the call's workspace (packs, the range flag, weight-gradient partials), also joins `flags`."""
    lib = _lib.load()
    B, H, W, cs = x.shape
    cout, cin, k, _ = w.shape
    y = torch.empty(B, H, W, (cout + 3) & ~3, device=x.device, dtype=torch.float32)
    if y.shape[3] != cout:
        y.zero_()
    wk = _workspace(work, (x.device.index, _lib.current_stream(x.device), cin, cout, k, B, H, W),
                    lib.hcf_aux_conv2d_workspace(cin, cout, k, B, H, W), x.device, zeroed=True)   # [0, 256): range flag + zero page
    flags.append(wk)
    b = None if bias is None else bias.contiguous()
    _lib.launch("hcf_aux_conv2d", x.device, x, cs, cin, B, H, W, w, b, cout, k, act, y, y.shape[3], wk, wk.numel(), prec)
    return y, wk


def _conv_backward(x, w, g, dx, dw, wk, prec):
    """Gradients of conv_k(x, w) given g = dL/d(pre-activation) into the caller's dx (channels [0, cin)) and dw; None: skipped."""
    B, H, W, cs = x.shape
    cout, cin, k, _ = w.shape
    _lib.launch("hcf_aux_conv2d_backward", x.device, x, cs, cin, B, H, W, w, cout, k, g, g.shape[3], dx, cs, dw, wk, wk.numel(), prec)


def _range_redo(run, prec, restore=None):
    """run(prec, flags) speculatively at the requested precision. Under f16x3 the convs raise the flag word of their workspace
    when an activation leaves the f16 range (the pass then holds inf / NaN): every flag is cleared, `restore` undoes what the
    pass left behind, and the pass is redone exactly. The flag read is the one stream sync of an f16x3 call."""
    flags = []
    out = run(prec, flags)
    if prec == 1 and flags:
        uniq = list({id(f): f for f in flags}.values())
        if bool(torch.stack([f[:4].view(torch.int32)[0] for f in uniq]).any()):
            for f in uniq:
                f[:4].zero_()
            if restore is not None:
                restore()
            out = run(0, [])
    return out


class _ConvNHWC(torch.autograd.Function):
    """y = act(conv_k(x, w) + bias) on NHWC device tensors through the C ABI; act in {0 none, 1 relu, 2 lrelu 0.2}."""

    @staticmethod
    def forward(ctx, x, w, bias, act, prec, work, flag_owner):
        if not x.is_cuda:
            raise _lib.HcfError("hcflow_amd.gan runs on MI355X only (no CPU fallback): move the module and its inputs to a GPU")
        assert x.shape[3] % 4 == 0 and x.shape[3] >= w.shape[1] and x.is_contiguous() and x.dtype == torch.float32
        w = w.contiguous()
        y, wk = _conv_forward(x, w, bias, act, prec, work, flag_owner)
        ctx.save_for_backward(x, w, y if act else None)
        ctx.meta = (act, prec, bias is not None, wk)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w, y = ctx.saved_tensors
        act, prec, has_bias, wk = ctx.meta
        g = g.contiguous()
        if act == 1:
            g = g * (y > 0)
        elif act == 2:
            g = g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.2))
        dx = torch.zeros_like(x) if ctx.needs_input_grad[0] else None
        dw = torch.empty_like(w) if ctx.needs_input_grad[1] else None       # frozen weights (VGG; netD during the G step): skipped
        _conv_backward(x, w, g, dx, dw, wk, prec)
        db = g[..., :w.shape[0]].sum(dim=(0, 1, 2)) if (has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db, None, None, None, None


_BN_NONE, _BN_TRAIN, _BN_EVAL = 0, 1, 2


def _interior(y: torch.Tensor):
    """The window (y0, x0, Ho, Wo) of a same-padded 3x3 conv's output [B,H,W,c] that equals the padding-0 conv's output."""
    return (1, 1, y.shape[1] - 2, y.shape[2] - 2)


def _bn_workspace(work, x, need):
    # not inlined: the forward and the backward pass must name the same key
    return _workspace(work, ("bn", x.device.index, _lib.current_stream(x.device)), max(need, 256), x.device, zeroed=False)


class _BnActNHWC(torch.autograd.Function):
    """y = act(BatchNorm2d(x[:, y0:y0+Ho, x0:x0+Wo, :C])) as a compact NHWC [B,Ho,Wo,roundup4(C)] device tensor through the C ABI
    (hcf_aux_bn_act); bn None: the window and the activation only. act in {0 none, 1 relu, 2 lrelu 0.2}. train() mode (or no
    running statistics) normalises with the batch statistics and moves bn's running_mean / running_var in place on the device;
    the backward pass returns dx over the whole H x W input with a zero border."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, Cc, window, act, work):
        if not x.is_cuda:
            raise _lib.HcfError("hcflow_amd.gan runs on MI355X only (no CPU fallback): move the module and its inputs to a GPU")
        lib = _lib.load()
        B, H, W, cs = x.shape
        y0, x0, Ho, Wo = window
        assert cs % 4 == 0 and cs >= Cc and x.is_contiguous() and x.dtype == torch.float32
        y = torch.empty(B, Ho, Wo, (Cc + 3) & ~3, device=x.device, dtype=torch.float32)
        smean = sinv = rmean = rvar = wk = None
        momentum, eps = 0.0, 1e-5
        if bn is None:
            mode = _BN_NONE
        else:
            eps = float(bn.eps)
            tracked = bn.track_running_stats and bn.running_mean is not None
            mode = _BN_TRAIN if (bn.training or not tracked) else _BN_EVAL
            if tracked:
                rmean, rvar = bn.running_mean, bn.running_var
                assert rmean.is_contiguous() and rvar.is_contiguous() and rmean.dtype == torch.float32
            if mode == _BN_TRAIN:
                if B * Ho * Wo < 2:
                    raise ValueError("Expected more than 1 value per channel when training, got input size %r"
                                     % ([B, Cc, Ho, Wo],))
                momentum = 0.0 if bn.momentum is None else float(bn.momentum)
                if bn.training and tracked:
                    with torch.no_grad():
                        bn.num_batches_tracked.add_(1)
                    if bn.momentum is None:                  # cumulative moving average (nn.BatchNorm2d)
                        momentum = 1.0 / float(bn.num_batches_tracked)
                else:
                    rmean = rvar = None                       # batch statistics without running statistics to move
                wk = _bn_workspace(work, x, lib.hcf_aux_bn_act_workspace(Cc, B, Ho, Wo))
            smean = torch.empty(Cc, device=x.device, dtype=torch.float32)
            sinv = torch.empty(Cc, device=x.device, dtype=torch.float32)
            gamma, beta = gamma.contiguous(), beta.contiguous()
        _lib.launch("hcf_aux_bn_act", x.device, x, cs, Cc, B, H, W, y0, x0, Ho, Wo, gamma, beta, rmean, rvar, mode, momentum, eps, act,
                    y, y.shape[3], smean, sinv, wk, 0 if wk is None else wk.numel())
        ctx.save_for_backward(x, gamma, beta, smean, sinv)
        ctx.meta = (Cc, window, act, mode, work)
        return y

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, gamma, beta, smean, sinv = ctx.saved_tensors
        Cc, (y0, x0, Ho, Wo), act, mode, work = ctx.meta
        B, H, W, cs = x.shape
        g = g.contiguous()
        dx = torch.empty_like(x)                              # every element written, the border and the padding channels as 0
        need_p = mode != _BN_NONE and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dgamma = torch.empty_like(gamma) if need_p else None  # frozen parameters (netD during the G step): skipped
        dbeta = torch.empty_like(beta) if need_p else None
        wk = None
        if mode == _BN_TRAIN or need_p:
            wk = _bn_workspace(work, x, lib.hcf_aux_bn_act_workspace(Cc, B, Ho, Wo))
        _lib.launch("hcf_aux_bn_act_backward", x.device, x, cs, Cc, B, H, W, y0, x0, Ho, Wo, gamma, beta, smean, sinv, mode, act,
                    g, g.shape[3], dx, cs, dgamma, dbeta, wk, 0 if wk is None else wk.numel())
        return (dx, dgamma if ctx.needs_input_grad[1] else None, dbeta if ctx.needs_input_grad[2] else None,
                None, None, None, None, None)


class _AuxNet(nn.Module):
    """Shared plumbing: precision policy and the per-layer workspaces."""

    def _aux_init(self):
        object.__setattr__(self, "_work", {})
        object.__setattr__(self, "_prec", ["exact"])

    def set_precision(self, mode: str):
        """"exact" (default): fp32-MFMA convs. "f16x3": fp32-equivalent split convs for the 3x3 forward passes; an input beyond
        the f16 range is detected after the pass and the pass is redone exactly (one stream sync per forward)."""
        assert mode in _PREC
        self._prec[0] = mode
        return self

    def _conv(self, x, conv: nn.Conv2d, act: int, flags, prec):
        w = conv.weight
        if conv.kernel_size == (4, 4):                       # 4x4 stride 2 pad 1 == squeeze2d + re-indexed 3x3
            x = squeeze2d_nhwc(x)
            w = _w4s2_as_3x3(w)
        return _ConvNHWC.apply(x, w, conv.bias, act, prec, self._work, flags)

    def _bn_act(self, y, bn: Optional[nn.BatchNorm2d], Cc: int, window=None, act: int = 2):
        """act(bn(window of y)) on the fused kernels (bn None: window + act only); window None: the whole of y."""
        win = (0, 0, y.shape[1], y.shape[2]) if window is None else window
        if bn is None:
            return _BnActNHWC.apply(y, None, None, None, Cc, win, act, self._work)
        return _BnActNHWC.apply(y, bn.weight, bn.bias, bn, Cc, win, act, self._work)

    def _run(self, body, x):
        prec = _PREC[self._prec[0]]
        # a speculative f16x3 pass in train() mode updates every BatchNorm's running statistics; if it is thrown away (range
        # overflow: its activations were inf / NaN) the exact re-run must start from the statistics BEFORE it
        restore = None
        if prec == 1 and self.training:
            bn_state = [(m, m.running_mean.clone(), m.running_var.clone(), m.num_batches_tracked.clone())
                        for m in self.modules() if isinstance(m, nn.BatchNorm2d) and m.track_running_stats and m.running_mean is not None]

            @torch.no_grad()
            def restore():
                for m, mean, var, cnt in bn_state:
                    m.running_mean.copy_(mean)
                    m.running_var.copy_(var)
                    m.num_batches_tracked.copy_(cnt)
        return _range_redo(lambda p, flags: body(x, flags, p), prec, restore)


class _DiscriminatorVGG(_AuxNet):
    """The VGG-style discriminators of discriminator_vgg_arch.py (:6-65, :68-107): ten convs (every second one 4x4 stride 2),
    BatchNorm + LeakyReLU after all but the first, two Linear layers on the fc_side x fc_side map that is left. Same modules /
    state_dict as the reference; convs on our conv kernels, BatchNorm + LeakyReLU as the subclass runs it (_bn_lrelu)."""

    def __init__(self, in_nc, nf, fc_side):
        super().__init__()
        self.conv0_0 = nn.Conv2d(in_nc, nf, 3, 1, 1, bias=True)
        self.conv0_1 = nn.Conv2d(nf, nf, 4, 2, 1, bias=False)
        self.bn0_1 = nn.BatchNorm2d(nf, affine=True)
        chans = [(nf, nf * 2), (nf * 2, nf * 4), (nf * 4, nf * 8), (nf * 8, nf * 8)]
        for i, (ci, co) in enumerate(chans, start=1):
            setattr(self, "conv%d_0" % i, nn.Conv2d(ci, co, 3, 1, 1, bias=False))
            setattr(self, "bn%d_0" % i, nn.BatchNorm2d(co, affine=True))
            setattr(self, "conv%d_1" % i, nn.Conv2d(co, co, 4, 2, 1, bias=False))
            setattr(self, "bn%d_1" % i, nn.BatchNorm2d(co, affine=True))
        self.linear1 = nn.Linear(512 * fc_side * fc_side, 100)
        self.linear2 = nn.Linear(100, 1)
        self.lrelu = nn.LeakyReLU(negative_slope=0.2, inplace=True)
        self._aux_init()

    def _bn_lrelu(self, y, bn: nn.BatchNorm2d):
        raise NotImplementedError

    def _body(self, x, flags, prec):
        fea = self._conv(_nhwc(x), self.conv0_0, 2, flags, prec)                       # bias + LeakyReLU fused
        fea = self._bn_lrelu(self._conv(fea, self.conv0_1, 0, flags, prec), self.bn0_1)
        for i in range(1, 5):
            fea = self._bn_lrelu(self._conv(fea, getattr(self, "conv%d_0" % i), 0, flags, prec), getattr(self, "bn%d_0" % i))
            fea = self._bn_lrelu(self._conv(fea, getattr(self, "conv%d_1" % i), 0, flags, prec), getattr(self, "bn%d_1" % i))
        fea = fea.permute(0, 3, 1, 2).reshape(fea.size(0), -1)                         # the reference flattens NCHW
        fea = self.lrelu(self.linear1(fea))
        return self.linear2(fea)

    def forward(self, x):
        return self._run(self._body, x)

    def reset_parameters(self):
        for layer in self.children():
            if hasattr(layer, "reset_parameters"):
                layer.reset_parameters()


class Discriminator_VGG_128(_DiscriminatorVGG):
    """Drop-in for discriminator_vgg_arch.Discriminator_VGG_128 (:6-65): 128 x 128 input, ``linear1`` on 512 * 4 * 4 features;
    every BatchNorm + LeakyReLU on the fused BN kernels."""

    def __init__(self, in_nc, nf):
        super().__init__(in_nc, nf, fc_side=4)

    def _bn_lrelu(self, y, bn: nn.BatchNorm2d):
        return self._bn_act(y, bn, bn.num_features)


class Discriminator_VGG_160(_DiscriminatorVGG):
    """Drop-in for discriminator_vgg_arch.Discriminator_VGG_160 (:68-107): 160 x 160 input, ``linear1`` on 512 * 5 * 5 features;
    BatchNorm + LeakyReLU on stock PyTorch ops."""

    def __init__(self, in_nc, nf):
        super().__init__(in_nc, nf, fc_side=5)

    def _bn_lrelu(self, y, bn: nn.BatchNorm2d):
        Cc = bn.num_features
        v = bn(y[..., :Cc].permute(0, 3, 1, 2))               # channels-last view: no copy; batch / running statistics as nn.BatchNorm2d
        return F.leaky_relu(v, 0.2).permute(0, 2, 3, 1).contiguous()


_VGG19 = [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"]


def _vgg19_features(use_bn):
    layers, cin = [], 3
    for v in _VGG19:
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers.append(nn.Conv2d(cin, v, kernel_size=3, padding=1))
            if use_bn:
                layers.append(nn.BatchNorm2d(v))
            layers.append(nn.ReLU(inplace=True))
            cin = v
    return layers


def _vgg_plan(netF, who="VGGFeatureExtractor"):
    """VGGFeatureExtractor.features as [(conv, bn, relu, pooled)]: each conv with the BatchNorm2d (or None), the ReLU and the
    MaxPool2d that follow it, in that order. The ReLU is fused into the conv where no BatchNorm sits between them."""
    mods, plan, i = list(netF.features), [], 0

    def take(kind):                                          # the next module if it is a `kind` (consumed), else None
        nonlocal i
        if i < len(mods) and isinstance(mods[i], kind):
            i += 1
            return mods[i - 1]
        return None

    while i < len(mods):
        conv = take(nn.Conv2d)
        if conv is None:
            raise ValueError("%s: unexpected %s at features.%d" % (who, type(mods[i]).__name__, i))
        bn = take(nn.BatchNorm2d)
        relu = take(nn.ReLU) is not None
        plan.append((conv, bn, relu, take(nn.MaxPool2d) is not None))
    return plan


class VGGFeatureExtractor(_AuxNet):
    """Drop-in for discriminator_vgg_arch.VGGFeatureExtractor (:110-137): VGG19 ``features[:feature_layer + 1]`` (34 = conv5_4
    before its ReLU), input normalisation, frozen weights. The stack has torchvision's ``features.N`` keys; pretrained weights
    are whatever the caller loads (none ship here)."""

    def __init__(self, feature_layer=34, use_bn=False, use_input_norm=True, device=torch.device("cpu")):
        super().__init__()
        self.use_input_norm = use_input_norm
        if self.use_input_norm:
            self.register_buffer("mean", torch.Tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1).to(device))
            self.register_buffer("std", torch.Tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1).to(device))
        self.features = nn.Sequential(*_vgg19_features(use_bn)[:(feature_layer + 1)])
        for k, v in self.features.named_parameters():
            v.requires_grad = False
        self._aux_init()

    def _body(self, x, flags, prec):
        if self.use_input_norm:
            x = (x - self.mean) / self.std
        y, Cc = _nhwc(x), 3
        for conv, bn, relu, pooled in _vgg_plan(self):
            Cc = conv.out_channels
            y = _ConvNHWC.apply(y, conv.weight, conv.bias, int(relu and bn is None), prec, self._work, flags)
            if bn is not None:
                y = bn(y[..., :Cc].permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
                if relu:
                    y = F.relu(y)
            if pooled:
                y = F.max_pool2d(y[..., :Cc].permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
        return _nchw(y, Cc).contiguous()

    def forward(self, x):
        return self._run(self._body, x)


class PatchGANDiscriminator(_AuxNet):
    """Drop-in for discriminator_vgg_arch.PatchGANDiscriminator (:159-189): ``model`` is the reference's ``nn.Sequential`` with its
    module indices (``model.0`` conv + bias, ``model.{2+3i}`` conv, ``model.{3+3i}`` BatchNorm2d, LeakyReLUs in between,
    ``model.{2+3n}`` the 1-channel conv), so keys and the seeded default initialisation match. Every 3x3 padding-0 conv runs as
    the same-padded conv kernel whose interior window the next step reads: the fused BN + LeakyReLU kernels for the n_layers
    middle layers, the window-only form of the same kernels after the first and the last conv. Output [B, 1, H - 2(n+2),
    W - 2(n+2)]."""

    def __init__(self, in_nc=3, ndf=64, n_layers=35, norm_layer=nn.BatchNorm2d):
        super().__init__()
        seq = [nn.Conv2d(in_nc, ndf, kernel_size=3, stride=1, padding=0), nn.LeakyReLU(0.2, True)]
        for _ in range(n_layers):
            seq += [nn.Conv2d(ndf, ndf, kernel_size=3, stride=1, padding=0, bias=False), norm_layer(ndf), nn.LeakyReLU(0.2, True)]
            if not (type(seq[-2]) is nn.BatchNorm2d and seq[-2].affine):
                raise NotImplementedError("PatchGANDiscriminator: only norm_layer=nn.BatchNorm2d (affine) has a kernel here")
        seq += [nn.Conv2d(ndf, 1, kernel_size=3, stride=1, padding=0, bias=False)]
        self.model = nn.Sequential(*seq)
        self.n_layers = n_layers
        self._aux_init()

    def _body(self, x, flags, prec):
        m, n = self.model, self.n_layers
        y = self._conv(_nhwc(x), m[0], 2, flags, prec)                                 # bias + LeakyReLU fused
        y = self._bn_act(y, None, m[0].out_channels, _interior(y), act=0)
        for i in range(n):
            conv, bn = m[2 + 3 * i], m[3 + 3 * i]
            y = self._conv(y, conv, 0, flags, prec)
            y = self._bn_act(y, bn, bn.num_features, _interior(y))
        y = self._conv(y, m[2 + 3 * n], 0, flags, prec)
        return _nchw(self._bn_act(y, None, 1, _interior(y), act=0), 1)

    def forward(self, x):
        shrink = 2 * (self.n_layers + 2)
        if x.dim() != 4 or x.shape[2] <= shrink or x.shape[3] <= shrink:
            raise ValueError("PatchGANDiscriminator(n_layers=%d): its %d padding-0 3x3 convs need an input larger than %d x %d, "
                             "got %s" % (self.n_layers, self.n_layers + 2, shrink, shrink, tuple(x.shape)))
        return self._run(self._body, x)


_CRITERIA = {"l1": 0, "l2": 1, "mse": 1}                    # feature_criterion of the recipes (HCFlow_SR_model.py:62-66)


def _perceptual_plan(netF):
    """_vgg_plan(netF), if PerceptualLoss has kernels for all of it."""
    plan = _vgg_plan(netF, "PerceptualLoss")
    if any(bn is not None for _, bn, _, _ in plan):
        raise ValueError("PerceptualLoss: use_bn=True (BatchNorm VGG) has no fused path here; networks.define_F builds "
                         "VGGFeatureExtractor(use_bn=False)")
    if not plan or plan[-1][3]:
        raise ValueError("PerceptualLoss: feature_layer must end on a conv or a ReLU (a trailing MaxPool2d is not supported)")
    return plan


class _PerceptualLossFn(torch.autograd.Function):
    """cri_fea(netF(fake), netF(real).detach()) as ONE node: convs through hcf_aux_conv2d / hcf_aux_conv2d_backward (dw = NULL,
    VGG is frozen), everything between them through the kernels of hcf_vgg.hip. The real pass keeps nothing; the fake pass keeps
    each conv's input and post-activation output; the loss kernel leaves dloss/dfeature, which backward scales and walks down."""

    @staticmethod
    def _pass(lib, netF, plan, x, prec, flags, keep):
        B, _, H, W = x.shape
        dev = x.device
        y = torch.empty(B, H, W, 4, device=dev, dtype=torch.float32)
        norm = netF.use_input_norm
        _lib.launch("hcf_aux_input_norm", dev, x, netF.mean if norm else None, netF.std if norm else None, B, H, W, y)
        tape = []
        for conv, _, relu, pooled in plan:
            cout, w = conv.out_channels, conv.weight.contiguous()
            z, wk = _conv_forward(y, w, conv.bias, int(relu), prec, netF._work, flags)       # VGG19 widths are multiples of 4
            if keep:
                tape.append((y, z if (relu or pooled) else None, w, wk))
            y = z
            if pooled:
                if H < 2 or W < 2:
                    raise ValueError("PerceptualLoss: the input is too small for the %d max-pools of this feature_layer"
                                     % sum(p for _, _, _, p in plan))
                p = torch.empty(B, H // 2, W // 2, cout, device=dev, dtype=torch.float32)
                _lib.launch("hcf_aux_maxpool2", dev, y, cout, cout, B, H, W, p, cout)
                y, H, W = p, H // 2, W // 2
        return y, tape

    @staticmethod
    def forward(ctx, fake, real, netF, plan, kind):
        lib = _lib.load()
        need_grad = ctx.needs_input_grad[0]
        xf, xr = fake.detach().to(torch.float32).contiguous(), real.detach().to(torch.float32).contiguous()

        def both(prec, flags):                                 # the real pass keeps nothing
            fr, _ = _PerceptualLossFn._pass(lib, netF, plan, xr, prec, flags, False)
            return (fr,) + _PerceptualLossFn._pass(lib, netF, plan, xf, prec, flags, need_grad)

        dev = fake.device
        fr, ff, tape = _range_redo(both, _PREC[netF._prec[0]])
        n = ff.numel()
        wk = _workspace(netF._work, ("fea", dev.index, _lib.current_stream(dev)), lib.hcf_aux_feature_loss_workspace(n), dev,
                        zeroed=False)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        gfea = torch.empty_like(ff) if need_grad else None
        _lib.launch("hcf_aux_feature_loss", dev, ff, fr, n, kind, loss, gfea, wk, wk.numel())
        ctx.tape, ctx.gfea, ctx.plan, ctx.netF = tape, gfea, plan, netF
        ctx.in_meta = (tuple(fake.shape), fake.dtype)
        return loss

    @staticmethod
    def backward(ctx, gout):
        plan, netF = ctx.plan, ctx.netF
        (B, _, H0, W0), dtype = ctx.in_meta
        g = ctx.gfea * gout                                    # a fresh tensor: the in-place activation backward below owns it
        dev = g.device
        for (conv, _, relu, pooled), (x, y, w, wk) in zip(reversed(plan), reversed(ctx.tape)):
            _, H, W, _ = x.shape
            cout, act = conv.out_channels, int(relu)
            if pooled:
                gpre = torch.empty(B, H, W, cout, device=dev, dtype=torch.float32)
                _lib.launch("hcf_aux_maxpool2_act_backward", dev, g, cout, y, cout, cout, B, H, W, act, gpre, cout)
                g = gpre
            elif act:
                _lib.launch("hcf_aux_act_backward", dev, g, y, act, g.numel(), g)
            dx = torch.empty_like(x)                           # channels [0, cin) written; the 4th channel of the image layer is never read
            _conv_backward(x, w, g, dx, None, wk, 0)
            g = dx
        gx = torch.empty(B, 3, H0, W0, device=dev, dtype=torch.float32)
        _lib.launch("hcf_aux_input_norm_backward", dev, g, netF.std if netF.use_input_norm else None, B, H0, W0, gx)
        return gx.to(dtype), None, None, None, None


class PerceptualLoss(nn.Module):
    """The feature loss of the HCFlow++ generator step (HCFlow_SR_model.py:229-232, HCFlow_Rescaling_model.py:237-240) as one call:

        cri = PerceptualLoss(netF, criterion="l1")           # netF: VGGFeatureExtractor, or nn.DataParallel around one
        l_g_fea = l_fea_w * cri(fake_H, real_H)              # == cri_fea(netF(fake_H), netF(real_H).detach())

    ``criterion``: the recipe's ``feature_criterion``, "l1" or "l2" ("mse"). Only ``fake_H`` receives a gradient. The convs are
    netF's own (``hcf_aux_conv2d`` at netF's ``set_precision``, ``hcf_aux_conv2d_backward`` without the weight gradient); input
    normalisation, max-pooling, the ReLU / max-pool backward and the criterion run on the kernels of ``hcf_vgg.hip``. Supports
    ``use_bn=False`` stacks whose ``feature_layer`` ends on a conv or a ReLU, ``use_input_norm`` either way. No CPU fallback."""

    def __init__(self, netF, criterion: str = "l1"):
        super().__init__()
        if isinstance(netF, (nn.DataParallel, nn.parallel.DistributedDataParallel)):
            netF = netF.module                                # the loss runs on the device of its inputs, keyed workspaces per device
        if not isinstance(netF, VGGFeatureExtractor):
            raise TypeError("PerceptualLoss: netF must be a hcflow_amd.gan.VGGFeatureExtractor, got %s" % type(netF).__name__)
        if criterion not in _CRITERIA:
            raise ValueError("PerceptualLoss: criterion must be one of %s, got %r" % (sorted(_CRITERIA), criterion))
        _perceptual_plan(netF)                                # raises ValueError for use_bn=True
        self.netF = netF
        self.kind = _CRITERIA[criterion]

    def forward(self, fake_H, real_H):
        if real_H.requires_grad:
            raise ValueError("PerceptualLoss: real_H requires grad, but the target features are detached (netF(real_H).detach()): "
                             "pass real_H.detach()")
        if not (fake_H.is_cuda and real_H.is_cuda):
            raise _lib.HcfError("hcflow_amd.gan runs on MI355X only (no CPU fallback): move the module and its inputs to a GPU")
        if fake_H.dim() != 4 or fake_H.shape[1] != 3 or fake_H.shape != real_H.shape or fake_H.device != real_H.device:
            raise ValueError("PerceptualLoss: fake_H and real_H must be [B,3,H,W] of one shape on one device, got %s and %s"
                             % (tuple(fake_H.shape), tuple(real_H.shape)))
        plan = _perceptual_plan(self.netF)                    # per call: a DataParallel replica has its own conv modules
        convs = [c for c, _, _, _ in plan]
        if any(c.weight.requires_grad or (c.bias is not None and c.bias.requires_grad) for c in convs):
            raise ValueError("PerceptualLoss: the VGG weights must be frozen (requires_grad=False), no weight gradient is computed")
        if convs[0].weight.device != fake_H.device:
            raise ValueError("PerceptualLoss: netF is on %s, the inputs on %s" % (convs[0].weight.device, fake_H.device))
        return _PerceptualLossFn.apply(fake_H, real_H, self.netF, plan, self.kind)
