"""LPIPS v0.1 with AlexNet on the MI355X kernels: the LPIPS column of the reference's test log.

``test_HCFlow.py:48`` builds ``loss_fn_alex = lpips.LPIPS(net='alex')`` and ``:132-133`` evaluates it on
``(2 * gt - 1, 2 * sr - 1)``. ``LPIPS`` here is a drop-in for ``lpips.LPIPS(net='alex')`` (version 0.1, ``lpips=True``,
``spatial=False``) that runs the whole network as ONE call of the C ABI (``hcf_lpips_alex`` in ``include/hcflow.h``,
``csrc/hcf_lpips.hip``), exact fp32 throughout. The math, for inputs x0, x1 in [-1, 1] (``normalize=True``: in [0, 1], mapped by
2x - 1 first):

* scaling layer: ``x' = (x - shift) / scale``, shift ``[-.030, -.088, -.188]``, scale ``[.458, .448, .450]``, applied before
  conv1's zero padding;
* AlexNet features ``relu_l``, l = 1..5 (the ReLU output after each conv):
  conv1 3 -> 64, 11x11, stride 4, pad 2; MaxPool 3 / 2; conv2 64 -> 192, 5x5, pad 2; MaxPool 3 / 2;
  conv3 192 -> 384, 3x3, pad 1; conv4 384 -> 256, 3x3, pad 1; conv5 256 -> 256, 3x3, pad 1;
* per layer: unit-normalise every pixel over channels, ``f / (sqrt(sum_c f^2) + 1e-10)``, square the difference of the two
  normalised maps, apply the 1x1 linear head ``lin_l`` (no bias), average over space;
* ``d(x0, x1) = sum_l`` of the five layer terms, returned as ``[B, 1, 1, 1]`` fp32 (``retPerLayer=True``: also the list of
  the five ``[B, 1, 1, 1]`` terms).

conv1 runs as a 5x5 stride-1 conv on the 4x4 space-to-depth grid of the scaled image (``alex_conv1_as_s2d`` re-indexes the
weight); H, W >= 31 is AlexNet's minimum (conv1 gives >= 7 rows, pool1 >= 3, pool2 >= 1).

``state_dict()`` has the keys and shapes of ``lpips.LPIPS(net='alex')``: ``scaling_layer.shift / scale``,
``net.slice{1..5}.{0,3,6,8,10}.weight / bias``, ``lin{0..4}.model.1.weight`` ``[1, C, 1, 1]``; ``lins.K.*`` aliases (the
``ModuleList`` lpips also registers) are accepted on load. ``load_pretrained(tv_alexnet, lpips_lin)`` fills the module from the
two files users keep offline: torchvision's AlexNet state dict (``features.{0,3,6,8,10}.*``, ``alexnet-owt-7be5be79.pth``) and
lpips' ``weights/v0.1/alex.pth``. Nothing is ever downloaded: without weights the parameters are seeded random.

No CPU fallback (off-GPU inputs raise ``HcfError``). ``LPIPS`` is the frozen metric: it has no backward, and inputs that
require grad raise. The call runs on the current stream without host synchronisation, is bit-reproducible, and an image's value
does not depend on the rest of the batch.

``LPIPSLoss(metric, reduction="mean")`` is the same measure as a loss (where a feature loss enters the generator step,
``HCFlow_SR_model.py:229-232``): one ``autograd.Function`` node whose forward is the metric's own call, bit for bit, and whose
backward is ONE call of ``hcf_lpips_alex_backward``, which walks back down the feature maps that the forward left in its
workspace. Each of ``in0`` / ``in1`` that requires grad receives a gradient (the backward convolutions cover only those halves
of the stacked batch); the parameters are frozen. Per layer and pixel, with ``n_i = sum_c f_i^2``, ``d_i = sqrt(n_i) + 1e-10``
and ``a_c = 2 w_c (f0_c / d0 - f1_c / d1) gout[b] / (h_l w_l)``:

    ``g_f0_c = a_c / d0 - f0_c (sum_k a_k f0_k) / (d0^2 sqrt(n0))``,  ``g_f1`` the same with ``-a``;

the term through the norm is DEFINED as 0 where ``n_i == 0`` (PyTorch autograd of the formula gives ``0 * inf = NaN`` there).
The max-pool backward gives a window's gradient to its first maximum in row-major order, as PyTorch does. No atomics: the
gradient is bit-reproducible, and sample b's gradient does not depend on the rest of the batch. No double backward.

``LPIPSMap(metric)`` is the same measure for sample sets, where one GT meets M samples (``hcf_lpips_alex_embed`` /
``hcf_lpips_alex_map``). ``embed(gt)`` runs AlexNet over the GT once and keeps its feature maps; ``compare(ref, sr)`` runs it over
the sample alone and the head against the kept maps: its ``[B, 1, 1, 1]`` is ``metric(gt, sr)`` bit for bit, with the convolutions
over B (M + 1) images where M metric calls take 2 B M. With ``spatial=True`` it also returns the per-pixel map
``D = sum_l up_l(d_l)`` of ``lpips.LPIPS(spatial=True)``: ``d_l`` is layer l's per-pixel value before the spatial mean, ``up_l``
PyTorch's bilinear upsampling to ``(H, W)`` with ``align_corners=False`` (source row ``sy = max(0, (y + 0.5) h_l / H - 0.5)``,
rows ``floor(sy)`` and ``min(floor(sy) + 1, h_l - 1)``, weight ``sy - floor(sy)``; columns alike), summed in layer order.
``sample_set(gt)`` accumulates, on the device, over the samples given to ``add``: ``map_mean[m, b] = mean_yx D_m[b]``,
``best_map[b] = min_m D_m[b]`` per pixel, ``local_best[b] = mean_yx best_map[b]``, ``global_best[b] = min_m map_mean[m, b]`` and
``score[b] = (global_best - local_best) / global_best`` (0 where ``global_best == 0``): the best whole sample against the
per-pixel best over the set. ``mean(D)`` is not the scalar LPIPS (the upsampling moves the mean by about 1e-4 relative), so the
scalar is returned next to it. The means are fixed-order fp64 sums: the same guarantees as the metric's.
"""
from __future__ import annotations

import ctypes as C
from typing import Mapping, Optional, Union

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

ALEX_CHANNELS = (64, 192, 384, 256, 256)
ALEX_CONV_INDEX = (0, 3, 6, 8, 10)          # torchvision alexnet().features indices of the five convs
MIN_SIDE = 31


def alex_conv1_as_s2d(w: torch.Tensor) -> torch.Tensor:
    """AlexNet conv1 weight [O, C, 11, 11] (stride 4, pad 2) -> the 5x5 stride-1 pad-2 weight [O, 16 C, 5, 5] acting on the 4x4
    space-to-depth grid (channel c * 16 + a * 4 + b holds input row 4Y + a, column 4X + b; zero padded to a multiple of 4).
    Output row y reads input rows 4y - 2 + i, i = 0..10: tap i sits on s2d row y + (i - 2) div 4, sub-row (i - 2) mod 4, i.e.
    j = i + 2 = 4 (dY + 1) + a with dY in -1..2; the 5x5 offset -2 is unused (zero). Same for columns. Exact, differentiable."""
    O, Cc = w.shape[0], w.shape[1]
    assert w.shape[2:] == (11, 11)
    wp = F.pad(w, (2, 3, 2, 3))                                   # j = i + 2 over [0, 16)
    wp = wp.reshape(O, Cc, 4, 4, 4, 4).permute(0, 1, 3, 5, 2, 4)  # [O, C, a, b, dY + 1, dX + 1]
    return F.pad(wp.reshape(O, Cc * 16, 4, 4), (1, 0, 1, 0))      # offsets -2..2 -> 5 taps


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.Tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.Tensor([.458, .448, .450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """lpips' 1x1 linear head (dropout in front, as ``use_dropout=True``; the dropout is inert in eval and in this module)."""

    def __init__(self, chn_in: int):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


class AlexNetSlices(nn.Module):
    """lpips.pretrained_networks.alexnet's module tree: torchvision's ``features`` split after each ReLU, global indices kept."""

    def __init__(self):
        super().__init__()
        feats = [nn.Conv2d(3, 64, 11, 4, 2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
                 nn.Conv2d(64, 192, 5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(3, 2),
                 nn.Conv2d(192, 384, 3, padding=1), nn.ReLU(inplace=True),
                 nn.Conv2d(384, 256, 3, padding=1), nn.ReLU(inplace=True),
                 nn.Conv2d(256, 256, 3, padding=1), nn.ReLU(inplace=True)]
        bounds = ((0, 2), (2, 5), (5, 8), (8, 10), (10, 12))
        for s, (lo, hi) in enumerate(bounds, start=1):
            sl = nn.Sequential()
            for x in range(lo, hi):
                sl.add_module(str(x), feats[x])
            setattr(self, "slice%d" % s, sl)
        self.N_slices = 5

    def convs(self):
        return [getattr(getattr(self, "slice%d" % (s + 1)), str(i)) for s, i in enumerate(ALEX_CONV_INDEX)]


def _checked_params(metric, in0, in1, loss: bool):
    """The input checks of ``LPIPS.forward`` (``loss`` off: inputs that require grad are refused) and ``LPIPSLoss.forward`` (on: the
    metric's parameters must be frozen); returns ``metric._params()``, which live on the inputs' device."""
    if loss and any(p.requires_grad for p in metric.parameters()):
        raise ValueError("LPIPSLoss: the parameters of the metric must be frozen (requires_grad=False), no parameter "
                         "gradient is computed")
    if not (in0.is_cuda and in1.is_cuda):
        raise _lib.HcfError("hcflow_amd.lpips runs on MI355X only (no CPU fallback): move the module and its inputs to a GPU")
    if not loss and (in0.requires_grad or in1.requires_grad):
        raise _lib.HcfError("hcflow_amd.lpips.LPIPS has no backward pass: call it on detached inputs (e.g. under torch.no_grad())")
    if in0.dim() != 4 or in0.shape[1] != 3 or in0.shape != in1.shape:
        raise _lib.HcfError("%s expects two [B,3,H,W] tensors of the same shape, got %s and %s"
                            % ("LPIPSLoss" if loss else "LPIPS", tuple(in0.shape), tuple(in1.shape)))
    H, W = in0.shape[2:]
    if H < MIN_SIDE or W < MIN_SIDE:
        raise _lib.HcfError("LPIPS (AlexNet) needs H, W >= %d, got %dx%d" % (MIN_SIDE, H, W))
    dev = in0.device
    if in1.device != dev:
        raise _lib.HcfError("in0 and in1 are on different devices")
    params = metric._params()
    if any(t.device != dev for t in params):
        raise _lib.HcfError("the LPIPS module's parameters are not on %s: call .to(%s) first" % (dev, dev))
    return params


def _param_ptrs(params):
    return (C.c_void_p * len(params))(*[t.data_ptr() for t in params])


def _alex_forward(params, in0, in1, normalize, per_layer: bool):
    """The one ``hcf_lpips_alex`` call of the metric and of the loss: (out [B], layers [B, 5] or None, the call's workspace)."""
    B, _, H, W = in0.shape
    dev = in0.device
    x0 = in0.detach().to(torch.float32).contiguous()
    x1 = in1.detach().to(torch.float32).contiguous()
    need = _lib.load().hcf_lpips_workspace(B, H, W)
    work = torch.empty(need, dtype=torch.uint8, device=dev)       # stream-ordered reuse by the caching allocator
    out = torch.empty(B, dtype=torch.float32, device=dev)
    layers = torch.empty(B, 5, dtype=torch.float32, device=dev) if per_layer else None
    _lib.launch("hcf_lpips_alex", dev, x0, x1, B, H, W, int(bool(normalize)), _param_ptrs(params), out, layers, work, need)
    return out, layers, work


class LPIPS(nn.Module):
    """Drop-in for ``lpips.LPIPS(net='alex')`` (v0.1) on the MI355X kernels. ``pnet_path`` / ``model_path``: local files of
    torchvision's AlexNet state dict and lpips' ``alex.pth`` (either may be omitted: those parameters stay seeded random).
    ``forward`` is the frozen metric and raises for inputs that require grad: ``LPIPSLoss(metric)`` is the differentiable form."""

    def __init__(self, pretrained: bool = True, net: str = "alex", version: str = "0.1", lpips: bool = True,
                 spatial: bool = False, pnet_rand: bool = False, pnet_tune: bool = False, use_dropout: bool = True,
                 model_path: Optional[str] = None, eval_mode: bool = True, verbose: bool = False,
                 pnet_path: Optional[str] = None, seed: int = 0):
        super().__init__()
        if net != "alex" or version != "0.1" or not lpips or spatial:
            raise _lib.HcfError("hcflow_amd.lpips implements LPIPS v0.1 with AlexNet, lpips=True, spatial=False only")
        self.pnet_type, self.version, self.lpips, self.spatial = net, version, lpips, spatial
        self.scaling_layer = ScalingLayer()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            self.net = AlexNetSlices()
            for l, c in enumerate(ALEX_CHANNELS):
                lin = NetLinLayer(c)
                with torch.no_grad():                                   # trained heads are non-negative
                    lin.model[1].weight.uniform_(0.0, 2.0 / c)
                setattr(self, "lin%d" % l, lin)
        self.L = 5
        for p in self.parameters():
            p.requires_grad = False
        self._register_load_state_dict_pre_hook(self._lins_alias)
        self._s2d_cache = None
        if pnet_path is not None or (pretrained and model_path is not None):
            self.load_pretrained(pnet_path, model_path if pretrained else None)
        if eval_mode:
            self.eval()

    @staticmethod
    def _lins_alias(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for k in [k for k in state_dict if k.startswith(prefix + "lins.")]:
            rest = k[len(prefix) + 5:]
            idx, tail = rest.split(".", 1)
            v = state_dict.pop(k)
            state_dict.setdefault("%slin%s.%s" % (prefix, idx, tail), v)

    def load_pretrained(self, tv_alexnet: Union[None, str, Mapping[str, torch.Tensor]] = None,
                        lpips_lin: Union[None, str, Mapping[str, torch.Tensor]] = None):
        """Copy torchvision's AlexNet weights (``features.{0,3,6,8,10}.weight / bias``; the classifier is ignored) and lpips'
        linear heads (``lin{0..4}.model.1.weight`` or ``lins.K.``) into this module. Paths are read with ``torch.load``."""
        def _get(src):
            return torch.load(src, map_location="cpu") if isinstance(src, str) else src

        sd = {}
        tv = _get(tv_alexnet)
        if tv is not None:
            for s, i in enumerate(ALEX_CONV_INDEX, start=1):
                for kind in ("weight", "bias"):
                    sd["net.slice%d.%d.%s" % (s, i, kind)] = tv["features.%d.%s" % (i, kind)]
        lin = _get(lpips_lin)
        if lin is not None:
            for l in range(5):
                k = "lin%d.model.1.weight" % l
                sd[k] = lin[k] if k in lin else lin["lins.%d.model.1.weight" % l]
        own = self.state_dict()
        for k, v in sd.items():
            if tuple(v.shape) != tuple(own[k].shape):
                raise _lib.HcfError("%s: shape %s, expected %s" % (k, tuple(v.shape), tuple(own[k].shape)))
        self.load_state_dict(sd, strict=False)
        return self

    def _params(self):
        convs = self.net.convs()
        w1 = convs[0].weight
        key = (w1.data_ptr(), w1._version, w1.device)
        if self._s2d_cache is None or self._s2d_cache[0] != key:
            self._s2d_cache = (key, alex_conv1_as_s2d(w1.detach().float()).contiguous())
        ts = [self.scaling_layer.shift, self.scaling_layer.scale, self._s2d_cache[1], convs[0].bias]
        for c in convs[1:]:
            ts += [c.weight, c.bias]
        ts += [getattr(self, "lin%d" % l).model[1].weight for l in range(5)]
        return [t.detach().float().contiguous() for t in ts]

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, retPerLayer: bool = False, normalize: bool = False):
        params = _checked_params(self, in0, in1, loss=False)
        B = in0.shape[0]
        out, layers, _ = _alex_forward(params, in0, in1, normalize, retPerLayer)
        val = out.view(B, 1, 1, 1)
        if retPerLayer:
            return val, [layers[:, l].reshape(B, 1, 1, 1) for l in range(5)]
        return val


class _LPIPSLossFn(torch.autograd.Function):
    """``metric(in0, in1)`` as ONE node. forward: the call of ``LPIPS.forward`` (``_alex_forward``); when an input
    wants a gradient the workspace of that call -- the tape -- and the parameter tensors stay alive in ``ctx``. backward: one
    ``hcf_lpips_alex_backward`` call over the halves of the stacked batch that want a gradient."""

    @staticmethod
    def forward(ctx, in0, in1, params, normalize):
        B, _, H, W = in0.shape
        out, _, work = _alex_forward(params, in0, in1, normalize, False)
        which = int(ctx.needs_input_grad[0]) | (int(ctx.needs_input_grad[1]) << 1)
        if which:                                                       # (under no_grad / detached inputs: no tape)
            ctx.tape = (work, params)
            ctx.meta = (which, B, H, W, int(bool(normalize)), in0.dtype, in1.dtype)
        return out.view(B, 1, 1, 1)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        work, params = ctx.tape
        which, B, H, W, normalize, dt0, dt1 = ctx.meta
        dev = work.device
        g = gout.reshape(B).to(torch.float32).contiguous()
        need = _lib.load().hcf_lpips_backward_workspace(B, H, W, which)
        bwork = torch.empty(need, dtype=torch.uint8, device=dev)
        g0 = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if which & 1 else None
        g1 = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if which & 2 else None
        _lib.launch("hcf_lpips_alex_backward", dev, B, H, W, normalize, _param_ptrs(params), g, which, g0, g1, work, work.numel(),
                    bwork, need)
        return (None if g0 is None else g0.to(dt0), None if g1 is None else g1.to(dt1), None, None)


class LPIPSLoss(nn.Module):
    """LPIPS as a loss, next to the frozen metric (``PerceptualLoss`` sits next to ``VGGFeatureExtractor`` the same way):

        metric = LPIPS(pnet_path=..., model_path=...).cuda()
        crit = LPIPSLoss(metric, reduction="mean")            # "mean" | "sum" | "none" ("none": [B,1,1,1])
        loss = crit(sr, gt, normalize=True)                   # the (in0, in1, normalize) convention of LPIPS.forward
        loss.backward()                                       # sr.grad

    Each of ``in0`` / ``in1`` that requires grad receives a gradient (in its own dtype); the parameters of ``metric`` must be
    frozen (``ValueError`` otherwise). The values are those of ``metric(in0.detach(), in1.detach(), normalize=...)`` bit for
    bit; "mean" / "sum" are torch reductions of that vector. Under ``no_grad``, or when neither input requires grad, only the
    forward runs and nothing is kept. The input checks are ``LPIPS.forward``'s (``HcfError``). See the module docstring for the
    math, the zero-norm convention and the max-pool tie rule."""

    REDUCTIONS = ("mean", "sum", "none")

    def __init__(self, metric: LPIPS, reduction: str = "mean"):
        super().__init__()
        if not isinstance(metric, LPIPS):
            raise TypeError("LPIPSLoss: metric must be a hcflow_amd.lpips.LPIPS, got %s" % type(metric).__name__)
        if reduction not in self.REDUCTIONS:
            raise ValueError("LPIPSLoss: reduction must be one of %s, got %r" % (self.REDUCTIONS, reduction))
        self.metric = metric
        self.reduction = reduction

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False):
        d = _LPIPSLossFn.apply(in0, in1, _checked_params(self.metric, in0, in1, loss=True), normalize)
        if self.reduction == "mean":
            return d.mean()
        if self.reduction == "sum":
            return d.sum()
        return d


class LPIPSRef:
    """What ``LPIPSMap.embed`` returns: the feature maps of one input in a device buffer (private layout), its shape and its
    ``normalize`` flag, and the parameter tensors the maps were made with."""

    def __init__(self, store, shape, normalize, params):
        self.store, self.shape, self.normalize, self.params = store, tuple(shape), bool(normalize), params


class LPIPSMap(nn.Module):
    """Per-pixel LPIPS and sample-set scores on the kernels of ``metric`` (a ``LPIPS``; no parameters of its own):

        m = LPIPSMap(metric)
        d_map = m(in0, in1, normalize=False)            # [B,1,H,W] fp32: lpips.LPIPS(spatial=True)'s value
        ref = m.embed(gt, normalize=True)               # GT through AlexNet once
        d = m.compare(ref, sr)                          # [B,1,1,1], bit-equal to metric(gt, sr, normalize=True)
        d, d_map = m.compare(ref, sr, spatial=True)
        acc = m.sample_set(gt, normalize=True)
        for sr in samples: acc.add(sr)                  # no host sync; no allocation after the first add
        r = acc.result()                                # lpips, map_mean [M,B]; global_best(_index), local_best, score [B]; best_map

    The input checks are ``LPIPS.forward``'s (``HcfError``). See the module docstring for the definitions."""

    def __init__(self, metric: LPIPS):
        super().__init__()
        if not isinstance(metric, LPIPS):
            raise TypeError("LPIPSMap: metric must be a hcflow_amd.lpips.LPIPS, got %s" % type(metric).__name__)
        self.metric = metric

    def embed(self, x: torch.Tensor, normalize: bool = False) -> LPIPSRef:
        params = _checked_params(self.metric, x, x, loss=False)
        B, _, H, W = x.shape
        need = _lib.load().hcf_lpips_embed_bytes(B, H, W)
        store = torch.empty(need, dtype=torch.uint8, device=x.device)
        xf = x.detach().to(torch.float32).contiguous()
        _lib.launch("hcf_lpips_alex_embed", x.device, xf, B, H, W, int(bool(normalize)), _param_ptrs(params), store, need)
        return LPIPSRef(store, x.shape, normalize, params)

    def _map_call(self, ref: LPIPSRef, x, out, out_map, map_mean, best_map, best_mean, first, work):
        """One ``hcf_lpips_alex_map`` call of ``x`` against ``ref`` (``work``: the call's scratch, or None for a fresh one)."""
        if not isinstance(ref, LPIPSRef):
            raise TypeError("LPIPSMap: ref must come from LPIPSMap.embed, got %s" % type(ref).__name__)
        _checked_params(self.metric, x, x, loss=False)
        if tuple(x.shape) != ref.shape or x.device != ref.store.device:
            raise _lib.HcfError("LPIPSMap: the reference was embedded for %s on %s, got %s on %s"
                                % (ref.shape, ref.store.device, tuple(x.shape), x.device))
        B, _, H, W = x.shape
        need = _lib.load().hcf_lpips_map_workspace(B, H, W)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=x.device)
        xf = x.detach().to(torch.float32).contiguous()
        _lib.launch("hcf_lpips_alex_map", x.device, ref.store, ref.store.numel(), xf, B, H, W, int(ref.normalize),
                    _param_ptrs(ref.params), out, None, out_map, map_mean, best_map, best_mean, int(bool(first)), work, need)
        return work

    def compare(self, ref: LPIPSRef, x: torch.Tensor, spatial: bool = False, normalize: Optional[bool] = None):
        """``metric(gt, x)`` for the embedded ``gt`` as ``[B,1,1,1]``; ``spatial=True``: ``(that, the map [B,1,H,W])``.
        ``normalize`` is the reference's; passing another value is refused."""
        if normalize is not None and isinstance(ref, LPIPSRef) and bool(normalize) != ref.normalize:
            raise _lib.HcfError("LPIPSMap.compare: the reference was embedded with normalize=%s" % ref.normalize)
        B, _, H, W = x.shape if x.dim() == 4 else (0, 0, 0, 0)
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        d_map = torch.empty(B, 1, H, W, dtype=torch.float32, device=x.device) if spatial else None
        self._map_call(ref, x, out, d_map, None, None, None, True, None)
        return (out.view(B, 1, 1, 1), d_map) if spatial else out.view(B, 1, 1, 1)

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False):
        _checked_params(self.metric, in0, in1, loss=False)
        return self.compare(self.embed(in0, normalize), in1, spatial=True)[1]

    def sample_set(self, gt: torch.Tensor, normalize: bool = False, capacity: int = 64) -> "LPIPSSampleSet":
        return LPIPSSampleSet(self, self.embed(gt, normalize), capacity)


class LPIPSSampleSet:
    """The accumulator of ``LPIPSMap.sample_set``. Its buffers (the call's scratch, ``best_map``, ``capacity`` rows of per-sample
    values) are allocated with the set; ``add`` launches one ``hcf_lpips_alex_map`` call into them and does not synchronise. Beyond
    ``capacity`` samples the row buffers double (the one allocation after the first add)."""

    def __init__(self, owner: LPIPSMap, ref: LPIPSRef, capacity: int = 64):
        B, _, H, W = ref.shape
        dev = ref.store.device
        self.owner, self.ref, self.M = owner, ref, 0
        self._rows = torch.empty(2, max(1, int(capacity)), B, dtype=torch.float32, device=dev)      # lpips, map_mean
        self._best_mean = torch.empty(B, dtype=torch.float32, device=dev)
        self._best_map = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
        self._work = torch.empty(_lib.load().hcf_lpips_map_workspace(B, H, W), dtype=torch.uint8, device=dev)

    def add(self, x: torch.Tensor):
        if self.M == self._rows.shape[1]:
            self._rows = torch.cat([self._rows, torch.empty_like(self._rows)], 1)
        m = self.M
        self.owner._map_call(self.ref, x, self._rows[0, m], None, self._rows[1, m], self._best_map, self._best_mean, m == 0,
                             self._work)
        self.M = m + 1
        return self

    def result(self):
        if self.M == 0:
            raise _lib.HcfError("LPIPSSampleSet.result: no sample was added")
        lp, mm = self._rows[0, :self.M].clone(), self._rows[1, :self.M].clone()
        gb, gi = mm.min(dim=0)
        lb = self._best_mean.clone()
        g64, l64 = gb.double(), lb.double()
        score = torch.where(g64 == 0, torch.zeros_like(g64), (g64 - l64) / g64)
        return {"lpips": lp, "map_mean": mm, "global_best": gb, "global_best_index": gi, "local_best": lb,
                "best_map": self._best_map.clone(), "score": score}
