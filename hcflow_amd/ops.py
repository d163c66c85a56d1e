"""Thin torch wrappers over the per-op C-ABI entry points (include/hcflow.h, ``hcf_op_*``).

Used by the unit parity tests; every function takes CUDA fp32 NCHW tensors and returns a new CUDA
tensor computed by the HIP kernels. No fallback paths. Every call goes through ``_lib.launch``: on the device of its
tensors, on the stream current there.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import torch

from . import _lib


def _dev(t: torch.Tensor) -> torch.Tensor:
    if t.device.type != "cuda":
        raise _lib.HcfError("hcflow_amd ops need CUDA (MI355X) tensors")
    return t.detach().to(torch.float32).contiguous()


def _host(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.detach().to("cpu", torch.float32).contiguous()


ACT = {None: 0, "none": 0, "relu": 1, "lrelu": 2}


def set_precision(mode: str):
    """Numerics of conv2d() below: "exact" (fp32 MFMA) or "f16x3" (split products on f16 MFMA)."""
    _lib.check(_lib.load().hcf_op_set_precision(_lib.Engine.PRECISIONS[mode]), None, "hcf_op_set_precision")


def conv2d(srcs: Sequence[torch.Tensor], weight: torch.Tensor, bias=None, scale=None, act=None,
           ups: Optional[Sequence[int]] = None, res1=None, rs1=0.0, res2=None, rs2=0.0) -> torch.Tensor:
    """act((conv(cat(upsampled srcs), weight) + bias) * scale) [* rs1 + res1] [* rs2 + res2]."""
    srcs = [_dev(s) for s in srcs]
    n = len(srcs)
    ups = list(ups) if ups is not None else [0] * n
    B = srcs[0].shape[0]
    H, W = srcs[0].shape[2] << ups[0], srcs[0].shape[3] << ups[0]
    cout, cin, k, _ = weight.shape
    assert sum(s.shape[1] for s in srcs) == cin
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    cs = (C.c_int32 * n)(*[s.shape[1] for s in srcs])
    us = (C.c_int32 * n)(*ups)
    out = torch.empty(B, cout, H, W, device=srcs[0].device)
    r1 = _dev(res1) if res1 is not None else None
    r2 = _dev(res2) if res2 is not None else None
    _lib.launch("hcf_op_conv2d", out.device, ptrs, cs, us, n, B, H, W, _host(weight), _host(bias), _host(scale), cout, k, ACT[act],
                r1, float(rs1), r2, float(rs2), out)
    return out


def conv2d_backward(srcs: Sequence[torch.Tensor], weight: torch.Tensor, grad_out: torch.Tensor,
                    ups: Optional[Sequence[int]] = None, need_input_grads: bool = True):
    """torch.autograd of ``F.conv2d(cat(upsampled srcs), weight, bias, 1, k // 2)``: returns
    ([d srcs] or None, d weight (CPU), d bias (CPU))."""
    srcs = [_dev(s) for s in srcs]
    g = _dev(grad_out)
    n = len(srcs)
    ups = list(ups) if ups is not None else [0] * n
    B, cout, H, W = g.shape
    co, cin, k, _ = weight.shape
    assert co == cout and sum(s.shape[1] for s in srcs) == cin
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    cs = (C.c_int32 * n)(*[s.shape[1] for s in srcs])
    us = (C.c_int32 * n)(*ups)
    dsrcs = [torch.empty_like(s) for s in srcs] if need_input_grads else None
    dptrs = (C.c_void_p * n)(*([d.data_ptr() for d in dsrcs] if dsrcs else [None] * n))
    dw = torch.empty(cout, cin, k, k, dtype=torch.float32)
    db = torch.empty(cout, dtype=torch.float32)
    _lib.launch("hcf_op_conv2d_backward", g.device, ptrs, cs, us, n, B, H, W, _host(weight), cout, k, g, dptrs, dw, db)
    return dsrcs, dw, db


def squeeze2d(x: torch.Tensor, haar: bool = False) -> torch.Tensor:
    x = _dev(x)
    B, Cc, H, W = x.shape
    out = torch.empty(B, 4 * Cc, H // 2, W // 2, device=x.device)
    _lib.launch("hcf_op_squeeze2d", x.device, x, out, B, Cc, H, W, int(haar))
    return out


def unsqueeze2d(x: torch.Tensor, haar: bool = False) -> torch.Tensor:
    x = _dev(x)
    B, C4, H, W = x.shape
    out = torch.empty(B, C4 // 4, H * 2, W * 2, device=x.device)
    _lib.launch("hcf_op_unsqueeze2d", x.device, x, out, B, C4, H, W, int(haar))
    return out


def step_inverse(z, h, mode: int, ns: int, mat, an_bias, an_logs) -> torch.Tensor:
    z, h = _dev(z), _dev(h)
    B, Cc, H, W = z.shape
    out = torch.empty_like(z)
    _lib.launch("hcf_op_step_inverse", z.device, z, h, out, B, Cc, H, W, h.shape[1], mode, ns,
                _host(mat), _host(an_bias.flatten()), _host(an_logs.flatten()))
    return out


INFO_FIELDS = ("launcher", "status", "ntb", "vec", "up", "fuse2", "tailc", "th", "scaled", "k1", "n16", "grid", "block", "tiles",
               "pre", "range_flag")


def _fused_launch(name, device, info, *args, fields=INFO_FIELDS):
    """_lib.launch of an entry that reports its launch in ``info``; a failure carries the record gathered so far
    (``HcfError.info``) and the entry's status (``HcfError.status``)."""
    try:
        _lib.launch(name, device, *args)
    except _lib.HcfError as e:
        e.info = dict(zip(fields, (int(v) for v in info)))
        e.status = next((k for k, v in _lib.ERR_NAMES.items() if "%s (%d)" % (v, k) in str(e)), None)
        raise
    return dict(zip(fields, (int(v) for v in info)))


def fcn12(srcs: Sequence[torch.Tensor], w1, bias1, scale1, w2, bias2, scale2, pre=None, ups: Optional[Sequence[int]] = None,
          form: int = 0, out: Optional[torch.Tensor] = None):
    """FCN layers 1 + 2 as ONE fused f16x3 launch (include/hcflow.h: hcf_op_fcn12): (out, info). ``form`` 0: the engine's routing
    (persistent kernel first), 1: the direct FUSE2 kernel. ``out``: a [B,64,H,W] tensor to write into (a refused launch leaves it
    untouched)."""
    srcs = [_dev(s) for s in srcs]
    n = len(srcs)
    ups = list(ups) if ups is not None else [0] * n
    B = srcs[0].shape[0]
    H, W = srcs[0].shape[2] << ups[0], srcs[0].shape[3] << ups[0]
    assert tuple(w1.shape) == (64, sum(s.shape[1] for s in srcs), 3, 3) and tuple(w2.shape) == (64, 64, 1, 1)
    ptrs = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
    cs = (C.c_int32 * n)(*[s.shape[1] for s in srcs])
    us = (C.c_int32 * n)(*ups)
    if out is None:
        out = torch.empty(B, 64, H, W, device=srcs[0].device)
    assert tuple(out.shape) == (B, 64, H, W) and out.dtype == torch.float32
    info = (C.c_int32 * 16)()
    p = _dev(pre) if pre is not None else None
    rec = _fused_launch("hcf_op_fcn12", out.device, info, ptrs, cs, us, n, B, H, W, _host(w1), _host(bias1), _host(scale1), _host(w2),
                        _host(bias2), _host(scale2), p, out, int(form), info)
    return out, rec


def conv2d_step_inverse(h2, w3, bias3, scale3, z, mode: int, ns: int, mat, an_bias, an_logs, zpad_n: Optional[int] = None):
    """Conv2dZeros with the inverse flow step in its epilogue as ONE fused f16x3 launch (include/hcflow.h:
    hcf_op_conv2d_step_inverse): (out_z, out_zpad or None, info)."""
    h2, z = _dev(h2), _dev(z)
    B, Cc, H, W = z.shape
    f_out, hid = int(w3.shape[0]), int(w3.shape[1])
    assert h2.shape == (B, hid, H, W) and tuple(w3.shape[2:]) == (3, 3)
    out = torch.empty_like(z)
    zpad = torch.empty(B, 16, H, W, device=z.device) if zpad_n is not None else None
    info = (C.c_int32 * 16)()
    rec = _fused_launch("hcf_op_conv2d_step_inverse", z.device, info, h2, hid, _host(w3), _host(bias3), _host(scale3), f_out, z, Cc,
                        int(mode), int(ns), _host(mat), _host(an_bias.flatten()), _host(an_logs.flatten()), out, zpad,
                        int(zpad_n or 0), B, H, W, info)
    return out, zpad, rec


class View(NamedTuple):
    """Channels [c0, c0 + n) of an NHWC buffer of ``cs`` floats per pixel that starts ``off`` floats into the flat CUDA fp32 tensor
    ``buf`` (include/hcflow.h: hcf_view). The *_views entries below use such windows as they are: nothing is copied or cleared."""
    buf: torch.Tensor
    off: int
    cs: int
    c0: int
    n: int
    up: int = 0


def _views(vs, device):
    """ctypes array of hcf_view for a sequence of View (None stays None: a NULL descriptor)."""
    if vs is None:
        return None
    for v in vs:
        if not (v.buf.is_cuda and v.buf.device == device and v.buf.dtype == torch.float32 and v.buf.is_contiguous()):
            raise _lib.HcfError("a view's buffer must be a contiguous CUDA fp32 tensor on %s" % device)
    return (_lib.hcf_view * len(vs))(*[_lib.hcf_view(v.buf.data_ptr() + 4 * int(v.off), int(v.cs), int(v.c0), int(v.n), int(v.up))
                                      for v in vs])


CONV_VIEWS_FIELDS = ("launcher", "status", "ntb", "vec", "up", "fuse2", "tailc", "th", "scaled", "k1", "n16", "grid", "block", "vec_epi",
                     "strip_w", "range_flag")
WGRAD_VIEWS_FIELDS = ("status", "f16", "taps", "vec", "db", "strip_w", "tpb", "nblk_x")
EPI_VIEWS_FIELDS = ("vec", "blocks")


def conv2d_views(srcs: Sequence[View], B: int, H: int, W: int, weight, bias, scale, act, out: View, res1: Optional[View] = None,
                 rs1: float = 0.0, res2: Optional[View] = None, rs2: float = 0.0, scaled: bool = False):
    """conv2d() on the caller's windows, written into ``out``'s window (include/hcflow.h: hcf_op_conv2d_views): the launch record.
    launcher 0 (exact kernel): ``ntb`` / ``vec`` / ``up`` hold VEC, vec_epi and NT of conv_mfma_kernel."""
    dev = out.buf.device
    k = int(weight.shape[2])
    assert int(weight.shape[0]) == out.n and int(weight.shape[1]) == sum(s.n for s in srcs)
    info = (C.c_int32 * 16)()
    return _fused_launch("hcf_op_conv2d_views", dev, info, _views(srcs, dev), len(srcs), B, H, W, _host(weight),
                         _host(bias), _host(scale), k, ACT[act], _views(None if res1 is None else [res1], dev), float(rs1),
                         _views(None if res2 is None else [res2], dev), float(rs2), _views([out], dev), int(bool(scaled)), info,
                         fields=CONV_VIEWS_FIELDS)


DGRAD_FUSED_FIELDS = CONV_VIEWS_FIELDS + ("rows", "units")


def conv2d_dgrad_fused_views(srcs: Sequence[View], B: int, H: int, W: int, weight, y: View, out: View, sum_pre, fb_max, fb_max2=None,
                             fb_act=None, fb_scale=None, sum_zy=None, want_zy: Optional[bool] = None, zy_mult: float = 1.0):
    """ONE launch of the fused data-gradient form (include/hcflow.h: hcf_op_conv2d_dgrad_fused_views): dL/dpre of the conv that
    produced ``y`` is written into ``out``'s window, its per-channel sums are ADDED to the CUDA tensors ``sum_pre`` / ``sum_zy``
    (``want_zy``, default: whether ``sum_zy`` is given, asks the kernel for the sums of dz * y; without it the row holds zeros)
    and the maxima folded into the one-element CUDA tensors ``fb_max`` / ``fb_max2``. Returns the launch record: CONV_VIEWS_FIELDS,
    then the rows of partial sums reduced and the Winograd unit count."""
    dev = out.buf.device
    k = int(weight.shape[2])
    assert int(weight.shape[0]) == out.n == y.n and int(weight.shape[1]) == sum(s.n for s in srcs)
    for t in (sum_pre, sum_zy, fb_max, fb_max2):
        assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
    assert sum_pre.numel() == out.n and (sum_zy is None or sum_zy.numel() == out.n)
    info = (C.c_int32 * 18)()
    zy = sum_zy is not None if want_zy is None else bool(want_zy)
    return _fused_launch("hcf_op_conv2d_dgrad_fused_views", dev, info, _views(srcs, dev), len(srcs), B, H, W, _host(weight), k,
                         _views([y], dev), ACT[fb_act], _host(fb_scale), int(zy), float(zy_mult), _views([out], dev),
                         sum_pre, sum_zy, fb_max, fb_max2, info, fields=DGRAD_FUSED_FIELDS)


def conv2d_wgrad_views(srcs: Sequence[View], B: int, H: int, W: int, g: View, k: int):
    """(dw on the CPU [g.n, cin, k, k], the plan record) of hcf_op_conv2d_wgrad_views."""
    dev = g.buf.device
    dw = torch.empty(g.n, sum(s.n for s in srcs), k, k, dtype=torch.float32)
    info = (C.c_int32 * 16)()
    rec = _fused_launch("hcf_op_conv2d_wgrad_views", dev, info, _views(srcs, dev), len(srcs), B, H, W,
                        _views([g], dev), k * k, dw, info, fields=WGRAD_VIEWS_FIELDS)
    return dw, rec


def conv_epilogue_backward_views(gy: View, B: int, H: int, W: int, y: Optional[View] = None, scale=None, act=None, rs1=None,
                                 g1: Optional[View] = None, rs2=None, g2: Optional[View] = None, gpre: Optional[View] = None,
                                 sum_pre=None, sum_zy=None, zy_mult: float = 1.0, absmax=None, absmax2=None, carry2=None):
    """hcf_op_conv_epilogue_backward_views: gpre (default: gy, in place) is written, g1 / g2 accumulated in the caller's buffers;
    sum_pre / sum_zy / absmax / absmax2 / carry2 are CUDA tensors or None. Returns the record (vec, blocks)."""
    dev = gy.buf.device
    one = lambda v: _views(None if v is None else [v], dev)
    info = (C.c_int32 * 4)()
    return _fused_launch("hcf_op_conv_epilogue_backward_views", dev, info, one(gy), one(y), _host(scale), ACT[act],
                         int(rs1 is not None), float(rs1 or 0.0), one(g1), int(rs2 is not None), float(rs2 or 0.0), one(g2),
                         one(gy if gpre is None else gpre), sum_pre, sum_zy, float(zy_mult), absmax, absmax2, carry2, B, H, W, info,
                         fields=EPI_VIEWS_FIELDS)


def step_forward_head(z, mat, an_bias, an_logs) -> torch.Tensor:
    z = _dev(z)
    B, Cc, H, W = z.shape
    out = torch.empty_like(z)
    _lib.launch("hcf_op_step_forward_head", z.device, z, out, B, Cc, H, W,
                _host(mat), _host(an_bias.flatten()), _host(an_logs.flatten()))
    return out


def step_forward_couple(z, h, mode: int, ns: int):
    z, h = _dev(z), _dev(h)
    B, Cc, H, W = z.shape
    out = torch.empty_like(z)
    ld = torch.empty(B, device=z.device)
    _lib.launch("hcf_op_step_forward_couple", z.device, z, h, out, ld, B, Cc, H, W, h.shape[1], mode, ns)
    return out, ld


def gauss_logp(h, x) -> torch.Tensor:
    h, x = _dev(h), _dev(x)
    B, Cc, H, W = x.shape
    out = torch.empty(B, device=x.device)
    _lib.launch("hcf_op_gauss_logp", x.device, h, x, out, B, Cc, H, W)
    return out


def gauss_sample(h, eps=None, tau: float = 1.0, seed: int = 0, rescale: bool = False) -> torch.Tensor:
    h = _dev(h)
    B, C2, H, W = h.shape
    out = torch.empty(B, C2 // 2, H, W, device=h.device)
    e = _dev(eps) if eps is not None else None
    _lib.launch("hcf_op_gauss_sample", h.device, h, e, float(tau), int(seed), out, B, C2 // 2, H, W, int(rescale))
    return out


# ---- backward kernels of the training path (hcf_train.hip), one entry per launcher ---------------------------------
def step_forward_backward(gzout, zout, h, za, mode: int, ns: int, mat, an_logs, gobj: float, g_bias=None, g_logs=None):
    """Coupling backward, then head backward, of one forward flow step: (gzin, gh, g_bias, g_logs); the two per-channel
    sums are added to ``g_bias`` / ``g_logs`` when given (zeros otherwise)."""
    gzout, zout, h, za = _dev(gzout), _dev(zout), _dev(h), _dev(za)
    B, Cc, H, W = zout.shape
    gzin, gh = torch.empty_like(zout), torch.empty_like(h)
    gb = torch.zeros(Cc, device=zout.device) if g_bias is None else _dev(g_bias).flatten().clone()
    gl = torch.zeros(Cc, device=zout.device) if g_logs is None else _dev(g_logs).flatten().clone()
    _lib.launch("hcf_op_step_forward_backward", zout.device, gzout, zout, h, za, gzin, gh, gb, gl, B, Cc, H, W, h.shape[1], mode, ns,
                _host(mat), _host(an_logs.flatten()), float(gobj))
    return gzin, gh, gb, gl


def step_inverse_backward(gx, x, zc, h, mode: int, ns: int, mat, an_bias, an_logs, g_bias=None, g_logs=None):
    """Backward of one inverse flow step: (gz, gh, gzc, y, g_bias, g_logs)."""
    gx, x, zc, h = _dev(gx), _dev(x), _dev(zc), _dev(h)
    B, Cc, H, W = x.shape
    gz, gh, gzc, y = torch.empty_like(x), torch.empty_like(h), torch.empty_like(x), torch.empty_like(x)
    gb = torch.zeros(Cc, device=x.device) if g_bias is None else _dev(g_bias).flatten().clone()
    gl = torch.zeros(Cc, device=x.device) if g_logs is None else _dev(g_logs).flatten().clone()
    _lib.launch("hcf_op_step_inverse_backward", x.device, gx, x, zc, h, gz, gh, gzc, y, gb, gl, B, Cc, H, W, h.shape[1], mode, ns,
                _host(mat), _host(an_bias.flatten()), _host(an_logs.flatten()))
    return gz, gh, gzc, y, gb, gl


PRIOR_KIND = {"logp": 0, "sample": 1, "encode": 2}


def prior_backward(kind: str, a, h, ga=None, gz=None, rescale: bool = False, gobj: float = 1.0):
    """Gaussian prior backward: (ga, gh). ``ga`` is the input of kind "sample", ``gz`` (or None) that of "encode"."""
    a, h = _dev(a), _dev(h)
    B, Cc, H, W = a.shape
    ga = _dev(ga).clone() if kind == "sample" else torch.empty_like(a)
    gh = torch.empty_like(h)
    gzd = _dev(gz) if gz is not None else None
    _lib.launch("hcf_op_prior_backward", a.device, PRIOR_KIND[kind], a, h, ga, gh, gzd, B, Cc, H, W, int(rescale), float(gobj))
    return ga, gh


def prior_sample_backward(a, h, ga, rescale: bool = False, want_geps: bool = True):
    """Backward of the prior sample a = mean + e^logs eps given ``ga`` = dL/da: (gh, geps) with geps = dL/d eps (None when
    ``want_geps`` is off: the entry then runs the kernel of ``prior_backward("sample", ...)``)."""
    a, h, ga = _dev(a), _dev(h), _dev(ga)
    B, Cc, H, W = a.shape
    gh = torch.empty_like(h)
    geps = torch.empty_like(a) if want_geps else None
    _lib.launch("hcf_op_prior_sample_backward", a.device, a, h, ga, gh, geps, B, Cc, H, W, int(rescale))
    return gh, geps


def quant_logp_backward(z, lr, gobj: float, gz=None) -> torch.Tensor:
    """gz (zeros when None) + gobj * d logp(lr; Quant(z), logs = -6) / dz with the straight-through Quant."""
    z, lr = _dev(z), _dev(lr)
    B, _, H, W = z.shape
    out = torch.zeros_like(z) if gz is None else _dev(gz).clone()
    _lib.launch("hcf_op_quant_logp_backward", z.device, z, lr, out, B, H, W, float(gobj))
    return out


def quant_logp_backward_lr(z, lr, gobj: float, gz=None):
    """``quant_logp_backward`` that also returns d / d lr = gobj * (Quant(z) - lr) * e^12: (gz, glr)."""
    z, lr = _dev(z), _dev(lr)
    B, _, H, W = z.shape
    out = torch.zeros_like(z) if gz is None else _dev(gz).clone()
    glr = torch.empty_like(lr)
    _lib.launch("hcf_op_quant_logp_backward_lr", z.device, z, lr, out, glr, B, H, W, float(gobj))
    return out, glr


def prior_encode_logp_backward(a, h, geps=None, glogp=None, rescale: bool = False, gobj: float = 0.0):
    """Prior backward of the SR encode (eps = (a - mean) e^-logs is an output and logp joins the log-density): (ga, gh) from the
    seeds ``geps`` = dL/d eps (None: zero) and ``glogp`` = dL/d logp per sample, a [B] tensor (None: the scalar ``gobj``)."""
    a, h = _dev(a), _dev(h)
    B, Cc, H, W = a.shape
    ga, gh = torch.empty_like(a), torch.empty_like(h)
    ge = _dev(geps) if geps is not None else None
    gl = _dev(glogp) if glogp is not None else None
    assert gl is None or gl.numel() == B
    _lib.launch("hcf_op_prior_encode_logp_backward", a.device, a, h, ga, gh, ge, gl, B, Cc, H, W, int(rescale), float(gobj))
    return ga, gh


def input_grad(gz, haar: bool = False) -> torch.Tensor:
    """dL/d hr [B,C,2H,2W] from gz = dL/d z [B,4C,H,W] of z = squeeze2d(hr) (or Haar(hr)): unsqueeze2d(gz), or Haar inv(gz) / 4."""
    gz = _dev(gz)
    B, C4, H, W = gz.shape
    assert C4 % 4 == 0
    out = torch.empty(B, C4 // 4, 2 * H, 2 * W, device=gz.device, dtype=torch.float32)
    _lib.launch("hcf_op_input_grad", gz.device, gz, out, B, C4 // 4, H, W, int(haar))
    return out


GRAD_KIND = {"add": 0, "add_clamp01": 1, "mask_unit_range": 2, "mask_flat": 3}


def output_grad_backward(kind: str, g, z, gz=None) -> torch.Tensor:
    """The gradient kernels of an NCHW (clamped) output on a copy of ``gz`` (include/hcflow.h: hcf_op_output_grad_backward)."""
    z = _dev(z)
    B, Cc, H, W = z.shape
    gd = _dev(g) if g is not None else None
    out = torch.zeros_like(z) if gz is None else _dev(gz).clone()
    _lib.launch("hcf_op_output_grad_backward", z.device, GRAD_KIND[kind], gd, z, out, B, Cc, H, W)
    return out


def conv_epilogue_backward(gy, y=None, scale=None, act=None, rs1=None, g1=None, rs2=None, g2=None, want_pre=True, want_zy=False,
                           zy_mult: float = 1.0, sum_pre=None, sum_zy=None, want_max: int = 0, carry2=None, cs=None, c0: int = 0):
    """Backward of the fused conv epilogue. rs1 / rs2 not None: the forward conv had that residual (its gradient is added to a copy
    of g1 / g2 when given). want_max: 1 absmax, 2 absmax and absmax2 (``carry2``: a float folded into absmax2). The tensors sit
    at channels [c0, c0 + n) of an NHWC buffer of ``cs`` floats per pixel (default: n rounded up to 4).
    Returns a dict: gpre, g1, g2, sum_pre, sum_zy, absmax, absmax2 (None where not asked for)."""
    gy = _dev(gy)
    B, n, H, W = gy.shape
    dev = gy.device
    yd = _dev(y) if y is not None else None
    g1d = _dev(g1).clone() if g1 is not None else None
    g2d = _dev(g2).clone() if g2 is not None else None
    gpre = torch.empty_like(gy)
    sp_ = (torch.zeros(n, device=dev) if sum_pre is None else _dev(sum_pre).clone()) if want_pre else None
    sz_ = (torch.zeros(n, device=dev) if sum_zy is None else _dev(sum_zy).clone()) if want_zy else None
    m1 = torch.zeros(1, device=dev) if want_max >= 1 else None
    m2 = torch.zeros(1, device=dev) if want_max >= 2 else None
    cr = torch.tensor([float(carry2)], device=dev, dtype=torch.float32) if carry2 is not None else None
    cs = ((n + 3) // 4) * 4 if cs is None else cs
    _lib.launch("hcf_op_conv_epilogue_backward", dev, gy, yd, _host(scale), ACT[act], int(rs1 is not None), float(rs1 or 0.0), g1d,
                int(rs2 is not None), float(rs2 or 0.0), g2d, gpre, sp_, sz_, float(zy_mult), m1, m2, cr, B, n, H, W, int(cs), int(c0))
    return {"gpre": gpre, "g1": g1d, "g2": g2d, "sum_pre": sp_, "sum_zy": sz_, "absmax": m1, "absmax2": m2}


def lu_chain(dW, P, L, U, dl, du, dlog_s):
    """(dl, du, dlog_s) + the chain rule of dL/dW into the factors of W = P L U' (copies of the given accumulators)."""
    dW, P, L, U = _dev(dW), _dev(P), _dev(L), _dev(U)
    Cc = dW.shape[0]
    dl, du, ds = _dev(dl).clone(), _dev(du).clone(), _dev(dlog_s).clone()
    _lib.launch("hcf_op_lu_chain", dW.device, dW, P, L, U, dl, du, ds, Cc)
    return dl, du, ds


def seed_sum(g) -> torch.Tensor:
    """sum_b g[b] of a [B] vector as one device float: one block, fixed order, float64 accumulation (hcf_op_seed_sum)."""
    g = _dev(g).reshape(-1)
    out = torch.empty(1, device=g.device, dtype=torch.float32)
    _lib.launch("hcf_op_seed_sum", g.device, g, g.numel(), out)
    return out


def axpy_job(x, y, alpha: float, k_dev=None) -> torch.Tensor:
    """One log-det job of the training backward on a copy of ``y``: y + k * (x if x is not None else 1) with k = ``alpha``, or
    ``alpha * k_dev[0]`` when the one-float device tensor ``k_dev`` is given (hcf_op_axpy_job)."""
    out = _dev(y).clone()
    xd = _dev(x) if x is not None else None
    assert xd is None or xd.numel() == out.numel()
    kd = _dev(k_dev) if k_dev is not None else None
    _lib.launch("hcf_op_axpy_job", out.device, xd, out, out.numel(), float(alpha), kd)
    return out
