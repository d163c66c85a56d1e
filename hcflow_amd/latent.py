"""Latent-space helpers over ``HCFlowNet_SR.encode`` / ``decode`` (and the rescaling net's aliases).

Plain torch on the tensors the engine returns -- a few elementwise operations on < 100 MB, no kernels of their own. ``eps`` is
always the list the inverse pass takes: one [B, C_l, h_l, w_l] tensor per level, deepest level first (config.eps_shapes).
``lr_consistency`` is the one helper that reaches a kernel: the bicubic degradation of ``hcflow_amd.resize``.

The two ``get_*`` functions are the wrapper-level calls the reference's model class names (HCFlow_SR_model.py:328-351:
get_encode_z_and_nll, get_sr_with_z) with working semantics: there they pass keywords HCFlowNet_SR.forward does not take.
"""
import math

import torch

from .config import eps_shapes


def scale(eps, tau):
    """tau * eps per level: the encoded image re-decoded at temperature ``tau`` (tau = 1: the image itself, 0: the prior mean)."""
    return [e * float(tau) for e in eps]


def lerp(eps_a, eps_b, t):
    """Straight line between two latents, per level; exact at t = 0 and t = 1."""
    assert len(eps_a) == len(eps_b)
    return [torch.lerp(a, b, float(t)) for a, b in zip(eps_a, eps_b)]


def slerp(eps_a, eps_b, t):
    """Great-circle interpolation, per SAMPLE over all levels jointly: the angle is the one between a sample's whole latent
    vectors (every level concatenated), so a path between two N(0, I) draws keeps the norm a Gaussian draw has. Samples whose
    two latents are (anti)parallel fall back to ``lerp``. Exact at t = 0 and t = 1, and slerp(a, a, t) = a."""
    assert len(eps_a) == len(eps_b) and len(eps_a) > 0
    t = float(t)
    B = eps_a[0].shape[0]
    dot = sum((a.double() * b.double()).reshape(B, -1).sum(1) for a, b in zip(eps_a, eps_b))
    na = sum((a.double() ** 2).reshape(B, -1).sum(1) for a in eps_a).sqrt()
    nb = sum((b.double() ** 2).reshape(B, -1).sum(1) for b in eps_b).sqrt()
    cos = (dot / (na * nb).clamp_min(1e-300)).clamp(-1.0, 1.0)
    omega = torch.acos(cos)
    so = torch.sin(omega)
    ok = so > 1e-6
    so_ = torch.where(ok, so, torch.ones_like(so))
    ca = torch.sin((1.0 - t) * omega) / so_
    cb = torch.sin(t * omega) / so_
    out = []
    for a, b in zip(eps_a, eps_b):
        shp = (B,) + (1,) * (a.dim() - 1)
        s = (a * ca.to(a.dtype).view(shp) + b * cb.to(a.dtype).view(shp))
        out.append(torch.where(ok.view(shp), s, torch.lerp(a, b, t)))
    return out


def dirac_logp(lq, z_lr):
    """log N(lq; mean = Quant(z_lr), logs = -6) per sample, the Dirac-LR term of the objective (HCFlowNet_SR_arch.py:58-63),
    in float64. Quant (Basic.py:187-191) is evaluated in float32 as the forward pass does."""
    zq = (torch.clamp(z_lr.float(), 0, 1) * 255.).round() / 255.
    d = zq.double() - lq.to(z_lr.device).double()
    return (-0.5 * (-12.0 + d * d * math.exp(12.0) + math.log(2 * math.pi))).sum(dim=[1, 2, 3])


def get_encode_z_and_nll(net, lq, hr, add_gt_noise=True, noise=None):
    """(eps, nll): the latents of ``hr`` and its negative log-likelihood in bits per dimension PER SAMPLE, with the Dirac term
    evaluated at ``lq`` -- the mean of ``nll`` is the number ``net(hr=hr, lr=lq)`` returns for the same noise
    (HCFlowNet_SR_arch.py:63-65). ``noise``: explicit U[0,1) tensor; otherwise drawn when ``add_gt_noise`` (the reference's
    default for this call)."""
    z, eps, logp = net.encode(hr, noise=noise, add_gt_noise=add_gt_noise)
    pixels = int(hr.shape[2]) * int(hr.shape[3])
    objective = logp.double() + dirac_logp(lq, z)
    return eps, (-objective) / (math.log(2.0) * pixels)


def nll_per_sample(net, hr, lq, noise=None, add_gt_noise=True):
    """[B] float64: the negative log-likelihood of ``hr`` given ``lq`` in bits per dimension PER SAMPLE, differentiable -- what
    ``get_encode_z_and_nll`` computes without a graph. It is ``net.encode(..., param_grad=True)``'s ``logp`` (the taped pass when
    a parameter or ``hr`` requires grad) plus the Dirac-LR term at ``lq`` (HCFlowNet_SR_arch.py:58-63) with Quant straight-through (Basic.py:186-195:
    forward the rounded value, backward the identity), so any weighting of the samples -- hard-example weights, importance
    weights, a curriculum -- trains the net: ``(w * nll_per_sample(net, hr, lq)).sum().backward()``. Its mean is the number
    ``net(hr=hr, lr=lq)`` returns for the same noise. ``noise``: explicit U[0,1) tensor; otherwise drawn when ``add_gt_noise``."""
    z, _, logp = net.encode(hr, noise=noise, add_gt_noise=add_gt_noise, param_grad=True)
    zd = z.double()                                   # (Quant itself in float32, as the forward pass evaluates it)
    zq = zd + (((torch.clamp(z, 0, 1) * 255.).round() / 255.).double() - zd).detach()
    d = zq - lq.detach().to(z.device).double()
    dirac = (-0.5 * (-12.0 + d * d * math.exp(12.0) + math.log(2 * math.pi))).sum(dim=[1, 2, 3])
    pixels = int(hr.shape[2]) * int(hr.shape[3])
    return -(logp.double() + dirac) / (math.log(2.0) * pixels)


def get_sr_with_z(net, lq, heat=None, seed=None, eps=None):
    """(sr, eps): ``lq`` super-resolved with the given latents, or -- when ``eps`` is None -- with N(0, heat) draws made here
    (``seed``: a generator of its own; None: torch's global one; ``heat`` None = 1.0), returned so that the call can be repeated or
    edited. Given ``eps`` is used as it is (already at its temperature: ``scale(eps, tau)``)."""
    if eps is None:
        tau = 1.0 if heat is None else float(heat)
        B, _, h, w = lq.shape
        g = None
        if seed is not None:
            g = torch.Generator(device=lq.device).manual_seed(int(seed))
        eps = [torch.randn(s, generator=g, device=lq.device) * tau for s in eps_shapes(net.cfg, B, h, w)]
    sr = net(lr=lq, eps_std=1.0 if heat is None else float(heat), reverse=True, eps=eps)
    return sr, eps


def sample_nll(net, lq, heat, seed=None, eps=None):
    """(sr, eps_or_None, nll): ``lq`` super-resolved at temperature ``heat`` (or with the given ``eps``, used as they are) by
    ``net.sample_with_logp`` -- one inverse pass -- and the sample's negative log-likelihood given ``lq`` in bits per dimension,
    [B] float64: -(logp + Dirac-LR term at ``lq``) / (ln 2 * H * W), the per-sample number of ``get_encode_z_and_nll`` for
    hr = the unclamped sample without dequantisation noise. The flow's LR latent of its own sample is ``lq`` itself, so the Dirac
    term is ``dirac_logp(lq, lq)``. ``sr`` is clamped; ``eps`` comes back as given (None: the device drew them from ``seed``)."""
    sr, logp = net.sample_with_logp(lq, 1.0 if heat is None else heat, eps=eps, seed=seed)
    pixels = int(sr.shape[2]) * int(sr.shape[3])
    objective = logp.double() + dirac_logp(lq, lq.to(logp.device))
    return sr, eps, (-objective) / (math.log(2.0) * pixels)


def lr_consistency(lq, scale, kind="l2", weight=1.0):
    """The degradation's data term of every shipped configuration as a callable on ``hr``: the LR image is the MATLAB-style
    bicubic down-scale of the HR image (``resize.imresize``: utils/imresize.py on the device, differentiable), so

        ``kind="l2"``:  ``weight * mean((imresize(hr, 1 / scale) - lq) ** 2)``
        ``kind="l1"``:  ``weight * mean(abs(imresize(hr, 1 / scale) - lq))``

    ``scale`` is the integer SR factor 2 .. 8. Pass it as ``refine_image(data_loss=...)``, or composed with ``net.decode`` as
    ``optimise(loss_fn=...)``. ``ValueError`` for an illegal scale or kind (here, before any engine call); ``HcfError`` for a
    CPU ``lq`` (no fallback)."""
    from fractions import Fraction
    from . import _lib
    from .resize import imresize, parse_scale
    if isinstance(scale, bool) or not isinstance(scale, int):
        raise ValueError("lr_consistency: scale is the integer SR factor 2..8, got %r" % (scale,))
    down = Fraction(1, parse_scale(scale)[0])
    if kind not in ("l2", "l1"):
        raise ValueError("lr_consistency: kind must be 'l2' or 'l1', got %r" % (kind,))
    if not isinstance(lq, torch.Tensor) or not lq.is_cuda:
        raise _lib.HcfError("lr_consistency: lq must be a GPU tensor (no fallback)")
    lq = lq.detach().float()
    weight = float(weight)

    def data_loss(hr):
        d = imresize(hr, down) - lq
        return weight * (d * d).mean() if kind == "l2" else weight * d.abs().mean()
    return data_loss


def optimise(net, z_lr, eps, loss_fn, steps, lr=0.02, optimise_lr=False, optimizer=None):
    """Gradient descent in the latent space with the weights frozen: ``steps`` iterations of ``loss_fn(net.decode(z_lr, eps))``
    (a scalar) over clones of ``eps`` -- and of ``z_lr`` when ``optimise_lr`` -- with ``torch.optim.Adam(tensors, lr=lr)``, or
    with ``optimizer(tensors)`` when a factory is given. Returns ``(z_lr, eps, losses)``: the moved latents, detached, and the
    loss of every step (evaluated BEFORE that step's update) as floats. The caller's tensors are not written.

    Every parameter of ``net`` has ``requires_grad`` switched off for the duration, so each backward pass is the engine's
    input-gradient-only one (no weight-gradient work at all), and gets its flag back afterwards, also on an error; no parameter
    is written. ``eps`` entries that are None (levels left to the device sampler) stay None and are not optimised. ``decode`` is
    unclamped: a clamp would zero the gradient of every saturated pixel."""
    steps = int(steps)
    assert steps >= 0
    eps_v = [None if e is None else e.detach().clone().float().requires_grad_(True) for e in eps]
    z_v = z_lr.detach().clone().float()
    if optimise_lr:
        z_v.requires_grad_(True)
    moved = [e for e in eps_v if e is not None] + ([z_v] if optimise_lr else [])
    assert moved, "nothing to optimise: every eps entry is None and optimise_lr is off"
    opt = torch.optim.Adam(moved, lr=float(lr)) if optimizer is None else optimizer(moved)
    params = list(net.parameters())
    flags = [p.requires_grad for p in params]
    history = []
    try:
        for p in params:
            p.requires_grad_(False)
        with torch.enable_grad():
            for _ in range(steps):
                opt.zero_grad(set_to_none=True)
                loss = loss_fn(net.decode(z_v, eps_v))
                loss.backward()
                opt.step()
                history.append(loss.detach())
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)
    losses = [float(v) for v in torch.stack(history).cpu()] if history else []
    return z_v.detach(), [None if e is None else e.detach() for e in eps_v], losses


def refine_image(net, hr0, lq, data_loss=None, steps=20, lr=1e-4, weight=1.0, noise=None, optimizer=None):
    """Gradient descent on the IMAGE with the weights frozen: ``steps`` iterations on
    ``weight * nll(hr | lq) + data_loss(hr)`` over a clone of ``hr0``, where ``nll`` is ``net(hr=hr, lr=lq, reverse=False)``'s
    (bits per dimension, HCFlowNet_SR_arch.py:47-67) -- the trained flow as an image prior: MAP restoration
    (``data_loss`` = the degradation's data term), likelihood-guided refinement of an SR sample (``data_loss=None``). With
    ``torch.optim.Adam([hr], lr=lr)``, or ``optimizer([hr])`` when a factory is given. Returns ``(hr, losses, nlls)``: the moved
    image, detached, and the total loss and the NLL of every step (evaluated BEFORE that step's update) as floats. The caller's
    tensors are not written.

    ``noise``: the U[0,1) dequantisation tensor of the NLL (:52); None: drawn once with torch.rand and held for all steps, so that
    every step descends the same function. ``lq`` is an 8-bit image in [0, 1] (values k / 255) in practice: the Dirac-LR term
    (:58-63) is e^12 / 2 * (Quant(z) - lq)^2 per element with a straight-through Quant, so an ``lq`` off that grid contributes a
    constant gradient that no step can reduce. ``lr`` is in image units (one grey level = 1 / 255 = 3.9e-3).

    Every parameter of ``net`` has ``requires_grad`` switched off for the duration, so each backward pass is the engine's
    input-gradient-only one, and gets its flag back afterwards, also on an error; no parameter is written."""
    steps = int(steps)
    assert steps >= 0
    hr = hr0.detach().clone().float().requires_grad_(True)
    lq = lq.detach()
    if noise is None:
        noise = torch.rand(hr.shape, device=hr.device)
    opt = torch.optim.Adam([hr], lr=float(lr)) if optimizer is None else optimizer([hr])
    params = list(net.parameters())
    flags = [p.requires_grad for p in params]
    losses, nlls = [], []
    try:
        for p in params:
            p.requires_grad_(False)
        with torch.enable_grad():
            for _ in range(steps):
                opt.zero_grad(set_to_none=True)
                _, nll = net(hr=hr, lr=lq, reverse=False, noise=noise)
                loss = float(weight) * nll
                if data_loss is not None:
                    loss = loss + data_loss(hr)
                loss.backward()
                opt.step()
                losses.append(loss.detach())
                nlls.append(nll.detach())
    finally:
        for p, f in zip(params, flags):
            p.requires_grad_(f)
    as_floats = lambda h: [float(v) for v in torch.stack(h).cpu()] if h else []
    return hr.detach(), as_floats(losses), as_floats(nlls)
