"""CPU restatement of the SR encode (HR -> LR latent, eps per level, log-density) composed from the oracle's own blocks.

The walk is ``O.flownet_forward``'s (FlowNet_SR_x4.py:84-101, FlowNet_SR_x8.py:91-116); the one difference sits in the prior loop:
where ``O.condflow_forward`` folds the split half into ``gaussian_logp`` (ConditionalFlow.py:46-57), the standardised value
``eps = (a - mean) * exp(-logs)`` is kept and the log-density is written through it, ``-0.5 (2 logs + eps^2 + ln 2pi)``
(Basic.py:78-94 with (x - mean)^2 / exp(2 logs) = eps^2). ``oracle/`` is not edited.
"""
import math

import numpy as np
import torch

from oracle import hcflow_oracle as O

LOG2PI = float(np.log(2 * np.pi))


def encode(hr, p, cfg, noise=None):
    """(z [B,3,h,w] unquantised, [eps, deepest level first: the order of the inverse pass], logp [B] without the Dirac-LR term)."""
    assert cfg.sr
    B, C, H, W = hr.shape
    x = hr if noise is None else hr + noise / cfg.quant
    logdet = torch.zeros(B, dtype=hr.dtype) + float(-np.log(cfg.quant) * H * W)
    plan, after = O._plan_from_state(p, cfg)
    L = sum(1 for e in plan if e["type"] == "split")
    z, ys, a_s = x, [], []
    for ent in plan:
        pre = "flow.layers.%d" % ent["idx"]
        if ent["type"] == "squeeze":
            z = O.haar_forward(z) if cfg.squeeze == "haar" else O.squeeze2d(z)
        elif ent["type"] == "flowstep":
            z, logdet = O.flowstep_forward(z, None, logdet, p, pre, cfg.perm, cfg.coupling, cfg.nn_module, ent["lr_vs_others"])
        else:
            n = ent["n_split"]
            z, a = z[:, :n], z[:, n:]
            ys.append(z)
            a_s.append(a)
    cfs, eps = {}, []
    for level in reversed(range(L)):
        u = [ys[level]] + [O._up(cfs[l2], 2 ** (l2 - level)) for l2 in range(level + 1, L)]
        u = torch.cat(u, 1) if len(u) > 1 else u[0]
        pre = "flow.level%d_condFlow" % level
        cf = O.cond_features(u, p, pre, cfg)
        a = a_s[level]
        for k in range(after[level]):
            a, logdet = O.flowstep_forward(a, cf, logdet, p, "%s.additional_flow_steps.%d" % (pre, k), cfg.c_perm, cfg.c_coupling,
                                           cfg.c_nn_module)
        mean, logs = O.split_cross(O.conv_zeros(cf, p, pre + ".f"))
        e = (a - mean) * torch.exp(-logs)
        logdet = logdet + O.sum_chw(-0.5 * (logs * 2. + e * e + LOG2PI))
        cfs[level] = cf
        eps.append(e)
    return z, eps, logdet


def decode(z, eps, p, cfg):
    """The oracle's inverse pass fed the encoded latents, unclamped: returns hr + noise / quant."""
    return O.sr_inverse(z, p, cfg, 1.0, eps, clamp=False)


def dirac_logp(lr, z):
    """logp(lr; mean = Quant(z), logs = -6) per sample in float64 (HCFlowNet_SR_arch.py:58-63)."""
    zq = O.quantize(z.detach().cpu().float()).double()
    d = zq - lr.detach().cpu().double()
    return (-0.5 * (-12.0 + d * d / math.exp(-12.0) + LOG2PI)).sum(dim=[1, 2, 3])
