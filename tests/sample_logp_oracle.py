"""CPU restatement of sampling WITH the density (hcf_inverse_logp, HCFlowNet_SR.sample_with_logp) from the oracle's own blocks.

The walk is ``O.flownet_inverse``'s (FlowNet_SR_x4.py:106-123, FlowNet_SR_x8.py:121-144); beside the image it returns the closed
form the engine computes on the way:

    logp = -ln(quant) H W                                                      (HCFlowNet_SR_arch.py:53)
         + sum over levels of -0.5 (2 logs + eps^2 + ln 2pi)                    the prior term of the eps USED, temperature 1
         + sum over the affine couplings of sum(logscale)                       evaluated on the inverse path (same z1 as forward)
         + sum over the flow steps of (sum(actnorm logs) + slogdet W) * pixels  the data-independent terms

The DEFINITION it is held to is ``encode_oracle.encode(x_unclamped, noise=None)``'s ``logp``. ``oracle/`` is not edited.

Precision: the oracle's inverse pass runs in float32 only (``O.invconv_inverse`` rounds W^-1 to float32 as the reference does,
Permutations.py:72-74), so the image and every term are evaluated in float32 by the oracle's own blocks, bit for bit what
``O.sr_inverse`` computes; the terms are then added up in float64. The encode it is compared with runs in float64 throughout
(``widen``).
"""
import numpy as np
import torch

from oracle import hcflow_oracle as O

LOG2PI = float(np.log(2 * np.pi))


def widen(p):
    """The parameter dict in float64: the widest precision the oracle's blocks run in."""
    return {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}


def _step_inverse(z, u, p, pre, perm, kind, nn_module, lr_vs_others=True):
    """O.flowstep_inverse that also returns the step's FORWARD log-det per sample: the coupling's sum of logscale as evaluated here
    (None for an additive step) plus the ActNorm / invertible-conv constants (FlowStep.py:40-51)."""
    pix = z.shape[2] * z.shape[3]
    z, sl = O.coupling(z, u, p, pre + ".affine", kind, nn_module, lr_vs_others, reverse=True)
    ld = O.actnorm_logdet(p[pre + ".actnorm.logs"], pix)
    if perm == "invconv" and (pre + ".permute.l") in p:
        Wi, _ = O.invconv_lu_weight(p, pre + ".permute", reverse=True)
        _, sum_log_s = O.invconv_lu_weight(p, pre + ".permute", reverse=False)
        z = O.invconv_forward(z, Wi)
        ld = ld + sum_log_s * pix
    elif perm == "invconv":
        Wm = p[pre + ".permute.weight"]
        z = O.invconv_inverse(z, Wm)
        ld = ld + O.invconv_logdet(Wm, pix)
    ld = ld.double()
    if sl is not None:
        ld = ld + sl.double()
    return O.actnorm_inverse(z, p[pre + ".actnorm.bias"], p[pre + ".actnorm.logs"]), ld


def inverse_with_logp(lr, p, cfg, eps):
    """(x [B,3,H,W] unclamped, logp [B] float64) for the given ``eps`` (one tensor per level, deepest first, used as they are)."""
    assert cfg.sr
    B, _, h, w = lr.shape
    plan, after = O._plan_from_state(p, cfg)
    L = sum(1 for e in plan if e["type"] == "split")
    logp = torch.zeros(B, dtype=torch.float64) + float(-np.log(cfg.quant) * (h * cfg.scale) * (w * cfg.scale))
    cfs, draw, z = {}, 0, lr
    for ent in reversed(plan):
        pre = "flow.layers.%d" % ent["idx"]
        if ent["type"] == "flowstep":
            z, ld = _step_inverse(z, None, p, pre, cfg.perm, cfg.coupling, cfg.nn_module, ent["lr_vs_others"])
            logp = logp + ld
        elif ent["type"] == "squeeze":
            z = O.haar_inverse(z) if cfg.squeeze == "haar" else O.unsqueeze2d(z)
        else:
            level = ent["level"]
            u = [z] + [O._up(cfs[l2], 2 ** (l2 - level)) for l2 in range(level + 1, L)]
            u = torch.cat(u, 1) if len(u) > 1 else u[0]
            cpre = "flow.level%d_condFlow" % level
            cf = O.cond_features(u, p, cpre, cfg)
            mean, logs = O.split_cross(O.conv_zeros(cf, p, cpre + ".f"))
            e = eps[draw]
            draw += 1
            logp = logp + O.sum_chw(-0.5 * (logs.double() * 2. + e.double() * e.double() + LOG2PI))
            a = mean + torch.exp(logs) * e
            for k in reversed(range(after[level])):
                a, ld = _step_inverse(a, cf, p, "%s.additional_flow_steps.%d" % (cpre, k), cfg.c_perm, cfg.c_coupling,
                                      cfg.c_nn_module)
                logp = logp + ld
            cfs[level] = cf
            z = torch.cat((z, a), 1)
    return z, logp
