"""Inputs, losses and oracle runs shared by tests/test_encode_train_cpu.py and tests/test_gpu_encode_train.py: the PARAMETER
gradients of the SR encode (z, every eps_l, logp) under the CPU oracle's autograd (tests/encode_oracle.py, oracle/hcflow_oracle.py).

The inputs, the smooth loss and its unequal per-sample weights on logp are tests/input_grad_cases.py's. The comparison is the
per-tensor form of tests/test_gpu_train_full.py::test_full_depth_gradients_match_oracle_autograd: for every parameter tensor
||g - g_ref|| / max(||g_ref||, 1e-6 * gmax), gmax the largest reference norm of the case; the worst tensor is held to the gate.
Every oracle run is made once and never written."""
import functools
import math

import torch

from oracle import hcflow_oracle as O
from tests import encode_oracle as E
from tests import input_grad_cases as K

NETS = ["SR_4X_tiny", "SR_8X_tiny", "SR_4X_tiny_LU"]
GATE = 3e-4
SEEDS = ["all", "logp", "z", "eps"]          # the smooth loss over every output, and one seed at a time


def keys(name):
    from hcflow_amd.config import param_spec
    return [k for k, _, _ in param_spec(K._cfg(name))]


def trainable(name, dtype=torch.float32):
    """a copy of the net's parameters in ``dtype`` with requires_grad on what the reference trains (tests/util.py trainable)"""
    from tests.util import trainable as _trainable
    q = _trainable(K._params(name), K._cfg(name))
    if dtype == torch.float32:
        return q
    return {k: (v.detach().to(dtype).requires_grad_(True) if v.requires_grad else v.detach().to(dtype)) for k, v in q.items()}


def loss_of(which, z, eps, logp):
    """'all': K.smooth_loss over z, every eps_l and logp (unequal sample weights: a B * g in place of sum_b g_b shows);
    'logp' / 'z' / 'eps': that output alone (eps: the shallowest level's, the last of the list)"""
    if which == "all":
        return K.smooth_loss([z] + list(eps), logp)
    if which == "logp":
        return (logp * K.sample_weights(logp.shape[0]).to(logp.device)).sum() / 1000.0
    if which == "z":
        return K.smooth_loss([z])
    assert which == "eps"
    return K.smooth_loss([eps[-1]])


@functools.lru_cache(maxsize=None)
def encode_param_oracle(name, which="all", double=False):
    """{key: d loss / d parameter} of tests.encode_oracle.encode under loss_of(which) on K.inputs(name, 7); a parameter the loss does
    not reach has a zero gradient"""
    dtype = torch.float64 if double else torch.float32
    cfg = K._cfg(name)
    hr, _, _ = K.inputs(name, 7)
    q = trainable(name, dtype)
    torch.set_num_threads(8)
    z, eps, logp = E.encode(hr.to(dtype), q, cfg)
    loss_of(which, z, eps, logp).backward()
    return {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in q.items() if v.requires_grad}


def worst(got, ref):
    """(largest per-tensor relative error, its key, gmax) of {key: gradient} against the reference dict"""
    gmax = max(float(r.double().norm()) for r in ref.values())
    out = (0.0, None)
    for k, r in ref.items():
        g = got[k]
        assert g is not None, "%s: no gradient" % k
        err = float((g.detach().cpu().double() - r.double()).norm()) / max(float(r.double().norm()), 1e-6 * gmax)
        if not err <= out[0]:
            out = (err, k)
    return out[0], out[1], gmax


# ---- the decomposition nll = mean_b( -(logp_b + dirac_b) / (ln 2 * pixels) ) on the CPU
@functools.lru_cache(maxsize=None)
def nll_param_oracle(name, double=False):
    """{key: d nll / d parameter} of O.sr_forward on the NLL inputs (K.inputs(name): clear of Quant's rounding steps)"""
    dtype = torch.float64 if double else torch.float32
    cfg = K._cfg(name)
    hr, lr, noise = K.inputs(name)
    q = trainable(name, dtype)
    torch.set_num_threads(8)
    _, nll = O.sr_forward(hr.to(dtype), lr.to(dtype), q, cfg, noise=noise.to(dtype))
    nll.backward()
    return float(nll.detach()), {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in q.items() if v.requires_grad}


def nll_from_encode(z, logp, lr, pixels):
    """[B]: -(logp + Dirac-LR term at lr with the straight-through Quant) / (ln 2 * pixels), the oracle's blocks"""
    zq = z + (O.quantize(z.detach()) - z).detach()
    dirac = O.gaussian_logp(lr, -torch.ones_like(lr) * 6, zq)
    return -(logp + dirac) / float(math.log(2.0) * pixels)


@functools.lru_cache(maxsize=None)
def nll_decomposed_oracle(name):
    """(mean nll, {key: gradient}) of the decomposition over tests.encode_oracle.encode, fp32, on the NLL inputs"""
    cfg = K._cfg(name)
    hr, lr, noise = K.inputs(name)
    q = trainable(name)
    torch.set_num_threads(8)
    z, _, logp = E.encode(hr, q, cfg, noise=noise)
    nll = nll_from_encode(z, logp, lr, hr.shape[2] * hr.shape[3]).mean()
    nll.backward()
    return float(nll.detach()), {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach() for k, v in q.items() if v.requires_grad}
