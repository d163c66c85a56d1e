"""Inputs and oracle runs shared by tests/test_input_grad_cpu.py and tests/test_gpu_input_grad.py: the gradients of the forward
passes (NLL, encode, rescaling forward) w.r.t. their images under the fp32 CPU oracle's autograd.

The NLL's Dirac-LR term passes through ``round`` (Basic.Quant), so one flipped rounding between two implementations moves the
gradient by e^12 / 255 per element: the NLL inputs are seeds at which every raw LR-latent value inside (0, 1) stays MARGIN clear of
the rounding steps (k + 1/2) / 255 (measured on the CPU, SR_4X_tiny: a seed with a 3.7e-5 margin puts the fp32 oracle 2e-7 from its
float64 self, one with 1e-8 puts it 3e-4 away). Every oracle run is made once and never written."""
import functools

import torch

from oracle import hcflow_oracle as O

NETS = ["SR_4X_tiny", "SR_8X_tiny", "Rescaling_4X_tiny"]
NLL_SEEDS = {"SR_4X_tiny": 7, "SR_8X_tiny": 45}
MARGIN = 2e-5
B, LR_H, LR_W = 2, 10, 12


def _cfg(name):
    from hcflow_amd.config import preset
    return preset(name)


def _params(name):
    from tests.util import cached_params
    return cached_params(name, 11)


@functools.lru_cache(maxsize=None)
def inputs(name, seed=None, b=B, h=LR_H, w=LR_W):
    """(hr, lr, noise) drawn with torch.rand in that order from one generator; seed None: the net's NLL seed (the rescaling net: 7)."""
    cfg = _cfg(name)
    g = torch.Generator().manual_seed(NLL_SEEDS.get(name, 7) if seed is None else seed)
    hr = torch.rand(b, 3, h * cfg.scale, w * cfg.scale, generator=g)
    lr = torch.rand(b, 3, h, w, generator=g)
    noise = torch.rand(b, 3, h * cfg.scale, w * cfg.scale, generator=g)
    return hr, lr, noise


def rounding_margin(z):
    """smallest distance of a value of z inside (0, 1) from a rounding step (k + 1/2) / 255 of Quant"""
    v = z.detach().double().flatten()
    v = v[(v > 0) & (v < 1)] * 255.0
    return float(((v - torch.floor(v)) - 0.5).abs().min()) / 255.0


@functools.lru_cache(maxsize=None)
def raw_lr_latent(name, seed=None):
    """the oracle's LR latent before Quant for the NLL inputs"""
    cfg, p = _cfg(name), _params(name)
    hr, _, noise = inputs(name, seed)
    with torch.no_grad():
        logdet = torch.zeros(hr.shape[0])
        z, _, _ = O.flownet_forward(hr + noise / cfg.quant, logdet, p, cfg)
    return z


@functools.lru_cache(maxsize=None)
def nll_oracle(name):
    """(out_lr, nll, d nll / d hr, d nll / d lr) of O.sr_forward with the explicit noise"""
    cfg, p = _cfg(name), _params(name)
    hr, lr, noise = inputs(name)
    hr_, lr_ = hr.clone().requires_grad_(True), lr.clone().requires_grad_(True)
    torch.set_num_threads(8)
    out_lr, nll = O.sr_forward(hr_, lr_, p, cfg, noise=noise)
    g_hr, g_lr = torch.autograd.grad(nll, [hr_, lr_])
    return out_lr.detach(), nll.detach(), g_hr, g_lr


def sample_weights(b):
    """unequal per-sample weights of the logp term"""
    return torch.tensor([0.7 + 0.9 * i for i in range(b)])


def _wgt(t, seed):
    return torch.randn(t.shape, generator=torch.Generator().manual_seed(seed))


def smooth_loss(tensors, logp=None):
    """sum over the tensors of <t, w_t> / numel + mean(t^2) / 2 with seeded random w_t (+ <logp, sample weights> / pixels): smooth
    on purpose, every output takes part with a gradient of its own"""
    loss = 0.0
    for i, t in enumerate(tensors):
        loss = loss + (t * _wgt(t, 100 + i).to(t.device)).sum() / t.numel() + 0.5 * (t ** 2).mean()
    if logp is not None:
        loss = loss + (logp * sample_weights(logp.shape[0]).to(logp.device)).sum() / 1000.0
    return loss


@functools.lru_cache(maxsize=None)
def encode_oracle(name, b=B, h=LR_H, w=LR_W):
    """(z, eps, logp, d loss / d hr) of tests.encode_oracle.encode under smooth_loss over z, every eps_l and logp"""
    from tests import encode_oracle as E
    cfg, p = _cfg(name), _params(name)
    hr, _, _ = inputs(name, 7, b, h, w)
    hr_ = hr.clone().requires_grad_(True)
    torch.set_num_threads(8)
    z, eps, logp = E.encode(hr_, p, cfg)
    g_hr, = torch.autograd.grad(smooth_loss([z] + list(eps), logp), [hr_])
    return z.detach(), [e.detach() for e in eps], logp.detach(), g_hr


@functools.lru_cache(maxsize=None)
def rescale_oracle(name="Rescaling_4X_tiny"):
    """(LR unclamped, z1, z2, d loss / d hr) of the rescaling forward (O.rescale_forward's walk, O.flownet_forward, without its
    clamp: the loss is smooth) under smooth_loss over all three"""
    cfg, p = _cfg(name), _params(name)
    hr, _, _ = inputs(name, 7)
    hr_ = hr.clone().requires_grad_(True)
    torch.set_num_threads(8)
    z, _, fz = O.flownet_forward(hr_, None, p, cfg)
    g_hr, = torch.autograd.grad(smooth_loss([z, fz[0], fz[1]]), [hr_])
    return z.detach(), fz[0].detach(), fz[1].detach(), g_hr
