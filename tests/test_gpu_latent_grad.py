"""-m gpu: gradients of the inverse pass w.r.t. its latents with the weights frozen (hcf_train_backward_inverse_ex, the
input-gradient-only backward, gauss_sample_bwd_eps_kernel, hcflow_amd.latent.optimise).

References: float64 torch.autograd of a = mean + e^logs eps for the kernel; the fp32 CPU oracle (oracle/hcflow_oracle.py
sr_inverse / rescale_inverse) under torch.autograd for the module. The module gate is the one
test_reverse_path_gradients_match_reference uses, ||g - g_ref|| <= 5e-4 ||g_ref|| per tensor: on these inputs the fp32 oracle sits
2.1e-7 .. 4.2e-7 from a float64 run of itself, three orders inside it. The loss is smooth on purpose (an L1 loss puts sign flips
into the comparison). Every oracle run is made once per (net, size, clamp) and shared. Every test prints measured error and gate."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import hcflow_oracle as O
from tests import train_glue_ref as R

pytestmark = pytest.mark.gpu

GATE = 5e-4
NETS = ["SR_4X_tiny", "SR_8X_tiny", "Rescaling_4X_tiny"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- 1. the kernel against float64
@functools.lru_cache(maxsize=None)
def _op_case(C_, H, W, rescale):
    g = torch.Generator().manual_seed(31 + C_ + 100 * H + 1000 * rescale)
    B = 2
    mean = torch.randn(B, C_, H, W, generator=g)
    s = torch.rand(B, C_, H, W, generator=g) * 2 - 1
    eps32 = torch.randn(B, C_, H, W, generator=g) * 0.8
    ga = torch.randn(B, C_, H, W, generator=g)
    h32 = torch.stack((mean, s), 2).reshape(B, 2 * C_, H, W)             # h[:, 0::2] = mean, h[:, 1::2] = s
    h = h32.double().requires_grad_(True)
    eps = eps32.double().requires_grad_(True)
    sd = h[:, 1::2]
    logs = 0.318 * torch.atan(2 * sd) if rescale else sd
    a = h[:, 0::2] + torch.exp(logs) * eps
    gh, geps = torch.autograd.grad((ga.double() * a).sum(), [h, eps])
    return dict(a=a.detach().float(), h=h32, ga=ga), {"gh": ("v", gh), "geps": ("v", geps)}


@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("hw", [(5, 7), (16, 16), (20, 24)])          # partial block, exactly one block, two blocks with a partial last
@pytest.mark.parametrize("C_", [6, 21, 45])                           # the latents of the shipped nets; 45 takes the sliced-tile path
def test_prior_sample_backward_op(dev, C_, hw, rescale):
    """gauss_sample_bwd_eps_kernel: gh and geps at the gate tests/test_gpu_train_glue.py applies to hcf_op_prior_backward kind 1
    (elementwise 2e-6 * max(1, |ref|max)); gh bit-identical to gauss_sample_bwd_kernel's, also through the NULL-geps form."""
    from hcflow_amd import ops
    k, ref = _op_case(C_, hw[0], hw[1], rescale)
    a, h, ga = k["a"].to(dev), k["h"].to(dev), k["ga"].to(dev)
    gh, geps = ops.prior_sample_backward(a, h, ga, bool(rescale))
    R.check({"gh": gh, "geps": geps}, ref, "prior_sample_backward C=%d %s rescale=%d" % (C_, hw, rescale))
    _, gh_old = ops.prior_backward("sample", a, h, ga, None, bool(rescale), 1.0)
    assert torch.equal(gh, gh_old), "gh differs from gauss_sample_bwd_kernel's"
    gh_null, none = ops.prior_sample_backward(a, h, ga, bool(rescale), want_geps=False)
    assert none is None and torch.equal(gh_null, gh_old)


# ---------------------------------------------------------------- the module against the oracle's autograd
def _loss(out, w):
    return (out * w).sum() / out.numel() + 0.5 * (out ** 2).mean()


def _inputs(name, B, h, w):
    from hcflow_amd.config import preset
    cfg = preset(name)
    # (this seed: the raw 2 x 10 x 12 output of SR_4X_tiny stays 2.2e-4 clear of the clamp bounds, test_latent_gradients_clamped_output)
    lr = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(13))
    eps = O.draw_eps(cfg, B, h, w, 0.8, 7)
    wgt = torch.randn(B, 3, h * cfg.scale, w * cfg.scale, generator=torch.Generator().manual_seed(9))
    return cfg, lr, eps, wgt


@functools.lru_cache(maxsize=None)
def _oracle(name, B, h, w, clamp):
    """(raw output, d loss / d lr, [d loss / d eps_l]) of the fp32 oracle; computed once, never written."""
    from tests.util import cached_params
    cfg, lr, eps, wgt = _inputs(name, B, h, w)
    p = cached_params(name, 11)
    lr_ = lr.clone().requires_grad_(True)
    eps_ = [e.clone().requires_grad_(True) for e in eps]
    torch.set_num_threads(8)
    fn = O.sr_inverse if cfg.sr else O.rescale_inverse
    out = fn(lr_, p, cfg, 1.0, eps=eps_, clamp=clamp)
    g = torch.autograd.grad(_loss(out, wgt), [lr_] + eps_)
    return out.detach(), g[0], list(g[1:])


def _net(name, dev, precision, train=False, frozen=True):
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling
    from hcflow_amd.config import preset
    from tests.util import cached_params
    cfg = preset(name)
    net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(cached_params(name, 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).set_precision(precision)
    net.train() if train else net.eval()
    if frozen:
        for p in net.parameters():
            p.requires_grad_(False)
    return net


def _counts(net, dev):
    """hcf_train_backward_counts of the inverse pass's tape slot."""
    from hcflow_amd import _lib
    eng, _ = net._engine_for(dev)
    _lib.check(eng.lib.hcf_train_select_tape(eng.handle, 1), eng.handle, "hcf_train_select_tape")
    out = (C.c_int64 * 4)()
    _lib.check(eng.lib.hcf_train_backward_counts(eng.handle, out), eng.handle, "hcf_train_backward_counts")
    return [int(v) for v in out]


def _relerr(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    return float((got - ref).norm() / ref.norm())


def _check_grads(what, lr_g, eps_g, ref_lr, ref_eps):
    bad = []
    for nm, got, ref in [("lr", lr_g, ref_lr)] + [("eps[%d]" % i, g, r) for i, (g, r) in enumerate(zip(eps_g, ref_eps))]:
        if got is None:
            bad.append((nm, "no gradient"))
            continue
        e = _relerr(got, ref)
        print("%s d/d%s: relative error %.3e, gate %.1e, |g_ref| %.3e" % (what, nm, e, GATE, float(ref.norm())))
        if not e <= GATE:
            bad.append((nm, e))
    assert not bad, (what, bad)


def _run(net, dev, lr, eps, wgt, clamp, how="decode"):
    lr_d = lr.to(dev).requires_grad_(True)
    eps_d = [e.to(dev).requires_grad_(True) for e in eps]
    if how == "decode":
        out = net.decode(lr_d, eps_d, clamp=clamp)
    elif how == "forward":
        assert clamp
        out = net(lr=lr_d, z=None, u=None, eps_std=1.0, reverse=True, eps=eps_d)
    else:
        out = net.reverse_flow_diracLR(lr_d, None, None, eps_std=1.0, eps=eps_d, clamp=clamp)
    assert out.requires_grad, "the output carries no graph"
    _loss(out, wgt.to(dev)).backward()
    return out.detach(), lr_d.grad, [e.grad for e in eps_d]


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", NETS)
def test_latent_gradients_match_oracle(dev, name, precision):
    """Frozen weights, eval(): d loss / d lr and d loss / d eps_l of decode() against the oracle's autograd; the backward pass did
    no parameter-gradient work. 10 x 12 LR: maps of 10 x 12 / 20 x 24 / 40 x 48, none a multiple of a tile."""
    cfg, lr, eps, wgt = _inputs(name, 2, 10, 12)
    raw, ref_lr, ref_eps = _oracle(name, 2, 10, 12, False)
    net = _net(name, dev, precision)
    out, g_lr, g_eps = _run(net, dev, lr, eps, wgt, False)
    assert float((out.cpu() - raw).abs().max()) <= 1e-4 * max(1.0, float(raw.abs().max()))
    _check_grads("%s %s" % (name, precision), g_lr, g_eps, ref_lr, ref_eps)
    assert _counts(net, dev) == [0, 0, 0, 0]
    assert all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize("how", ["forward", "reverse_flow_diracLR"])
def test_latent_gradients_through_the_other_entry_points(dev, how):
    """forward(..., reverse=True, eps=...) and reverse_flow_diracLR (both clamped by default) in train() mode, weights frozen."""
    name = "SR_4X_tiny"
    cfg, lr, eps, wgt = _inputs(name, 2, 10, 12)
    _, ref_lr, ref_eps = _oracle(name, 2, 10, 12, True)
    net = _net(name, dev, "f16x3", train=True)
    _, g_lr, g_eps = _run(net, dev, lr, eps, wgt, True, how)
    _check_grads("%s %s" % (name, how), g_lr, g_eps, ref_lr, ref_eps)
    assert _counts(net, dev) == [0, 0, 0, 0]


def test_latent_gradients_winograd_dgrad_route(dev):
    """B = 1, 32 x 32 LR: level 0 of SR_4X_tiny runs at 64 x 64 = the default HCF_DGRAD_WINO_MIN_PIX, so the dense blocks' gather
    data gradients take the Winograd kernels (f16x3), input-gradient-only."""
    name = "SR_4X_tiny"
    cfg, lr, eps, wgt = _inputs(name, 1, 32, 32)
    _, ref_lr, ref_eps = _oracle(name, 1, 32, 32, False)
    net = _net(name, dev, "f16x3")
    _, g_lr, g_eps = _run(net, dev, lr, eps, wgt, False)
    _check_grads("%s 32x32 f16x3" % name, g_lr, g_eps, ref_lr, ref_eps)
    assert _counts(net, dev) == [0, 0, 0, 0]


def test_latent_gradients_clamped_output(dev):
    """clamp=True: about 60 % of the outputs leave [0, 1] with these weights and none lies within 1e-4 of a bound, so the mask is
    exercised and stable. Against the oracle at clamp=True, and against our own clamp=False backward fed g_out * mask."""
    name = "SR_4X_tiny"
    cfg, lr, eps, wgt = _inputs(name, 2, 10, 12)
    raw, _, _ = _oracle(name, 2, 10, 12, False)
    outside = float(((raw < 0) | (raw > 1)).float().mean())
    near = float(torch.minimum(raw.abs(), (raw - 1).abs()).min())
    print("outside [0, 1]: %.1f %%, closest to a bound: %.3e" % (100 * outside, near))
    assert 0.3 < outside < 0.9 and near > 1e-4
    _, ref_lr, ref_eps = _oracle(name, 2, 10, 12, True)
    net = _net(name, dev, "f16x3")
    _, g_lr, g_eps = _run(net, dev, lr, eps, wgt, True)
    _check_grads("%s clamp" % name, g_lr, g_eps, ref_lr, ref_eps)
    # the same through the unclamped pass: torch's clamp hands our backward g_out * (0 <= raw <= 1)
    lr_d = lr.to(dev).requires_grad_(True)
    eps_d = [e.to(dev).requires_grad_(True) for e in eps]
    _loss(torch.clamp(net.decode(lr_d, eps_d, clamp=False), 0, 1), wgt.to(dev)).backward()
    for nm, a, b in [("lr", g_lr, lr_d.grad)] + [("eps[%d]" % i, g, e.grad) for i, (g, e) in enumerate(zip(g_eps, eps_d))]:
        print("clamp inside / outside d/d%s: max |diff| %.3e of max %.3e" % (nm, float((a - b).abs().max()), float(b.abs().max())))
        assert torch.allclose(a, b, rtol=1e-6, atol=0.0), nm


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
def test_full_backward_unchanged_and_eps_gradient_beside_it(dev, precision):
    """Parameters requiring grad (train(), ActNorms inited): the same call with eps plain and with eps.requires_grad_() gives
    bit-identical parameter gradients, the pass counts its parameter-gradient work, and eps.grad comes with it."""
    name = "SR_4X_tiny"
    cfg, lr, eps, wgt = _inputs(name, 2, 10, 12)
    _, ref_lr, ref_eps = _oracle(name, 2, 10, 12, False)
    net = _net(name, dev, precision, train=True, frozen=False)
    grads = []
    for with_eps in (False, True):
        net.zero_grad(set_to_none=True)
        lr_d = lr.to(dev).requires_grad_(True)
        eps_d = [e.to(dev).requires_grad_(with_eps) for e in eps]
        _loss(net.decode(lr_d, eps_d, clamp=False), wgt.to(dev)).backward()
        counts = _counts(net, dev)
        print("eps.requires_grad=%s: counts %s" % (with_eps, counts))
        assert counts[0] > 0 and counts[2] > 0 and sum(counts) > 0
        grads.append([None if p.grad is None else p.grad.clone() for p in net.parameters()])
        if with_eps:
            _check_grads("%s %s full backward" % (name, precision), lr_d.grad, [e.grad for e in eps_d], ref_lr, ref_eps)
        else:
            assert all(e.grad is None for e in eps_d)
    assert any(g is not None and float(g.abs().max()) > 0 for g in grads[0])
    for a, b in zip(*grads):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


def test_device_drawn_eps_has_the_gradient_of_the_same_draws(dev):
    """eps=None, eps_std=0.8 and a fixed seed, lr.requires_grad_(), weights frozen: lr.grad equals the one of the call that is
    handed the device's draws (tests/philox_ref.py) explicitly."""
    from tests import philox_ref
    name, seed, tau = "SR_4X_tiny", 1234, 0.8
    cfg, lr, _, wgt = _inputs(name, 2, 10, 12)
    net = _net(name, dev, "f16x3")
    lr_a = lr.to(dev).requires_grad_(True)
    out_a = net(lr=lr_a, z=None, u=None, eps_std=tau, reverse=True, seed=seed)
    _loss(out_a, wgt.to(dev)).backward()
    assert _counts(net, dev) == [0, 0, 0, 0]
    draws = [torch.from_numpy(e).to(dev) for e in philox_ref.level_eps(cfg, 2, 10, 12, tau, seed)]
    lr_b = lr.to(dev).requires_grad_(True)
    out_b = net(lr=lr_b, z=None, u=None, eps_std=tau, reverse=True, eps=draws)
    _loss(out_b, wgt.to(dev)).backward()
    assert float((out_a - out_b).detach().abs().max()) <= 1e-4
    e = _relerr(lr_a.grad, lr_b.grad.cpu())
    print("device-drawn against explicit eps, d/dlr: relative error %.3e, gate %.1e" % (e, GATE))
    assert e <= GATE


def test_inference_path_is_untouched(dev):
    """Nothing requires grad, or no grad mode: no graph, as before."""
    name = "SR_4X_tiny"
    cfg, lr, eps, _ = _inputs(name, 2, 10, 12)
    net = _net(name, dev, "f16x3")
    assert not net.decode(lr.to(dev), [e.to(dev) for e in eps]).requires_grad
    with torch.no_grad():
        assert not net.decode(lr.to(dev), [e.to(dev).requires_grad_(True) for e in eps]).requires_grad


def test_latent_optimise_recovers_a_perturbed_encoding(dev):
    """latent.optimise on SR_4X_tiny: the encoding of a seeded image, eps perturbed by 0.3 * randn, 20 Adam steps on the MSE to the
    image. The loss falls monotonically over the first and the last third of the history and ends below half its start; no
    parameter moves and every requires_grad flag is back."""
    from hcflow_amd import latent
    net = _net("SR_4X_tiny", dev, "f16x3", frozen=False)
    g = torch.Generator().manual_seed(21)
    hr = torch.rand(2, 3, 40, 48, generator=g).to(dev)
    with torch.no_grad():
        z, eps, _ = net.encode(hr)
    eps_p = [e + 0.3 * torch.randn(e.shape, generator=g).to(dev) for e in eps]
    before = [p.detach().clone() for p in net.parameters()]
    flags = [p.requires_grad for p in net.parameters()]
    flags[0] = False
    next(net.parameters()).requires_grad_(False)                     # a mixed set of flags to restore
    z2, eps2, losses = latent.optimise(net, z, eps_p, lambda out: F.mse_loss(out, hr), 20)
    print("losses:", " ".join("%.4e" % v for v in losses))
    assert len(losses) == 20 and len(eps2) == len(eps_p)
    n = len(losses) // 3
    for part in (losses[:n], losses[-n:]):
        assert all(b < a for a, b in zip(part, part[1:])), losses
    assert losses[-1] < 0.5 * losses[0], losses
    assert torch.equal(z2, z) and not any(e.requires_grad for e in eps2)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    assert [p.requires_grad for p in net.parameters()] == flags
    assert all(p.grad is None for p in net.parameters())
