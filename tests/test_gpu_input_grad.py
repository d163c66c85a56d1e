"""-m gpu: gradients of the forward passes w.r.t. their images (hcf_train_backward_ex, hcf_train_backward_rescale_ex,
hcf_train_encode_sr / hcf_train_backward_encode, the input-gradient-only backward of the forward tapes, input_grad_emit_kernel,
gauss_encode_logp_bwd_kernel, the Dirac backward's lr output, hcflow_amd.latent.refine_image).

References: float64 torch.autograd for the kernels, at the gate tests/test_gpu_train_glue.py uses (elementwise
2e-6 * max(1, |ref|max)); the fp32 CPU oracle (oracle/hcflow_oracle.py sr_forward / flownet_forward, tests/encode_oracle.py) under
torch.autograd for the module, at the project's gate ||g - g_ref|| <= 5e-4 ||g_ref|| per tensor. On these inputs the fp32 oracle sits
2e-7 .. 3e-7 from a float64 run of itself (NLL d/d lr: 3e-8), three orders inside the gate. The NLL inputs keep a margin from Quant's
rounding steps (tests/input_grad_cases.py); the losses are smooth on purpose. Every oracle run is made once and shared. Every test
prints measured error and gate."""
import ctypes as C
import functools
import math

import pytest
import torch

from oracle import hcflow_oracle as O
from tests import input_grad_cases as K
from tests import train_glue_ref as R

pytestmark = pytest.mark.gpu

GATE = 5e-4
HWS = [(5, 7), (16, 16), (20, 24)]          # partial block, exactly one block, two blocks with a ragged last one
CS = [6, 21, 45]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------- 1. the kernels against float64
@functools.lru_cache(maxsize=None)
def _prior_case(C_, H, W, rescale):
    g = torch.Generator().manual_seed(57 + C_ + 100 * H + 1000 * rescale)
    B = 2
    mean = torch.randn(B, C_, H, W, generator=g)
    s = torch.rand(B, C_, H, W, generator=g) * 2 - 1
    a32 = torch.randn(B, C_, H, W, generator=g)
    geps = torch.randn(B, C_, H, W, generator=g)
    glogp = torch.tensor([0.6, -1.7])
    h32 = torch.stack((mean, s), 2).reshape(B, 2 * C_, H, W)             # h[:, 0::2] = mean, h[:, 1::2] = s
    h = h32.double().requires_grad_(True)
    a = a32.double().requires_grad_(True)
    sd = h[:, 1::2]
    logs = 0.318 * torch.atan(2 * sd) if rescale else sd
    eps = (a - h[:, 0::2]) * torch.exp(-logs)
    logp = (-0.5 * (2 * logs + eps * eps + math.log(2 * math.pi))).sum(dim=[1, 2, 3])
    ga, gh = torch.autograd.grad((geps.double() * eps).sum() + (glogp.double() * logp).sum(), [a, h])
    return dict(a=a32, h=h32, geps=geps, glogp=glogp), {"ga": ("v", ga), "gh": ("v", gh)}


@pytest.mark.parametrize("rescale", [0, 1])
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C_", CS)
def test_prior_encode_logp_backward_op(dev, C_, hw, rescale):
    """gauss_encode_logp_bwd_kernel: both seeds at once against float64 autograd; the eps seed alone is gauss_encode_bwd_kernel's
    output bit for bit; a uniform logp seed alone (as a [B] vector and as the scalar) is gauss_logp_bwd_kernel's bit for bit (that
    kernel has the SR form only: rescale = 0)."""
    from hcflow_amd import ops
    k, ref = _prior_case(C_, hw[0], hw[1], rescale)
    a, h, geps, glogp = k["a"].to(dev), k["h"].to(dev), k["geps"].to(dev), k["glogp"].to(dev)
    ga, gh = ops.prior_encode_logp_backward(a, h, geps, glogp, bool(rescale))
    R.check({"ga": ga, "gh": gh}, ref, "prior_encode_logp_backward C=%d %s rescale=%d" % (C_, hw, rescale))
    ga_e, gh_e = ops.prior_encode_logp_backward(a, h, geps, None, bool(rescale), gobj=0.0)
    ga_old, gh_old = ops.prior_backward("encode", a, h, None, geps, bool(rescale))
    assert torch.equal(ga_e, ga_old) and torch.equal(gh_e, gh_old), "eps seed alone differs from gauss_encode_bwd_kernel"
    if not rescale:
        ga_old, gh_old = ops.prior_backward("logp", a, h, None, None, False, 0.6)
        uniform = torch.full((2,), 0.6, device=dev)
        for ga_l, gh_l in (ops.prior_encode_logp_backward(a, h, None, uniform, False),
                           ops.prior_encode_logp_backward(a, h, None, None, False, gobj=0.6)):
            assert torch.equal(ga_l, ga_old) and torch.equal(gh_l, gh_old), "logp seed alone differs from gauss_logp_bwd_kernel"


@pytest.mark.parametrize("haar", [0, 1])
@pytest.mark.parametrize("hw", HWS)
@pytest.mark.parametrize("C_", CS)
def test_input_grad_emit_op(dev, C_, hw, haar):
    """input_grad_emit_kernel is a pure index map (times 1/4 for Haar): bit-exact against unsqueeze2d / the Haar transpose
    (Haar inv / 4, the oracle's sum order) of the same values, also into an output that is only 4-byte aligned (the pair stores)."""
    from hcflow_amd import ops, _lib
    g = torch.Generator().manual_seed(5 + C_ + 10 * hw[0] + haar)
    gz = torch.randn(2, 4 * C_, hw[0], hw[1], generator=g)
    ref = O.haar_inverse(gz) * 0.25 if haar else O.unsqueeze2d(gz)
    got = ops.input_grad(gz.to(dev), bool(haar))
    assert got.shape == ref.shape and torch.equal(got.cpu(), ref)
    buf = torch.full((ref.numel() + 1,), float("nan"), device=dev)       # an odd float offset
    out = buf[1:]
    gzd = gz.to(dev)
    lib = _lib.load()
    _lib.check(lib.hcf_op_input_grad(gzd.data_ptr(), out.data_ptr(), 2, C_, hw[0], hw[1], haar, None), None, "hcf_op_input_grad")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(ref.shape), ref) and bool(torch.isnan(buf[0]))


@functools.lru_cache(maxsize=None)
def _quant_case(H, W):
    """z = (k + u) / 255, integer k in [-20, 275], u uniform in +-0.4 (tests/train_glue_ref.py quant_case): no input near a rounding
    tie, both clamp sides hit."""
    g = torch.Generator().manual_seed(300 + H)
    kk = torch.randint(-20, 276, (2, 3, H, W), generator=g).double()
    u = (torch.rand(2, 3, H, W, generator=g).double() * 2 - 1) * 0.4
    z32 = ((kk + u) / 255).float()
    lr32 = torch.rand(2, 3, H, W, generator=g)
    gz0 = torch.randn(2, 3, H, W, generator=g) * 100
    gobj = -0.45
    z = z32.double().requires_grad_(True)
    lr = lr32.double().requires_grad_(True)
    q = z + ((torch.clamp(z, 0, 1) * 255.).round() / 255. - z).detach()           # Basic.Quant: backward the identity
    logp = O.gaussian_logp(q, torch.full_like(q, -6.0), lr)
    gz, glr = torch.autograd.grad(gobj * logp.sum(), [z, lr])
    return dict(z=z32, lr=lr32, gz0=gz0, gobj=gobj), {"gz": ("v", gz0.double() + gz), "glr": ("v", glr)}


@pytest.mark.parametrize("hw", HWS)
def test_quant_logp_backward_lr_op(dev, hw):
    """The Dirac backward with the lr output: gz and glr against float64 autograd; gz bit-identical to the call without it."""
    from hcflow_amd import ops
    k, ref = _quant_case(*hw)
    gz, glr = ops.quant_logp_backward_lr(k["z"].to(dev), k["lr"].to(dev), k["gobj"], k["gz0"].to(dev))
    R.check({"gz": gz, "glr": glr}, ref, "quant_logp_backward_lr %s" % (hw,))
    assert torch.equal(gz, ops.quant_logp_backward(k["z"].to(dev), k["lr"].to(dev), k["gobj"], k["gz0"].to(dev)))


# ---------------------------------------------------------------- 2. the module against the oracle's autograd
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
    """hcf_train_backward_counts of the forward passes' tape slot."""
    from hcflow_amd import _lib
    eng, _ = net._engine_for(dev)
    _lib.check(eng.lib.hcf_train_select_tape(eng.handle, 0), eng.handle, "hcf_train_select_tape")
    out = (C.c_int64 * 4)()
    _lib.check(eng.lib.hcf_train_backward_counts(eng.handle, out), eng.handle, "hcf_train_backward_counts")
    return [int(v) for v in out]


def _relerr(got, ref):
    got, ref = got.detach().cpu().double(), ref.double()
    return float((got - ref).norm() / ref.norm())


def _check_grad(what, got, ref):
    assert got is not None, "%s: no gradient" % what
    e = _relerr(got, ref)
    print("%s: relative error %.3e, gate %.1e, |g_ref| %.3e" % (what, e, GATE, float(ref.norm())))
    assert e <= GATE, (what, e)


def _close(what, got, ref, tol):
    err = float((got.detach().cpu() - ref).abs().max())
    bound = tol * max(1.0, float(ref.abs().max()))
    print("%s: max |diff| %.3e, bound %.3e" % (what, err, bound))
    assert err <= bound, (what, err, bound)


def _nll_step(net, dev, name, hr_grad=True, lr_grad=True):
    hr, lr, noise = K.inputs(name)
    hr_d, lr_d = hr.to(dev).requires_grad_(hr_grad), lr.to(dev).requires_grad_(lr_grad)
    out_lr, nll = net(hr=hr_d, lr=lr_d, reverse=False, noise=noise.to(dev))
    assert nll.requires_grad, "the NLL carries no graph"
    nll.backward()
    return out_lr.detach(), nll.detach(), hr_d.grad, lr_d.grad


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", sorted(K.NLL_SEEDS))
def test_nll_gradients_wrt_images_match_oracle(dev, name, precision):
    """Frozen weights, eval(): d nll / d hr and d nll / d lr of net(hr=, lr=, noise=) against the oracle's autograd, on inputs clear
    of the Quant rounding steps; the backward pass did no parameter-gradient work."""
    margin = K.rounding_margin(K.raw_lr_latent(name))
    print("%s: rounding margin of the oracle's LR latent %.3e, required %.1e" % (name, margin, K.MARGIN))
    assert margin >= K.MARGIN
    ref_lr, ref_nll, ref_ghr, ref_glr = K.nll_oracle(name)
    net = _net(name, dev, precision)
    out_lr, nll, g_hr, g_lr = _nll_step(net, dev, name)
    err = float((out_lr.cpu() - ref_lr).abs().max())
    print("%s %s out_lr: max |diff| %.3e, bound 1.0e-05" % (name, precision, err))
    assert err <= 1e-5, "a rounding of the LR latent flipped: the gradients are not comparable"
    assert abs(float(nll) - float(ref_nll)) <= 1e-5 * abs(float(ref_nll))
    _check_grad("%s %s d nll/d hr" % (name, precision), g_hr, ref_ghr)
    _check_grad("%s %s d nll/d lr" % (name, precision), g_lr, ref_glr)
    assert _counts(net, dev) == [0, 0, 0, 0]
    assert all(p.grad is None for p in net.parameters())


def _encode_step(net, dev, name, b=K.B, h=K.LR_H, w=K.LR_W):
    hr, _, _ = K.inputs(name, 7, b, h, w)
    hr_d = hr.to(dev).requires_grad_(True)
    z, eps, logp = net.encode(hr_d)
    assert z.requires_grad and logp.requires_grad and all(e.requires_grad for e in eps), "encode's outputs carry no graph"
    K.smooth_loss([z] + list(eps), logp).backward()
    return z, eps, logp, hr_d.grad


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", sorted(K.NLL_SEEDS))
def test_encode_gradient_wrt_hr_matches_oracle(dev, name, precision):
    """Frozen weights: d loss / d hr of a smooth loss over z, every eps_l and logp (unequal per-sample weights) through encode()."""
    ref_z, ref_eps, ref_logp, ref_g = K.encode_oracle(name)
    net = _net(name, dev, precision)
    z, eps, logp, g_hr = _encode_step(net, dev, name)
    _close("%s %s z" % (name, precision), z, ref_z, 1e-4)
    for i, (e, r) in enumerate(zip(eps, ref_eps)):
        _close("%s %s eps[%d]" % (name, precision, i), e, r, 1e-4)
    assert torch.allclose(logp.detach().cpu(), ref_logp, rtol=1e-5, atol=0.0)
    _check_grad("%s %s encode d/d hr" % (name, precision), g_hr, ref_g)
    assert _counts(net, dev) == [0, 0, 0, 0]
    assert all(p.grad is None for p in net.parameters())


def test_encode_gradient_winograd_dgrad_route(dev):
    """B = 1, HR 128 x 128: level 0 of SR_4X_tiny runs at 64 x 64 = the default HCF_DGRAD_WINO_MIN_PIX, so the dense blocks' gather
    data gradients take the Winograd kernels (f16x3). The encode path: it has no rounding term."""
    name = "SR_4X_tiny"
    _, _, _, ref_g = K.encode_oracle(name, 1, 32, 32)
    net = _net(name, dev, "f16x3")
    _, _, _, g_hr = _encode_step(net, dev, name, 1, 32, 32)
    _check_grad("%s 128x128 f16x3 encode d/d hr" % name, g_hr, ref_g)
    assert _counts(net, dev) == [0, 0, 0, 0]


def test_encode_with_trainable_weights_is_refused(dev):
    net = _net("SR_4X_tiny", dev, "f16x3", frozen=False)
    hr, _, _ = K.inputs("SR_4X_tiny", 7)
    with pytest.raises(NotImplementedError, match="weights frozen"):
        net.encode(hr.to(dev).requires_grad_(True))
    assert not net.encode(hr.to(dev))[0].requires_grad                  # a plain hr: the inference path, as before


def test_encode_backward_refuses_a_gradient_buffer(dev):
    """hcf_train_backward_encode is input-gradient-only by definition: a parameter-gradient buffer is refused with
    HCF_ERR_UNSUPPORTED and a message, before anything runs -- the tape then still serves the real backward."""
    net = _net("SR_4X_tiny", dev, "f16x3")
    hr, _, _ = K.inputs("SR_4X_tiny", 7)
    hr_d = hr.to(dev).requires_grad_(True)
    z, eps, logp = net.encode(hr_d)
    eng, _ = net._engine_for(dev)
    total = sum(p.numel() for p in net._params())
    flat, g_hr = torch.empty(total, device=dev), torch.empty_like(hr_d)
    assert eng.lib.hcf_train_backward_encode(eng.handle, None, None, 0, None, flat.data_ptr(), total, g_hr.data_ptr(), None) == -6
    assert b"per-sample" in eng.lib.hcf_last_error(eng.handle)
    K.smooth_loss([z] + list(eps), logp).backward()
    _check_grad("encode d/d hr after the refusal", hr_d.grad, K.encode_oracle("SR_4X_tiny")[3])


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
def test_rescaling_forward_gradient_wrt_hr_matches_oracle(dev, precision):
    """Frozen weights: d loss / d hr of a smooth loss over (LR unclamped, z1, z2) of the rescaling net's forward pass (Haar input
    end), through normal_flow_diracLR(clamp=False) and through encode()."""
    name = "Rescaling_4X_tiny"
    ref_lr, ref_z1, ref_z2, ref_g = K.rescale_oracle(name)
    net = _net(name, dev, precision)
    hr, _, _ = K.inputs(name, 7)
    hr_d = hr.to(dev).requires_grad_(True)
    out_lr, z1, z2 = net.normal_flow_diracLR(hr_d, clamp=False)
    assert out_lr.requires_grad
    for nm, got, ref in (("lr", out_lr, ref_lr), ("z1", z1, ref_z1), ("z2", z2, ref_z2)):
        _close("%s %s %s" % (name, precision, nm), got, ref, 1e-4)
    K.smooth_loss([out_lr, z1, z2]).backward()
    _check_grad("%s %s forward d/d hr" % (name, precision), hr_d.grad, ref_g)
    assert _counts(net, dev) == [0, 0, 0, 0]
    hr_e = hr.to(dev).requires_grad_(True)
    lr_raw, (e2, e1) = net.encode(hr_e)
    K.smooth_loss([lr_raw, e1, e2]).backward()
    assert torch.equal(hr_e.grad, hr_d.grad)


# ---------------------------------------------------------------- 3. beside the parameter gradients; the paths that must not move
@pytest.mark.parametrize("precision", ["exact", "f16x3"])
def test_full_backward_unchanged_and_hr_gradient_beside_it(dev, precision):
    """Trainable weights (train(), ActNorms inited): one NLL step that also asks for d/d hr gives parameter gradients bit-identical
    to a step that does not, counts its parameter-gradient work, and its d/d hr is bit-identical to the input-gradient-only pass."""
    name = "SR_4X_tiny"
    net = _net(name, dev, precision, train=True, frozen=False)
    grads, ghr = [], None
    for with_hr in (False, True):
        net.zero_grad(set_to_none=True)
        _, _, g_hr, g_lr = _nll_step(net, dev, name, hr_grad=with_hr, lr_grad=False)
        counts = _counts(net, dev)
        print("hr.requires_grad=%s: counts %s" % (with_hr, counts))
        assert counts[0] > 0 and counts[2] > 0 and counts[3] > 0
        assert g_lr is None and (g_hr is not None) == with_hr
        grads.append([None if p.grad is None else p.grad.clone() for p in net.parameters()])
        ghr = g_hr
    assert any(g is not None and float(g.abs().max()) > 0 for g in grads[0])
    for a, b in zip(*grads):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    for p in net.parameters():
        p.requires_grad_(False)
    net.zero_grad(set_to_none=True)
    _, _, g_only, _ = _nll_step(net, dev, name, hr_grad=True, lr_grad=False)
    assert _counts(net, dev) == [0, 0, 0, 0]
    assert torch.equal(g_only, ghr), "d/d hr of the full pass differs from the input-gradient-only pass"
    _check_grad("%s %s train() d nll/d hr" % (name, precision), g_only, K.nll_oracle(name)[2])


def test_two_phase_backward_keeps_refusing_a_null_gradient_buffer(dev):
    from hcflow_amd import _lib
    name = "SR_4X_tiny"
    net = _net(name, dev, "f16x3", train=True)
    hr, lr, noise = K.inputs(name)
    out_lr, nll = net(hr=hr.to(dev).requires_grad_(True), lr=lr.to(dev), reverse=False, noise=noise.to(dev))
    eng, _ = net._engine_for(dev)
    assert eng.lib.hcf_train_backward_phase(eng.handle, 0, 1.0, None, 0, None) == -1
    nll.backward()                                                        # the tape is still good for the whole pass


@pytest.mark.parametrize("name", ["SR_4X_tiny", "Rescaling_4X_tiny"])
def test_inference_path_is_untouched(dev, name):
    """Under no_grad -- also with an hr that requires grad -- the calls return what they returned before any taped pass on the same
    module, bit for bit, carry no graph, and no parameter is written."""
    net = _net(name, dev, "f16x3")
    hr, lr, noise = K.inputs(name)
    hr_d, lr_d, noise_d = hr.to(dev), lr.to(dev), noise.to(dev)
    before = [p.detach().clone() for p in net.parameters()]

    def infer(x):
        with torch.no_grad():
            if net.cfg.sr:
                out = list(net(hr=x, lr=lr_d, reverse=False, noise=noise_d))
                z, eps, logp = net.encode(x)
                out += [z, logp] + list(eps)
            else:
                out = list(net(hr=x, reverse=False))
                lr_raw, e = net.encode(x)
                out += [lr_raw] + list(e)
        return out

    first = infer(hr_d)
    assert not any(t.requires_grad for t in first)
    assert not any(t.requires_grad for t in (net(hr=hr_d, lr=lr_d, reverse=False, noise=noise_d) if net.cfg.sr else net(hr=hr_d)))
    x = hr_d.clone().requires_grad_(True)
    if net.cfg.sr:
        net(hr=x, lr=lr_d, reverse=False, noise=noise_d)[1].backward()
        z, eps, logp = net.encode(x)
        K.smooth_loss([z] + list(eps), logp).backward()
    else:
        K.smooth_loss(list(net(hr=x, reverse=False))).backward()
    assert x.grad is not None
    for a, b in zip(first, infer(x)):
        assert not b.requires_grad and torch.equal(a, b)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))


def test_refine_image_lowers_the_nll_of_a_decoded_sample(dev):
    """latent.refine_image on SR_4X_tiny: a sample decoded from an 8-bit LR image, 20 steps with data_loss=None. The NLL ends below
    its start; no parameter moves and every requires_grad flag is back."""
    from hcflow_amd import latent
    name = "SR_4X_tiny"
    net = _net(name, dev, "f16x3", frozen=False)
    g = torch.Generator().manual_seed(5)
    lq = ((torch.rand(2, 3, 10, 12, generator=g) * 255).round() / 255).to(dev)
    eps = [e.to(dev) for e in O.draw_eps(net.cfg, 2, 10, 12, 0.8, 3)]
    with torch.no_grad():
        hr0 = net.decode(lq, eps)
    hr0_c = hr0.clone()
    before = [p.detach().clone() for p in net.parameters()]
    flags = [p.requires_grad for p in net.parameters()]
    flags[0] = False
    next(net.parameters()).requires_grad_(False)                     # a mixed set of flags to restore
    torch.manual_seed(1)
    hr, losses, nlls = latent.refine_image(net, hr0, lq, steps=20)
    print("nll:", " ".join("%.4f" % v for v in nlls))
    assert len(nlls) == 20 and losses == nlls
    assert nlls[-1] < nlls[0], nlls
    assert _counts(net, dev) == [0, 0, 0, 0]
    assert torch.equal(hr0, hr0_c) and not hr.requires_grad and not torch.equal(hr, hr0)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    assert [p.requires_grad for p in net.parameters()] == flags
    assert all(p.grad is None for p in net.parameters())
