"""-m gpu: the native VGG19 perceptual loss (hcflow_amd/gan.py: PerceptualLoss; kernels in hcflow_amd/csrc/hcf_vgg.hip).
Each kernel against PyTorch on its own (selections bit for bit, arithmetic to the ulp), then the whole loss and its gradient at
fake_H against (a) the composed path F.l1_loss(netF(fake), netF(real).detach()) on the same netF -- the same conv kernels on the
same inputs -- and (b) an fp64 evaluation with stock ops, with the gates of tests/test_gpu_gan.py."""
import copy
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from hcflow_amd import _lib, gan

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23                                            # one unit in the last place of fp32, relative
POOL_SHAPES = [(2, 64, 8, 12), (1, 128, 9, 13), (2, 4, 2, 2), (1, 512, 5, 7)]     # (1, 128, 9, 13), (1, 512, 5, 7): odd both ways


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _from_nhwc(y, Cc):
    return y[..., :Cc].permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------------ the kernels, one by one
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2_is_bit_equal_to_torch(shape):
    B, Cc, H, W = shape
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    xn = gan._nhwc(x)
    y = torch.full((B, H // 2, W // 2, Cc), float("nan"), device="cuda")
    rc = _lib.load().hcf_aux_maxpool2(xn.data_ptr(), Cc, Cc, B, H, W, y.data_ptr(), Cc, _stream())
    assert rc == 0
    assert torch.equal(_from_nhwc(y, Cc), F.max_pool2d(x, 2, 2))


def _pool_act_backward(y, gp, act):
    """hcf_aux_maxpool2_act_backward on NCHW test tensors; the output buffer starts as NaN, so every element must be written."""
    B, Cc, H, W = y.shape
    yn, gn = gan._nhwc(y), gan._nhwc(gp)
    out = torch.full((B, H, W, Cc), float("nan"), device="cuda")
    rc = _lib.load().hcf_aux_maxpool2_act_backward(gn.data_ptr(), Cc, yn.data_ptr(), Cc, Cc, B, H, W, act, out.data_ptr(), Cc,
                                                   _stream())
    assert rc == 0
    return _from_nhwc(out, Cc)


def _pool_act_backward_fp64(y, gp, act):
    """CPU fp64 autograd of F.max_pool2d(y), times (y > 0) for relu. A selection: no arithmetic, so the fp32 result is exact."""
    yd = y.detach().cpu().double().requires_grad_(True)
    F.max_pool2d(yd, 2, 2).backward(gp.detach().cpu().double())
    g = yd.grad * (yd.detach() > 0) if act == 1 else yd.grad
    return g.float()


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool2_act_backward_is_bit_equal_to_fp64_autograd(shape):
    B, Cc, H, W = shape
    gen = torch.Generator().manual_seed(2)
    y = F.relu(torch.randn(shape, generator=gen)).cuda()                  # about half the entries are exact zeros
    gp = torch.randn(B, Cc, H // 2, W // 2, generator=gen).cuda()
    for act in (1, 0):
        assert torch.equal(_pool_act_backward(y, gp, act).cpu(), _pool_act_backward_fp64(y, gp, act)), act


def test_maxpool2_act_backward_sends_ties_to_the_first_maximum():
    gen = torch.Generator().manual_seed(3)
    y = torch.randint(0, 3, (2, 64, 9, 13), generator=gen).float().cuda()  # windows with tied positive maxima, and all-zero windows
    gp = torch.randn(2, 64, 4, 6, generator=gen).cuda()
    for act in (1, 0):
        got, want = _pool_act_backward(y, gp, act).cpu(), _pool_act_backward_fp64(y, gp, act)
        assert torch.equal(got, want), act
    assert not got[:, :, 8, :].any() and not got[:, :, :, 12].any()        # the odd last row and column: written, and zero


@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_backward_is_bit_equal_to_the_conv_nodes_expression(act):
    gen = torch.Generator().manual_seed(4)
    y = torch.randn(2, 9, 13, 64, generator=gen)
    y = torch.where(y > 0.5, torch.zeros_like(y), y).cuda()               # exact zeros among both signs
    g = torch.randn(2, 9, 13, 64, generator=gen).cuda()
    if act == 1:                                                           # _ConvNHWC.backward
        want = g * (y > 0)
    elif act == 2:
        want = g * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, 0.2))
    else:
        want = g.clone()
    lib = _lib.load()
    out = torch.full_like(g, float("nan"))
    assert lib.hcf_aux_act_backward(g.data_ptr(), y.data_ptr(), act, g.numel(), out.data_ptr(), _stream()) == 0
    assert torch.equal(out, want)
    g2 = g.clone()
    assert lib.hcf_aux_act_backward(g2.data_ptr(), y.data_ptr(), act, g2.numel(), g2.data_ptr(), _stream()) == 0     # in place
    assert torch.equal(g2, want)


@pytest.mark.parametrize("shape", [(2, 3, 6, 10), (1, 3, 5, 7)])
def test_input_norm_forward_and_backward(shape):
    """Against fp64 (x - mean) / std and its adjoint g / std, within 2 ulp of fp32 relative: each value takes one subtract and
    one divide (forward), one divide (backward)."""
    B, _, H, W = shape
    lib = _lib.load()
    netF = gan.VGGFeatureExtractor(feature_layer=2, device=torch.device("cuda")).cuda()
    mean, std = netF.mean, netF.std
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(shape, generator=gen).cuda()
    y = torch.full((B, H, W, 4), float("nan"), device="cuda")
    assert lib.hcf_aux_input_norm(x.data_ptr(), mean.data_ptr(), std.data_ptr(), B, H, W, y.data_ptr(), _stream()) == 0
    want = (x.double() - mean.double()) / std.double()
    assert bool(((_from_nhwc(y, 3).double() - want).abs() <= 2 * ULP * want.abs()).all())
    assert not y[..., 3].any()                                             # the padding channel is written 0
    y2 = torch.full((B, H, W, 4), float("nan"), device="cuda")             # use_input_norm=False: the layout change only
    assert lib.hcf_aux_input_norm(x.data_ptr(), None, None, B, H, W, y2.data_ptr(), _stream()) == 0
    assert torch.equal(_from_nhwc(y2, 3), x) and not y2[..., 3].any()
    g = torch.randn(B, H, W, 4, generator=gen).cuda()                      # channel 3 holds garbage on purpose: it has no adjoint
    dx = torch.full(shape, float("nan"), device="cuda")
    assert lib.hcf_aux_input_norm_backward(g.data_ptr(), std.data_ptr(), B, H, W, dx.data_ptr(), _stream()) == 0
    wantg = _from_nhwc(g, 3).double() / std.double()
    assert bool(((dx.double() - wantg).abs() <= 2 * ULP * wantg.abs()).all())
    dx2 = torch.full(shape, float("nan"), device="cuda")
    assert lib.hcf_aux_input_norm_backward(g.data_ptr(), None, B, H, W, dx2.data_ptr(), _stream()) == 0
    assert torch.equal(dx2, _from_nhwc(g, 3))


def _feature_loss(a, b, kind, with_grad=True):
    lib = _lib.load()
    n = a.numel()
    wk = torch.empty(lib.hcf_aux_feature_loss_workspace(n), dtype=torch.uint8, device="cuda")
    loss = torch.full((), float("nan"), device="cuda")
    grad = torch.full_like(a, float("nan")) if with_grad else None
    rc = lib.hcf_aux_feature_loss(a.data_ptr(), b.data_ptr(), n, kind, loss.data_ptr(), None if grad is None else grad.data_ptr(),
                                  C.c_void_p(wk.data_ptr()), wk.numel(), _stream())
    assert rc == 0
    return loss, grad


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 4096, 2 * 512 * 2 * 3 + 4])
def test_feature_loss_value_gradient_and_reproducibility(n, kind):
    gen = torch.Generator().manual_seed(6 + n)
    a = torch.randn(n, generator=gen)
    b = torch.randn(n, generator=gen)
    b[1::3] = a[1::3]                                                      # entries where a == b (none for n = 1)
    a, b = a.cuda(), b.cuda()
    loss, grad = _feature_loss(a, b, kind)
    d = a.double() - b.double()
    want = d.abs().mean() if kind == 0 else (d * d).mean()
    wantg = torch.sign(d) / n if kind == 0 else 2 * d / n
    # fp64 accumulation and one rounding to fp32
    assert abs(float(loss) - float(want)) <= 1e-6 * float(want), (float(loss), float(want))
    assert bool(((grad.double() - wantg).abs() <= ULP * wantg.abs()).all())            # 1 ulp; exactly 0 where a == b
    loss2, grad2 = _feature_loss(a, b, kind)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    loss3, _ = _feature_loss(a, b, kind, with_grad=False)                  # the gradient is optional and changes nothing
    assert torch.equal(loss, loss3)


def test_kernels_past_one_grid_of_work():
    """Every elementwise kernel caps its grid at 2048 blocks of 256 threads and strides over the rest, the criterion at 1024 partial
    blocks of 4096 floats: sizes just past those caps, where a thread takes a second item, against the same references."""
    lib = _lib.load()
    gen = torch.Generator().manual_seed(7)
    shape = (2, 64, 260, 261)                                              # 2 * 130 * 131 windows * 16 float4 columns > 2048 * 256
    x = torch.randn(shape, generator=gen)
    y = F.relu(x).cuda()
    yn = gan._nhwc(y)
    p = torch.full((2, 130, 130, 64), float("nan"), device="cuda")        # 2 * 130 * 130 * 16 items: past the cap as well
    assert lib.hcf_aux_maxpool2(yn.data_ptr(), 64, 64, 2, 260, 261, p.data_ptr(), 64, _stream()) == 0
    assert torch.equal(_from_nhwc(p, 64), F.max_pool2d(y, 2, 2))
    gp = torch.randn(2, 64, 130, 130, generator=gen).cuda()
    assert torch.equal(_pool_act_backward(y, gp, 1).cpu(), _pool_act_backward_fp64(y, gp, 1))
    g = torch.randn(yn.shape, generator=gen).cuda()                        # 8.7 M floats = 2.2 M float4 items
    want = g * (yn > 0)
    assert lib.hcf_aux_act_backward(g.data_ptr(), yn.data_ptr(), 1, g.numel(), g.data_ptr(), _stream()) == 0
    assert torch.equal(g, want)
    img = torch.rand(1, 3, 727, 729, generator=gen).cuda()                 # 530 k pixels > 2048 * 256
    out = torch.full((1, 727, 729, 4), float("nan"), device="cuda")
    assert lib.hcf_aux_input_norm(img.data_ptr(), None, None, 1, 727, 729, out.data_ptr(), _stream()) == 0
    assert torch.equal(_from_nhwc(out, 3), img) and not out[..., 3].any()
    back = torch.full_like(img, float("nan"))
    assert lib.hcf_aux_input_norm_backward(out.data_ptr(), None, 1, 727, 729, back.data_ptr(), _stream()) == 0
    assert torch.equal(back, img)
    n = 1024 * 4096 + 4096 + 3                                             # one block wraps; three floats behind the last float4
    a, b = torch.randn(n, generator=gen).cuda(), torch.randn(n, generator=gen).cuda()
    loss, grad = _feature_loss(a, b, 0)
    d = a.double() - b.double()
    assert abs(float(loss) - float(d.abs().mean())) <= 1e-6 * float(d.abs().mean())
    assert bool(((grad.double() - torch.sign(d) / n).abs() <= ULP / n).all())


# ------------------------------------------------------------------------------------------------ the whole loss
def _make_netF(feature_layer=34, use_input_norm=True, seed=9):
    torch.manual_seed(seed)
    net = gan.VGGFeatureExtractor(feature_layer=feature_layer, use_bn=False, use_input_norm=use_input_norm,
                                  device=torch.device("cuda")).cuda().eval()
    with torch.no_grad():        # variance-preserving weights, as tests/test_gpu_gan.py:98-102
        for m in net.features:
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                m.bias.normal_(0, 0.05)
    return net


SHAPES = [(2, 3, 32, 48), (2, 3, 36, 52)]                                  # (36, 52): the third pool sees 9 x 13
CRITERIA = {"l1": F.l1_loss, "l2": F.mse_loss}


def _images(shape):
    gen = torch.Generator().manual_seed(shape[2])
    return torch.rand(shape, generator=gen).cuda(), torch.rand(shape, generator=gen).cuda()


def _fused(netF, crit, fake, real):
    x = fake.detach().clone().requires_grad_(True)
    loss = gan.PerceptualLoss(netF, criterion=crit)(x, real)
    loss.backward()
    return loss.detach(), x.grad


def _composed(netF, crit, fake, real):
    x = fake.detach().clone().requires_grad_(True)
    loss = CRITERIA[crit](netF(x), netF(real).detach())
    loss.backward()
    return loss.detach(), x.grad


_REF = {}


def _fp64(netF_key, netF, crit, shape):
    """The stock fp64 evaluation, computed once per (net, criterion, shape) and shared by the exact and the f16x3 tests:
    (loss, gradient at fake, max |feature|)."""
    key = (netF_key, crit, shape)
    if key not in _REF:
        fake, real = _images(shape)
        ref = copy.deepcopy(netF).double()
        xd = fake.double().requires_grad_(True)
        fea = ref.features((xd - ref.mean) / ref.std)
        with torch.no_grad():
            fea_real = ref.features((real.double() - ref.mean) / ref.std)
        loss = CRITERIA[crit](fea, fea_real)
        loss.backward()
        _REF[key] = (float(loss.detach()), xd.grad.clone(), float(max(fea.detach().abs().max(), fea_real.abs().max())))
    return _REF[key]


@pytest.fixture(scope="module")
def netF34():
    return _make_netF()


def _check_against_fp64(netF, crit, shape, loss, grad):
    want, wantg, feamax = _fp64("34", netF, crit, shape)
    # the feature gate of tests/test_gpu_gan.py:109 carried to a mean, and its gradient gate (:119: L2, 5e-2, ReLU units flipping)
    print("fp64: loss %.9g want %.9g (gate %.3g); grad err %.3g of %.3g" % (
        float(loss), want, 1e-4 * max(1.0, feamax), float((grad.double() - wantg).norm()), float(wantg.norm())))
    assert abs(float(loss) - want) <= 1e-4 * max(1.0, feamax), (float(loss), want, feamax)
    err = float((grad.double() - wantg).norm())
    assert err <= 5e-2 * float(wantg.norm()), (err, float(wantg.norm()))


def _check_against_composed(netF, crit, fake, real, loss, grad):
    closs, cgrad = _composed(netF, crit, fake, real)
    gmax = float(cgrad.abs().max())
    print("composed: loss %.9g vs %.9g; grad maxdiff %.3g of max %.3g" % (
        float(loss), float(closs), float((grad - cgrad).abs().max()), gmax))
    # the same conv kernels on the same inputs: only the final scale may round differently
    assert abs(float(loss) - float(closs)) <= 1e-6 * abs(float(closs)), (float(loss), float(closs))
    assert float((grad - cgrad).abs().max()) <= 1e-5 * gmax, (float((grad - cgrad).abs().max()), gmax)


@pytest.mark.parametrize("crit", ["l1", "l2"])
@pytest.mark.parametrize("shape", SHAPES)
def test_whole_loss_exact(netF34, shape, crit):
    netF34.set_precision("exact")
    fake, real = _images(shape)
    loss, grad = _fused(netF34, crit, fake, real)
    assert loss.shape == () and grad.shape == fake.shape and bool(torch.isfinite(grad).all())
    _check_against_composed(netF34, crit, fake, real, loss, grad)
    _check_against_fp64(netF34, crit, shape, loss, grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_whole_loss_f16x3(netF34, shape):
    netF34.set_precision("f16x3")
    try:
        fake, real = _images(shape)
        loss, grad = _fused(netF34, "l1", fake, real)
        _check_against_fp64(netF34, "l1", shape, loss, grad)
    finally:
        netF34.set_precision("exact")


def test_f16x3_overflow_is_redone_exactly(netF34, monkeypatch):
    """fake * 1e6 leaves the f16 range: the range flag is raised, both passes are redone at exact precision (four passes instead
    of two) and the result is the exact path's, bit for bit."""
    fake, real = _images(SHAPES[0])
    fake = fake * 1e6
    netF34.set_precision("exact")
    want, wantg = _fused(netF34, "l1", fake, real)
    assert bool(torch.isfinite(want))
    passes = []
    orig = gan._PerceptualLossFn._pass
    monkeypatch.setattr(gan._PerceptualLossFn, "_pass", staticmethod(lambda *a: (passes.append(a[4]), orig(*a))[1]))
    netF34.set_precision("f16x3")
    try:
        loss, grad = _fused(netF34, "l1", fake, real)
        assert passes == [1, 1, 0, 0], passes                              # precision of each pass: speculative, then exact
        assert torch.equal(loss, want) and torch.equal(grad, wantg)
        del passes[:]
        _fused(netF34, "l1", *_images(SHAPES[0]))                          # the flags were cleared: an in-range call is not redone
        assert passes == [1, 1], passes
    finally:
        netF34.set_precision("exact")


@pytest.mark.parametrize("variant", ["no_input_norm", "feature_layer_8"])
def test_variants_match_the_composed_path(variant):
    netF = _make_netF(use_input_norm=False) if variant == "no_input_norm" else _make_netF(feature_layer=8)
    fake, real = _images(SHAPES[0])
    loss, grad = _fused(netF, "l1", fake, real)
    _check_against_composed(netF, "l1", fake, real, loss, grad)


def test_two_identical_calls_are_bit_identical(netF34):
    netF34.set_precision("exact")
    fake, real = _images(SHAPES[1])
    l1, g1 = _fused(netF34, "l1", fake, real)
    l2, g2 = _fused(netF34, "l1", fake, real)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_generator_step_with_the_fused_loss_matches_the_composed_loss():
    """One reverse-path generator step on the tiny SR preset (as tests/test_gpu_gan.py:152): l_fea_w * PerceptualLoss through
    netG's differentiable sampling pass -- every netG gradient finite, global L2 norm as with the composed loss."""
    from hcflow_amd import HCFlowNet_SR, preset, make_params
    cfg = preset("SR_4X_tiny")
    netG = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    netG.load_state_dict(make_params(cfg, 11), strict=True)
    for m in netG.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    netG = netG.cuda().train()
    netG.set_precision("exact")
    netF = _make_netF()
    gen = torch.Generator().manual_seed(1)
    lr = torch.rand(2, 3, 12, 20, generator=gen).cuda()
    real = torch.rand(2, 3, 48, 80, generator=gen).cuda()
    l_fea_w = 5e-2
    cri = gan.PerceptualLoss(netF, criterion="l1")
    norms = []
    for loss_of in (lambda fake: cri(fake, real), lambda fake: F.l1_loss(netF(fake), netF(real).detach())):
        netG.zero_grad(set_to_none=True)
        fake = netG(lr=lr, z=None, u=None, eps_std=0.8, reverse=True, seed=5)
        (l_fea_w * loss_of(fake)).backward()
        grads = [p.grad for p in netG.parameters() if p.grad is not None]
        assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
        norms.append(float(torch.sqrt(sum(g.double().square().sum() for g in grads))))
    print("generator gradient norm: fused %.9g composed %.9g" % tuple(norms))
    assert norms[0] > 0 and abs(norms[0] - norms[1]) <= 1e-4 * norms[1], norms
