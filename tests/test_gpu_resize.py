"""GPU checks of the differentiable MATLAB-bicubic resize (hcf_resize.hip, hcflow_amd/resize.py, latent.lr_consistency).

References: the reference's recorded float64 outputs (tests/golden/imresize_float.npz) and the float64 matrix oracle
(tests/resize_oracle.py). Gate of a resize, every element compared: |got - ref64| <= max(8 e32, 2^-23 max|ref64|), e32 = the
largest deviation of the fp32 CPU restatement of the same case from ref64 (the project's 8 x e32 convention). Compositions
(losses, chained nodes) are held to that gate plus the worst-case propagation of their input's error, worked out where used.
Each test prints its measured ratio to the gate."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from hcflow_amd import _lib, latent, resize
from hcflow_amd.resize import imresize, lr_psnr
from tests import resize_oracle as O

pytestmark = pytest.mark.gpu
EPS23 = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "imresize_float.npz"))


def scale_arg(s, up):
    return s if up else Fraction(1, s)


def run_fwd(x32, s, up, dev):
    """x32: numpy / torch fp32 [B, C, H, W] -> numpy float64 of the device result."""
    y = imresize(torch.as_tensor(x32).to(dev), scale_arg(s, up))
    return y.cpu().double().numpy()


def run_bwd(g32, H, W, s, up, dev):
    """The device transpose through autograd: g32 [B, C, Ho, Wo] -> float64 numpy [B, C, H, W]."""
    g = torch.as_tensor(g32).to(dev)
    x = torch.zeros(g.shape[0], g.shape[1], H, W, device=dev, requires_grad=True)
    imresize(x, scale_arg(s, up)).backward(g)
    return x.grad.cpu().double().numpy()


def held(got, ref64, restated32, what):
    bound, e32 = O.gate(ref64, restated32)
    err = float(np.abs(got - ref64).max())
    print("%s: max|err| %.3e  e32 %.3e  gate %.3e  ratio %.3f" % (what, err, e32, bound, err / bound))
    assert got.shape == ref64.shape and np.isfinite(got).all()
    assert err <= bound, (what, err, bound)
    return bound


def col_abs_sum(n, s, up):
    return float(np.abs(O.matrix(n, s, up)).sum(axis=0).max())


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("case", O.CASES, ids=lambda c: O.case_name(*c))
def test_forward_against_the_reference(dev, golden, case):
    H, W, s, up = case
    x, y = golden["x_" + O.case_name(*case)], golden["y_" + O.case_name(*case)]
    got = run_fwd(x.astype(np.float32)[None], s, up, dev)[0]
    held(got, y, O.forward32(x, s, up), "forward " + O.case_name(*case))


@pytest.mark.parametrize("C", [1, 3, 5])
def test_forward_batched_against_the_oracle(dev, C):
    rng = np.random.RandomState(40 + C)
    for H, W, s, up in O.CASES:
        x = rng.random_sample((2, C, H, W)).astype(np.float32)
        held(run_fwd(x, s, up, dev), O.forward(x, s, up), O.forward32(x, s, up), "forward B2 C%d %s" % (C, O.case_name(H, W, s, up)))


def test_forward_large_plane(dev):
    """One 2040 x 1356 plane at 1/4: long rows, 128 x 6 and 32 x 22 tiles, offsets of millions of elements."""
    x = np.random.RandomState(7).random_sample((1, 1, 2040, 1356)).astype(np.float32)
    got = run_fwd(x, 4, 0, dev)
    assert got.shape == (1, 1, 510, 339)
    held(got, O.forward(x, 4, 0), O.forward32(x, 4, 0), "forward 2040x1356 down4")


def offset_view(t, dev):
    """A contiguous copy of ``t`` that starts one float into a larger flat buffer: 4-byte aligned only."""
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


# widths with W % 4 == 0 (the aligned run takes the 16-byte path, the view cannot) and W % 4 != 0, Wo % 4 != 0
VIEW_CASES = [(16, 24, 2, 0), (13, 18, 4, 0), (40, 33, 8, 0), (40, 32, 4, 0), (5, 7, 4, 1), (9, 6, 2, 1), (6, 8, 3, 1)]


@pytest.mark.parametrize("case", VIEW_CASES, ids=lambda c: O.case_name(*c))
def test_views_aligned_to_four_bytes_give_the_same_bits(dev, case):
    H, W, s, up = case
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.rand(2, 3, H, W, generator=g).to(dev)
    sc = scale_arg(s, up)
    y = imresize(x, sc)
    assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
    assert torch.equal(imresize(offset_view(x, dev), sc), y)
    out = offset_view(torch.zeros_like(y), dev)
    assert imresize(x, sc, out=out) is out and torch.equal(out, y)
    # the backward: seed and result on 4-byte aligned storage
    gy = torch.randn(y.shape, generator=g).to(dev)
    xa = x.clone().requires_grad_(True)
    imresize(xa, sc).backward(gy)
    xb = x.clone().requires_grad_(True)
    imresize(xb, sc).backward(offset_view(gy, dev))
    assert torch.equal(xa.grad, xb.grad)


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("case", [(13, 18, 4, 0), (40, 33, 8, 0), (48, 64, 4, 0), (5, 7, 4, 1), (12, 16, 2, 1)], ids=lambda c: O.case_name(*c))
def test_bit_reproducible_and_independent_of_the_batch(dev, case):
    H, W, s, up = case
    g = torch.Generator().manual_seed(11)
    sc = scale_arg(s, up)
    x = torch.rand(3, 3, H, W, generator=g).to(dev)
    y = imresize(x, sc)
    assert torch.equal(imresize(x, sc), y)
    gy = torch.randn(y.shape, generator=g).to(dev)

    def grad(xs, gs):
        xv = xs.clone().requires_grad_(True)
        imresize(xv, sc).backward(gs)
        return xv.grad
    gx = grad(x, gy)
    assert torch.equal(grad(x, gy), gx)
    for b in range(3):
        assert torch.equal(imresize(x[b:b + 1], sc), y[b:b + 1])
        assert torch.equal(grad(x[b:b + 1], gy[b:b + 1]), gx[b:b + 1])


# ---------------------------------------------------------------- backward
@pytest.mark.parametrize("case", O.CASES, ids=lambda c: O.case_name(*c))
def test_backward_against_the_transpose(dev, case):
    H, W, s, up = case
    rng = np.random.RandomState(100 + H)
    g = rng.standard_normal((2, 3, O.out_len(H, s, up), O.out_len(W, s, up))).astype(np.float32)
    got = run_bwd(g, H, W, s, up, dev)
    held(got, O.backward(g, H, W, s, up), O.backward32(g, H, W, s, up), "backward " + O.case_name(*case))
    # <imresize(x), g> == <x, backward(g)>, dot products in float64
    x = rng.random_sample((2, 3, H, W)).astype(np.float32)
    lhs = float((run_fwd(x, s, up, dev) * g.astype(np.float64)).sum())
    rhs = float((x.astype(np.float64) * got).sum())
    print("adjoint %s: %.9e vs %.9e" % (O.case_name(*case), lhs, rhs))
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))


def test_backward_large_plane(dev):
    """The transposed tables at the large plane's lengths (up to 6 entries per index, 128 x 22 tiles)."""
    g = np.random.RandomState(8).standard_normal((1, 1, 510, 339)).astype(np.float32)
    got = run_bwd(g, 2040, 1356, 4, 0, dev)
    held(got, O.backward(g, 2040, 1356, 4, 0), O.backward32(g, 2040, 1356, 4, 0), "backward 2040x1356 down4")


# ---------------------------------------------------------------- autograd
def test_autograd_square_sum(dev):
    """d/dx sum(imresize(x, 1/4)^2) = A^T (2 y) A. Bound: the backward's gate on the exact seed, plus the seed's own error
    (2 x the forward's gate, and the fp32 doubling is exact) carried through the transpose: at most ||A_h||_1 ||A_w||_1 times it."""
    H, W, s, up = 13, 18, 4, 0
    x = np.random.RandomState(21).random_sample((2, 3, H, W)).astype(np.float32)
    xt = torch.as_tensor(x).to(dev).requires_grad_(True)
    y = imresize(xt, 1 / 4)
    assert y.grad_fn is not None
    y.square().sum().backward()
    y64 = O.forward(x, s, up)
    ref = O.backward(2 * y64, H, W, s, up)
    fb, _ = O.gate(y64, O.forward32(x, s, up))
    seed32 = (2 * y64).astype(np.float32)
    bb, _ = O.gate(O.backward(seed32, H, W, s, up), O.backward32(seed32, H, W, s, up))
    bound = bb + col_abs_sum(H, s, up) * col_abs_sum(W, s, up) * (2 * fb + EPS23 * float(np.abs(2 * y64).max()))
    err = float(np.abs(xt.grad.cpu().double().numpy() - ref).max())
    print("autograd square-sum: err %.3e bound %.3e ratio %.3f" % (err, bound, err / bound))
    assert err <= bound


def test_autograd_chain_through_two_nodes(dev):
    """imresize(imresize(x, 4), 1/4): gx = U^T (D^T g). Bound: the up node's gate on the exact inner gradient plus the down
    node's gate carried through U^T (at most ||U_h||_1 ||U_w||_1 times it)."""
    H, W = 6, 9
    rng = np.random.RandomState(22)
    x = rng.random_sample((2, 3, H, W)).astype(np.float32)
    g = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    xt = torch.as_tensor(x).to(dev).requires_grad_(True)
    u = imresize(xt, 4)
    y = imresize(u, 0.25)
    assert tuple(u.shape) == (2, 3, 24, 36) and tuple(y.shape) == (2, 3, H, W)
    assert y.grad_fn is not None and u.grad_fn is not None and y.grad_fn is not u.grad_fn
    y.backward(torch.as_tensor(g).to(dev))
    gu = O.backward(g, 4 * H, 4 * W, 4, 0)
    ref = O.backward(gu, H, W, 4, 1)
    b1, _ = O.gate(gu, O.backward32(g, 4 * H, 4 * W, 4, 0))
    gu32 = gu.astype(np.float32)
    b2, _ = O.gate(O.backward(gu32, H, W, 4, 1), O.backward32(gu32, H, W, 4, 1))
    bound = b2 + col_abs_sum(H, 4, 1) * col_abs_sum(W, 4, 1) * (b1 + EPS23 * float(np.abs(gu).max()))
    err = float(np.abs(xt.grad.cpu().double().numpy() - ref).max())
    print("autograd chain: err %.3e bound %.3e ratio %.3f" % (err, bound, err / bound))
    assert err <= bound
    # the forward of the chain, for the record: down(up(x)) is close to x but not x
    held(y.detach().cpu().double().numpy(), O.forward(O.forward(x, 4, 1), 4, 0), O.forward32(O.forward32(x, 4, 1), 4, 0), "chain forward")


def test_no_graph_without_a_gradient(dev):
    x = torch.rand(1, 3, 8, 12, device=dev)
    assert imresize(x, 0.5).grad_fn is None and not imresize(x, 2).requires_grad
    xr = x.clone().requires_grad_(True)
    with torch.no_grad():
        assert imresize(xr, 0.5).grad_fn is None
    assert imresize(xr, 0.5).grad_fn is not None
    o = torch.empty(1, 3, 4, 6, device=dev)                           # out= under autograd: written in place, still a node
    yo = imresize(xr, 0.5, out=o)
    assert yo.grad_fn is not None and yo.data_ptr() == o.data_ptr() and torch.equal(yo.detach(), imresize(x, 0.5))
    # a non-contiguous input is made contiguous and keeps its autograd link
    base = torch.rand(1, 3, 12, 8, device=dev, requires_grad=True)
    xt = base.transpose(2, 3)
    assert not xt.is_contiguous()
    y = imresize(xt, 0.5)
    assert torch.equal(y, imresize(xt.detach().contiguous(), 0.5))
    y.sum().backward()
    assert base.grad is not None and tuple(base.grad.shape) == (1, 3, 12, 8) and bool(base.grad.abs().sum() > 0)


def test_refusals_on_the_device(dev):
    x = torch.rand(1, 3, 8, 8, device=dev)
    with pytest.raises(_lib.HcfError):
        imresize(x.double(), 0.5)
    with pytest.raises(_lib.HcfError):
        imresize(x.half(), 2)
    with pytest.raises(_lib.HcfError):
        imresize(x[0], 2)
    with pytest.raises(_lib.HcfError):
        imresize(x, 2, out=torch.empty(1, 3, 16, 15, device=dev))
    with pytest.raises(_lib.HcfError):
        imresize(x, 2, out=torch.empty(1, 3, 16, 16))
    with pytest.raises(_lib.HcfError):
        imresize(x, 2, out=torch.empty(1, 3, 16, 16, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError):
        imresize(x, 3.0)


# ---------------------------------------------------------------- lr_consistency, lr_psnr
def _lr_case(seed, H, W, s, dev):
    """hr in [0, 1) and an lq that stays 0.05 .. 0.2 away from its down-scale (|d| has no zero crossing for the l1 gradient)."""
    rng = np.random.RandomState(seed)
    hr = rng.random_sample((2, 3, H, W)).astype(np.float32)
    low = O.forward(hr, s, 0)
    lq = (low + rng.choice([-1.0, 1.0], low.shape) * rng.uniform(0.05, 0.2, low.shape)).astype(np.float32)
    return hr, lq, low


@pytest.mark.parametrize("kind", ["l2", "l1"])
def test_lr_consistency_value_and_gradient(dev, kind):
    """Against the float64 composition. With delta = the forward's gate (the device's error on imresize(hr)), d = low - lq, N its
    size: value  l2: |err| <= w (2 mean|d| delta + delta^2), l1: <= w delta, plus 16 x 2^-24 |loss| for the fp32 subtraction,
    square and torch's tree mean; gradient: the backward's gate on the exact seed plus the seed's error -- l2: (2 w / N) (delta +
    2^-23 max|d|), l1: the seed w sign(d) / N is exact as d keeps its sign -- carried through the transpose (||A_h||_1 ||A_w||_1)."""
    H, W, s, w = 13, 18, 4, 0.7
    hr, lq, low = _lr_case(31, H, W, s, dev)
    fn = latent.lr_consistency(torch.as_tensor(lq).to(dev), s, kind=kind, weight=w)
    ht = torch.as_tensor(hr).to(dev).requires_grad_(True)
    loss = fn(ht)
    loss.backward()
    d = low - lq.astype(np.float64)
    N = d.size
    delta, _ = O.gate(low, O.forward32(hr, s, 0))
    if kind == "l2":
        ref, seed = w * (d * d).mean(), 2 * w * d / N
        vb = w * (2 * np.abs(d).mean() * delta + delta * delta)
        se = (2 * w / N) * (delta + EPS23 * float(np.abs(d).max()))
    else:
        ref, seed = w * np.abs(d).mean(), w * np.sign(d) / N
        vb, se = w * delta, 0.0
    vb += 16 * 2.0 ** -24 * abs(ref)
    seed32 = seed.astype(np.float32)
    gb, _ = O.gate(O.backward(seed32, H, W, s, 0), O.backward32(seed32, H, W, s, 0))
    gb += col_abs_sum(H, s, 0) * col_abs_sum(W, s, 0) * (se + EPS23 * float(np.abs(seed).max()))
    verr = abs(float(loss.detach()) - ref)
    gerr = float(np.abs(ht.grad.cpu().double().numpy() - O.backward(seed, H, W, s, 0)).max())
    print("lr_consistency %s: value err %.3e (bound %.3e, ratio %.3f), grad err %.3e (bound %.3e, ratio %.3f)"
          % (kind, verr, vb, verr / vb, gerr, gb, gerr / gb))
    assert verr <= vb and gerr <= gb


def test_refine_image_with_the_bicubic_data_term(dev):
    """latent.refine_image on SR_4X_tiny from hr0 = imresize(lq, 4) with lr_consistency as its data term: 3 steps run, every loss
    and the result are finite. (No descent is asserted.)"""
    from hcflow_amd import HCFlowNet_SR
    from hcflow_amd.config import preset
    from tests.util import cached_params
    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(cached_params("SR_4X_tiny", 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).eval()
    g = torch.Generator().manual_seed(5)
    lq = ((torch.rand(2, 3, 10, 12, generator=g) * 255).round() / 255).to(dev)
    hr0 = imresize(lq, 4)
    assert tuple(hr0.shape) == (2, 3, 40, 48)
    torch.manual_seed(1)
    hr, losses, nlls = latent.refine_image(net, hr0, lq, data_loss=latent.lr_consistency(lq, 4, weight=10.0), steps=3)
    print("refine_image: losses", losses, "nlls", nlls)
    assert len(losses) == len(nlls) == 3 and all(np.isfinite(v) for v in losses + nlls)
    assert tuple(hr.shape) == (2, 3, 40, 48) and bool(torch.isfinite(hr).all()) and not hr.requires_grad


@pytest.mark.parametrize("case", [(13, 18, 4), (17, 9, 3)], ids=lambda c: "%dx%d_s%d" % c)
def test_lr_psnr(dev, case):
    """Against -10 log10(mean d^2) in float64. |mse err| <= 2 mean|d| delta + delta^2 (delta: the forward's gate), and
    |psnr err| <= (10 / ln 10) |mse err| / (mse - |mse err|)."""
    H, W, s = case
    hr, lq, low = _lr_case(33 + s, H, W, s, dev)
    got = lr_psnr(torch.as_tensor(hr).to(dev), torch.as_tensor(lq).to(dev), s)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,) and got.is_cuda
    d = low - lq.astype(np.float64)
    delta, _ = O.gate(low, O.forward32(hr, s, 0))
    for b in range(2):
        mse = (d[b] ** 2).mean()
        me = 2 * np.abs(d[b]).mean() * delta + delta * delta
        bound = 10 / np.log(10) * me / (mse - me)
        err = abs(float(got[b]) + 10 * np.log10(mse))
        print("lr_psnr %s[%d]: %.6f dB, err %.3e bound %.3e ratio %.3f" % (case, b, float(got[b]), err, bound, err / bound))
        assert err <= bound
    ht = torch.as_tensor(hr).to(dev)
    exact = lr_psnr(ht, imresize(ht, Fraction(1, s)), s)
    assert bool(torch.isinf(exact).all()) and bool((exact > 0).all())
