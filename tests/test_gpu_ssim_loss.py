"""-m gpu: the SSIM criterion on the device (hcflow_amd/losses.py: ssim, SSIMLoss; hcf_ssim.hip) against the float64 oracle
(tests/ssim_loss_oracle.py, which tests/test_ssim_loss_cpu.py holds to oracle/metrics_oracle.py).

Gates.
  value     |v - ref| <= ulp32(ref) + 1e-13. ulp32(ref) is the one fp32 rounding; 1e-13 is the float64 floor: a map value is a
            ratio of 121-term sums of O(1) terms, each carrying at most 121 * 2^-53 = 1.3e-14.
  gradient  per element |g - ref| <= 2^-23 |ref| + 1e-10 max|ref|. The first term is the one fp32 rounding. The floor: on the
            near-identical inputs fp32 autograd is off by 1.8e-4 of max|g|, an amplification of about 3000 over fp32 epsilon (the
            cancellation in E[x^2] - mu^2 and between the three filtered coefficient maps); the same amplification on float64
            gives about 3e-13, so 1e-10 leaves a margin of 300. Two float64 evaluations of the gradient in different orders
            (the kernel's formula in torch against autograd) differ by 5e-13 of max|g| on these inputs.
Every case prints its largest error as a ratio to its gate before it asserts (run with -s to read them).

Shapes: the smallest at which the kernels can go wrong. The forward tiles the (H-10) x (W-10) map by 16 x 32 positions, the
backward tiles the H x W image by 16 x 32 pixels; each tile edge gets the shapes edge - 1, edge, edge + 1 and edge + 10 (the
halo), beside 11 x 11 (one map value), 11 x 12, 12 x 11, 16 x 27 and 43 x 37; B in {1, 2, 3} and C in {1, 3} are spread over them."""
import functools

import numpy as np
import pytest
import torch

from tests import ssim_loss_oracle as O

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
SHAPES = [(1, 1, 11, 11), (2, 3, 11, 12), (3, 1, 12, 11), (2, 3, 16, 27), (3, 3, 43, 37),
          (1, 3, 15, 31), (2, 1, 16, 32), (1, 3, 17, 33), (3, 1, 26, 42),      # backward: 16 x 32 pixels -1, 0, +1, +10
          (3, 1, 25, 41), (2, 1, 27, 43), (2, 3, 36, 52)]                      # forward: 16 x 32 positions -1, (0 above), +1, +10
KINDS = ["rand", "near"]
ids = lambda s: "x".join(map(str, s))


def L():
    from hcflow_amd import losses
    return losses


@functools.lru_cache(maxsize=None)
def inputs(shape, kind):
    """x, y fp32 on the GPU (never modified by a test) and one upstream weight per sample. 'near': y = x + 1e-3 * randn, rounded
    to fp32 -- where a refinement loop ends up and where fp32 loses the most."""
    g = torch.Generator().manual_seed(sum(shape) + 7 * len(kind))
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    y = torch.rand(shape, generator=g, dtype=torch.float64) if kind == "rand" else x + 1e-3 * torch.randn(shape, generator=g,
                                                                                                          dtype=torch.float64)
    w = torch.rand(shape[0], generator=g) + 0.5
    return x.float().cuda(), y.float().cuda(), w.cuda()


@functools.lru_cache(maxsize=None)
def reference(shape, kind, y_channel=False):
    """float64 on the CPU, computed once: rows, loss, the gradients of (rows * w).sum() and of the loss."""
    x, y, w = inputs(shape, kind)
    a, b = x.double().cpu().requires_grad_(True), y.double().cpu().requires_grad_(True)
    rows = O.ssim(a, b, y_channel)
    ga, gb = O.grads((rows * w.double().cpu()).sum(), a, b)
    loss = O.ssim_loss(a, b, y_channel)
    la, lb = O.grads(loss, a, b)
    return rows.detach(), loss.detach(), ga, gb, la, lb


def value_close(what, have, ref):
    have, ref = have.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert have.shape == ref.shape, (what, have.shape, ref.shape)
    gate = torch.tensor(np.spacing(ref.abs().numpy().astype(np.float32)).astype(np.float64)) + 1e-13
    err = (have - ref).abs()
    print("%s: value error / gate = %.3g (max err %.3g)" % (what, float((err / gate).max()), float(err.max())))
    assert bool((err <= gate).all()), (what, float(err.max()), have.tolist(), ref.tolist())


def grad_close(what, have, ref):
    have, ref = have.detach().double().cpu(), ref.detach().double().cpu()
    assert have.shape == ref.shape, (what, have.shape, ref.shape)
    gate = ULP * ref.abs() + 1e-10 * float(ref.abs().max())
    err = (have - ref).abs()
    print("%s: gradient error / gate = %.3g (max err %.3g of max|ref| %.3g)" % (what, float((err / gate).max()), float(err.max()),
                                                                           float(ref.abs().max())))
    assert bool((err <= gate).all()), (what, int((err > gate).sum()), float(err.max()), float(ref.abs().max()))


def run_rows(x, y, w, need=(True, True), **kw):
    """(rows, gx, gy) of ssim with the upstream vector w; a gradient that is not asked for is None."""
    a, b = x.clone().requires_grad_(need[0]), y.clone().requires_grad_(need[1])
    v = L().ssim(a, b, **kw)
    (v * w).sum().backward()
    return v.detach(), a.grad, b.grad


def run_loss(x, y, need=(True, True), **kw):
    a, b = x.clone().requires_grad_(need[0]), y.clone().requires_grad_(need[1])
    v = L().SSIMLoss(**kw)(a, b)
    v.backward()
    return v.detach(), a.grad, b.grad


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_ssim_matches_float64(shape, kind):
    """Per-sample values and the loss within one fp32 rounding; gx alone, gy alone and both, per element."""
    x, y, w = inputs(shape, kind)
    rows, loss, ga, gb, la, lb = reference(shape, kind)
    tag = "%s %s" % (ids(shape), kind)
    v, gx, gy = run_rows(x, y, w)
    assert v.dtype == torch.float32 and v.shape == (shape[0],)
    value_close(tag + " rows", v, rows)
    grad_close(tag + " rows gx (both)", gx, ga)
    grad_close(tag + " rows gy (both)", gy, gb)
    v1, gx1, none = run_rows(x, y, w, (True, False))
    assert none is None and torch.equal(v1, v)
    grad_close(tag + " rows gx alone", gx1, ga)
    v2, none, gy2 = run_rows(x, y, w, (False, True))
    assert none is None and torch.equal(v2, v)
    grad_close(tag + " rows gy alone", gy2, gb)
    l, lx, ly = run_loss(x, y)
    assert l.dtype == torch.float32 and l.dim() == 0
    value_close(tag + " loss", l, loss)
    grad_close(tag + " loss gx", lx, la)
    grad_close(tag + " loss gy", ly, lb)
    assert torch.equal(L().ssim(x, y), v) and torch.equal(L().SSIMLoss()(x, y), l)         # no graph, the same bits


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(1, 3, 11, 11), (2, 3, 16, 27), (3, 3, 43, 37)], ids=ids)
def test_y_channel_matches_float64_on_luma(shape, kind):
    x, y, w = inputs(shape, kind)
    rows, loss, ga, gb, la, lb = reference(shape, kind, True)
    tag = "%s %s Y" % (ids(shape), kind)
    v, gx, gy = run_rows(x, y, w, y_channel=True)
    value_close(tag + " rows", v, rows)
    grad_close(tag + " rows gx", gx, ga)
    grad_close(tag + " rows gy", gy, gb)
    l, lx, none = run_loss(x, y, (True, False), y_channel=True)
    value_close(tag + " loss", l, loss)
    grad_close(tag + " loss gx alone", lx, la)
    l2, none, ly = run_loss(x, y, (False, True), y_channel=True)
    assert torch.equal(l2, l)
    grad_close(tag + " loss gy alone", ly, lb)


@pytest.mark.parametrize("y_channel", [False, True])
def test_data_range_scales_the_constants(y_channel):
    """Inputs in [0, 255] with data_range = 255: the reference's own units."""
    shape = (2, 3, 16, 27)
    x, y, w = inputs(shape, "near")
    x255, y255 = (x.double() * 255).float(), (y.double() * 255).float()
    a, b = x255.double().cpu().requires_grad_(True), y255.double().cpu().requires_grad_(True)
    rows = O.ssim(a, b, y_channel, 255.0)
    ga, gb = O.grads((rows * w.double().cpu()).sum(), a, b)
    v, gx, gy = run_rows(x255, y255, w, y_channel=y_channel, data_range=255.0)
    value_close("data_range 255 rows", v, rows)
    grad_close("data_range 255 gx", gx, ga)
    grad_close("data_range 255 gy", gy, gb)


@pytest.mark.parametrize("y_channel", [False, True])
def test_identical_inputs_give_exactly_one_and_zero(y_channel):
    """Both factors of S are a value over its own bits and sums of ones are exact: 1.0 and 0.0, not nearly. The gradient is an
    exact zero too: at every position A = 0 and C = -2 B bit for bit, so the two products of the last step cancel."""
    for shape in [(2, 3, 11, 11), (3, 3, 43, 37), (2, 3, 36, 52)]:
        x, _, w = inputs(shape, "rand")
        v, gx, gy = run_rows(x, x, w, y_channel=y_channel)
        assert torch.equal(v, torch.ones_like(v)), v.tolist()
        assert not bool(gx.any()) and not bool(gy.any())
        l, lx, ly = run_loss(x, x, y_channel=y_channel)
        assert float(l) == 0.0 and not bool(lx.any()) and not bool(ly.any())


@pytest.mark.parametrize("shape", [(3, 3, 43, 37), (3, 1, 26, 42)], ids=ids)
def test_reproducible_and_independent_of_batch_and_alignment(shape):
    for kw in ({}, {"y_channel": True}):
        if kw and shape[1] != 3:
            continue
        x, y, w = inputs(shape, "near")
        first = run_rows(x, y, w, **kw)
        for a, b in zip(first, run_rows(x, y, w, **kw)):                   # two calls: equal bits
            assert torch.equal(a, b)
        lfirst = run_loss(x, y, **kw)
        for a, b in zip(lfirst, run_loss(x, y, **kw)):
            assert torch.equal(a, b)
        for b in range(shape[0]):                                          # row b of the batch = the one-sample call
            vb, gxb, gyb = run_rows(x[b:b + 1], y[b:b + 1], w[b:b + 1], **kw)
            assert torch.equal(vb[0], first[0][b]) and torch.equal(gxb[0], first[1][b]) and torch.equal(gyb[0], first[2][b])
        N = x.numel()
        bx, by = torch.empty(N + 1, device="cuda"), torch.empty(N + 3, device="cuda")
        xo, yo = bx[1:].view(shape), by[3:].view(shape)                    # 4 and 12 bytes past a 16-byte boundary
        xo.copy_(x)
        yo.copy_(y)
        assert xo.is_contiguous() and xo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == 12
        for a, b in zip(first, run_rows(xo, yo, w, **kw)):
            assert torch.equal(a, b)
        for a, b in zip(lfirst, run_loss(xo, yo, **kw)):
            assert torch.equal(a, b)
        # gx alone and gy alone are the bits of the joint call (S and every step of the backward are symmetric in x and y)
        assert torch.equal(run_rows(x, y, w, (True, False), **kw)[1], first[1])
        assert torch.equal(run_rows(x, y, w, (False, True), **kw)[2], first[2])


def test_values_are_the_pair_metrics_columns_on_stored_images():
    """ssim(from_image(a), from_image(b)) against the SSIM and SSIM_Y columns of PairMetrics (crop 0), gate ulp32 + 1e-13.
    PairMetrics works on the integers k, the criterion on fp32(k / 255), which is k / 255 (1 + d), |d| <= 2^-24 per pixel: in
    float64 the two definitions differ by about 5e-11 on a validation pair (an image and a degraded copy, SSIM 0.99, ulp32 6e-8;
    measured with the oracles on the CPU) -- far inside the gate. On two unrelated noise images SSIM is 1e-3, its ulp32 1e-10
    lies below that representation gap, and no kernel could meet the gate: the pair here is the kind the metric is used on."""
    from hcflow_amd import metrics
    ls = L()
    g = torch.Generator().manual_seed(3)
    B, H, W = 2, 43, 37
    a = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.int64)
    b = (a + torch.randint(-6, 7, (B, H, W, 3), generator=g, dtype=torch.int64)).clamp(0, 255)
    fa, fb = metrics.from_image(a.to(torch.uint8).cuda()), metrics.from_image(b.to(torch.uint8).cuda())
    pm = metrics.PairMetrics()
    m = pm.compare(pm.embed(fa, 0, 0), fb)
    assert bool((m[:, 1] < 1).all()) and bool((m[:, 1] > 0.9).all())
    value_close("PairMetrics ssim", ls.ssim(fa, fb), m[:, 1])
    value_close("PairMetrics ssim_y", ls.ssim(fa, fb, y_channel=True), m[:, 3])


def test_zero_upstream_and_nonfinite_pixels():
    """A sample whose upstream gradient is 0 gets exact zeros; a NaN pixel makes its sample's value (and the loss) non-finite and
    leaves the other samples alone; through finite_sum the poisoned term's inputs receive exact zeros."""
    ls = L()
    shape = (3, 3, 43, 37)
    x, y, w = inputs(shape, "near")
    rows, _, ga, gb, _, _ = reference(shape, "near")
    w0 = w.clone()
    w0[1] = 0.0
    v, gx, gy = run_rows(x, y, w0)
    assert not bool(gx[1].any()) and not bool(gy[1].any())
    grad_close("zero upstream, sample 0", gx[0], ga[0])
    grad_close("zero upstream, sample 2", gy[2], gb[2])
    xp = x.clone()
    xp[1, 2, 42, 36] = float("nan")                                        # the last pixel of sample 1: one window sees it
    vp, gxp, gyp = run_rows(xp, y, w0)
    assert not bool(torch.isfinite(vp[1])) and torch.equal(vp[0], v[0]) and torch.equal(vp[2], v[2])
    assert not bool(gxp[1].any()) and not bool(gyp[1].any())               # exact zeros, also at the poisoned pixel
    assert torch.equal(gxp[0], gx[0]) and torch.equal(gxp[2], gx[2])
    for poison in (float("nan"), float("inf")):
        xp[1, 2, 42, 36] = poison
        assert not bool(torch.isfinite(ls.SSIMLoss()(xp, y)))
        a, c = xp.clone().requires_grad_(True), x.clone().requires_grad_(True)
        total, vals = ls.finite_sum(0.5 * ls.SSIMLoss()(a, y), ls.SSIMLoss(y_channel=True)(c, y))
        assert not bool(torch.isfinite(vals[0])) and bool(torch.isfinite(vals[1])) and torch.equal(total.detach(), vals[1])
        total.backward()
        assert not bool(a.grad.any())
        grad_close("finite_sum keeps the finite term", c.grad, reference(shape, "near", True)[4])


def test_one_node_no_graph_without_grad_and_refusals_before_any_launch():
    ls = L()
    x, y, w = inputs((2, 3, 16, 27), "rand")
    a = x.clone().requires_grad_(True)
    for v in (ls.ssim(a, y), ls.SSIMLoss()(a, y)):
        assert type(v.grad_fn).__name__ == "_SsimFnBackward"               # ONE node between the result and the leaf
        assert [type(f).__name__ for f, _ in v.grad_fn.next_functions if f is not None] == ["AccumulateGrad"]
    assert ls.ssim(x, y).grad_fn is None and ls.SSIMLoss()(x, y).grad_fn is None
    with torch.no_grad():
        assert ls.SSIMLoss()(a, y).grad_fn is None
    # an upstream scalar on the device, a non-contiguous input whose autograd link is kept
    rows, loss, ga, gb, la, lb = reference((2, 3, 16, 27), "rand")
    at = x.transpose(2, 3).contiguous().requires_grad_(True)
    assert not at.transpose(2, 3).is_contiguous()
    s = torch.tensor(0.37, device="cuda")
    (s * ls.SSIMLoss()(at.transpose(2, 3), y)).backward()
    grad_close("non-contiguous, scaled", at.grad.transpose(2, 3), 0.37 * la)
    # refusals are worded in Python: nothing is launched (a launch on these shapes would be a status code, then an HcfError)
    for bad in (lambda: ls.ssim(x[:, :, :10], y[:, :, :10]), lambda: ls.SSIMLoss()(x[:, :, :, :10], y[:, :, :, :10]),
                lambda: ls.ssim(x[:, :1], y[:, :1], y_channel=True), lambda: ls.SSIMLoss(True)(x[:, :1], y[:, :1])):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ls.ssim(x, y[:, :2]), lambda: ls.ssim(x, y.double()), lambda: ls.ssim(x, y.cpu())):
        with pytest.raises(Exception) as e:
            bad()
        assert type(e.value).__name__ == "HcfError"
