"""CPU checks of the SSIM criterion (hcflow_amd/losses.py: ssim, SSIMLoss; hcf_ssim.hip): the float64 oracle the GPU tests use
(tests/ssim_loss_oracle.py) is the SSIM of oracle/metrics_oracle.py, every native entry refuses bad arguments before it touches a
device, and the module surface fails loudly off the GPU.

Gate of the oracle comparison: 1e-12 absolute on values in [-1, 1]. Both sides are float64 sums of 121 terms of O(1) evaluated in
different orders (grouped conv2d here, scipy correlate2d there): 121 * 2^-53 = 1.3e-14 per moment, through the ratio a few 1e-14;
measured 2.2e-15 or better."""
import ctypes as C

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from oracle import metrics_oracle as MO
from tests import ssim_loss_oracle as O

NEW = ["hcf_loss_ssim_workspace", "hcf_loss_ssim", "hcf_loss_ssim_backward"]
GATE = 1e-12
SHAPES = [(2, 3, 11, 11), (1, 1, 12, 11), (2, 3, 16, 27), (2, 3, 43, 37)]


def pairs(shape, kind, grid):
    """x, y float64 [B,C,H,W] in [0, 1]: random or near-identical, fp32-representable or multiples of 1/255."""
    g = torch.Generator().manual_seed(sum(shape) + len(kind))
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    y = torch.rand(shape, generator=g, dtype=torch.float64) if kind == "rand" else x + 1e-3 * torch.randn(shape, generator=g,
                                                                                                          dtype=torch.float64)
    if grid:
        return torch.round(x.clamp(0, 1) * 255) / 255, torch.round(y.clamp(0, 1) * 255) / 255
    return x.float().double(), y.float().double()


@pytest.mark.parametrize("grid", [False, True], ids=["float", "k255"])
@pytest.mark.parametrize("kind", ["rand", "near"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_oracle_is_the_metrics_oracle_ssim(shape, kind, grid):
    x, y = pairs(shape, kind, grid)
    B, Cn, H, W = shape
    v = O.ssim(x, y)
    m = O.ssim_map(x, y).mean(dim=(2, 3))
    v255 = O.ssim(255 * x, 255 * y, data_range=255.0)                  # the reference's own units
    for b in range(B):
        planes = [MO.ssim(255 * x[b, c].numpy(), 255 * y[b, c].numpy()) for c in range(Cn)]
        for c in range(Cn):
            assert abs(float(m[b, c]) - planes[c]) <= GATE
        hwc = lambda t_: np.ascontiguousarray((255 * t_[b]).numpy().transpose(1, 2, 0))
        ref = MO.calculate_ssim(hwc(x), hwc(y)) if Cn > 1 else MO.calculate_ssim(hwc(x)[:, :, 0], hwc(y)[:, :, 0])
        assert abs(float(v[b]) - ref) <= GATE and abs(float(v255[b]) - ref) <= GATE
        assert abs(float(v[b]) - float(np.mean(planes))) <= GATE
    assert abs(float(O.ssim_loss(x, y)) - (1.0 - float(v.mean()))) <= GATE


@pytest.mark.parametrize("grid", [False, True], ids=["float", "k255"])
@pytest.mark.parametrize("kind", ["rand", "near"])
def test_oracle_y_channel_is_bgr2y_then_ssim(kind, grid):
    x, y = pairs((2, 3, 16, 27), kind, grid)
    yx, yy = O.luma(x), O.luma(y)
    v = O.ssim(x, y, y_channel=True)
    for b in range(2):
        bgr = lambda t_: np.ascontiguousarray(t_[b].numpy()[::-1].transpose(1, 2, 0))       # RGB CHW -> BGR HWC
        ra, rb = MO.bgr2y(bgr(x)), MO.bgr2y(bgr(y))
        assert np.abs(yx[b, 0].numpy() - ra).max() <= GATE and np.abs(yy[b, 0].numpy() - rb).max() <= GATE
        assert abs(float(v[b]) - MO.calculate_ssim(ra * 255, rb * 255)) <= GATE
        # calculate_psnr_ssim's fourth number is this on the uncropped pair
        assert abs(float(v[b]) - MO.calculate_psnr_ssim(bgr(x), bgr(y), 0)[3]) <= GATE


def test_oracle_is_one_on_identical_inputs_and_differentiable():
    x, _ = pairs((1, 3, 16, 27), "rand", False)
    assert abs(float(O.ssim(x, x)) - 1.0) <= GATE
    a, b = x.clone().requires_grad_(True), (x * 0.9).requires_grad_(True)
    ga, gb = O.grads(O.ssim_loss(a, b), a, b)
    assert ga.shape == x.shape and gb.shape == x.shape and bool(torch.isfinite(ga).all()) and float(ga.abs().max()) > 0


def test_new_entries_are_bound():
    lib = _lib.load()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.hcf_loss_ssim_workspace.restype is C.c_size_t
    assert lib.hcf_loss_ssim.restype is C.c_int and lib.hcf_loss_ssim_backward.restype is C.c_int


def _host():
    buf = (C.c_float * 64)()                          # never dereferenced: every call below is refused first
    return buf, C.cast(buf, C.c_void_p).value


def test_ssim_entries_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    n = None
    buf, p = _host()

    def fwd(x=p, y=p, B=2, Cn=3, H=16, W=27, ych=0, R=1.0, rows=p, loss=n, work=p, wb=1 << 20):
        return lib.hcf_loss_ssim(x, y, B, Cn, H, W, ych, R, rows, loss, work, wb, n)

    def bwd(x=p, y=p, B=2, Cn=3, H=16, W=27, ych=0, R=1.0, g=p, gs=1, scale=1.0, gx=p, gy=n):
        return lib.hcf_loss_ssim_backward(x, y, B, Cn, H, W, ych, R, g, gs, scale, gx, gy, n)

    def ws(B=2, Cn=3, H=16, W=27, ych=0):
        return lib.hcf_loss_ssim_workspace(B, Cn, H, W, ych)
    assert fwd(x=n) == -1 and fwd(y=n) == -1 and fwd(rows=n) == -1 and fwd(work=n) == -1          # NULL pointers
    assert bwd(x=n) == -1 and bwd(y=n) == -1 and bwd(g=n) == -1 and bwd(gx=n, gy=n) == -1
    assert fwd(B=0) == -1 and fwd(Cn=0) == -1 and fwd(H=0) == -1 and fwd(W=-3) == -1 and bwd(B=0) == -1 and bwd(Cn=0) == -1
    assert fwd(ych=2) == -1 and bwd(ych=-1) == -1 and bwd(gs=2) == -1 and bwd(gs=-1) == -1
    assert fwd(R=0.0) == -1 and fwd(R=float("nan")) == -1 and bwd(R=float("inf")) == -1 and bwd(scale=float("nan")) == -1
    assert fwd(x=p + 2) == -1 and fwd(rows=p + 1) == -1 and fwd(work=p + 4) == -1 and bwd(gx=p + 2) == -1 and bwd(gy=p + 3) == -1
    assert fwd(H=10) == -5 and fwd(W=10) == -5 and bwd(H=10) == -5 and bwd(W=10) == -5            # no room for the window
    assert fwd(Cn=1, ych=1) == -5 and bwd(Cn=1, ych=1) == -5 and fwd(Cn=4, ych=1) == -5           # Y needs RGB
    assert fwd(B=21846) == -5 and bwd(B=65536, Cn=1) == -5 and fwd(H=(1 << 20) + 1) == -5         # planes, side
    assert fwd(wb=8) == -7 and fwd(wb=ws() - 1) == -7                                             # a short workspace
    assert ws(H=10) == 0 and ws(W=10) == 0 and ws(Cn=1, ych=1) == 0 and ws(B=0) == 0 and ws(ych=3) == 0
    # one slot per 16 x 32 tile of positions and plane, one per plane, one per sample
    assert ws() >= (2 * 3 * 1 + 2 * 3 + 2) * 8 and ws(H=11, W=11) >= (6 + 6 + 2) * 8
    assert ws(B=1, Cn=1, H=26, W=42) < ws(B=1, Cn=1, H=27 + 4096, W=42)
    assert ws(ych=1) <= ws()


def test_module_surface_fails_loudly_off_the_gpu():
    import hcflow_amd
    from hcflow_amd import losses
    for name in ("ssim", "SSIMLoss"):
        assert name in losses.__all__ and name in hcflow_amd.__all__ and getattr(hcflow_amd, name) is getattr(losses, name)
    a, b = torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16)
    for call in (lambda: losses.ssim(a, b), lambda: losses.ssim(a, b, y_channel=True), lambda: losses.SSIMLoss()(a, b),
                 lambda: losses.SSIMLoss(True, 255.0)(a, b)):
        with pytest.raises(_lib.HcfError, match="GPU only"):
            call()                                                      # a CPU tensor: no fallback
    with pytest.raises(_lib.HcfError, match="input is .* target is"):
        losses.ssim(a, b[:, :2])
    with pytest.raises(_lib.HcfError, match="float32 only"):
        losses.SSIMLoss()(a, b.double())
    with pytest.raises(_lib.HcfError):
        losses.ssim(a, "b")
    # what the kernels refuse as a status code is worded here, before any device is looked for
    with pytest.raises(ValueError, match="11 x 11 window"):
        losses.ssim(a[:, :, :10], b[:, :, :10])
    with pytest.raises(ValueError, match="11 x 11 window"):
        losses.SSIMLoss()(a[:, :, :, :10], b[:, :, :, :10])
    with pytest.raises(ValueError, match="y_channel"):
        losses.ssim(a[:, :1], b[:, :1], y_channel=True)
    with pytest.raises(ValueError):
        losses.ssim(a[0], b[0])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            losses.SSIMLoss(data_range=bad)
        with pytest.raises(ValueError):
            losses.ssim(a, b, data_range=bad)
