"""-m gpu: the flow-step glue, prior and squeeze kernels (hcflow_amd/csrc/hcf_flow.hip) at MULTI-BLOCK shapes against float64
evaluations of the CPU oracle. tests/test_gpu_ops.py runs the same entry points at 16-60 pixels per sample: one block, one
partly filled wave. Here a sample spans several 256-pixel blocks (64-pixel blocks in the 25..48-channel inverse tail) with a
ragged last one, so all four waves of block_sum, several partial slots per sample and both store branches of the 48-channel
tail are held to a reference of their own.

Gates: values 2e-6 * max(1, |ref|max) (the per-op gate of test_gpu_ops.py); per-sample sums 1e-5 of the sum of the absolute
terms (fp32 accumulation of a few thousand terms stays two orders below that; a dropped wave or block slot removes at least
1/12 of the terms)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import hcflow_oracle as O
from tests.util import maxdiff

pytestmark = pytest.mark.gpu

B = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _vgate(ref):
    return 2e-6 * max(1.0, float(ref.abs().max()))


def _check_sum(got, ref, absterms, what):
    """Per-sample sums against float64: |got - ref| <= 1e-5 * sum |term|."""
    got = got.detach().cpu().double()
    gate = 1e-5 * absterms
    err = (got - ref).abs()
    print("%s: per-sample sum error %s, gate %s" % (what, err.tolist(), gate.tolist()))
    assert bool((err <= gate).all()), (what, err.tolist(), gate.tolist())


# (C, ns, H, W): pixels per sample / blocks noted per case
STEP_CASES = [
    (12, 6, 20, 30),      # 600 px: 3 blocks, 88 px in the last
    (24, 12, 17, 31),     # 527 px: 3 blocks, 15 px in the last, the widest one-thread-per-pixel inverse
    (6, 3, 33, 8),        # 264 px: 8 px in the last block
    (21, 10, 19, 14),     # 266 px, odd C (padded to 24)
    (45, 22, 13, 10),     # 48-channel inverse tail: 130 px = 3 blocks of 64 with 2 px in the last, scalar stores (C % 4 != 0)
    (48, 24, 8, 16),      # exactly 2 blocks of 64, the 16-byte store branch
    (48, 24, 5, 13),      # 65 px: one pixel in the second block
    (28, 14, 8, 8),       # exactly 64 px, C = 28: the fourth wave owns no channel
]


@pytest.mark.parametrize("C,ns,H,W", STEP_CASES)
def test_step_affine_multi_block(dev, C, ns, H, W):
    from hcflow_amd import ops
    g = _gen(1000 * C + H)
    z = torch.randn(B, C, H, W, generator=g)
    h = torch.randn(B, 2 * (C - ns), H, W, generator=g) * 0.5
    Wm = torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64))[0].float() * 1.1
    bias = torch.randn(1, C, 1, 1, generator=g) * 0.1
    logs = torch.randn(1, C, 1, 1, generator=g) * 0.1
    zd, hd, Wd, bd, ld_ = z.double(), h.double(), Wm.double(), bias.double(), logs.double()
    # inverse: coupling^-1 -> W^-1 -> actnorm^-1 (AffineCouplings.py:65-87, Permutations.py:72-74, ActNorms.py:54,66); the
    # oracle's invconv_inverse rounds the inverse to float, the float64 evaluation keeps it
    shift, scale = O.split_cross(hd)
    ls = O.logscale_of(scale)
    z2 = zd[:, ns:] * torch.exp(-ls) - shift
    winv = torch.inverse(Wd).view(C, C, 1, 1)
    ref = O.actnorm_inverse(F.conv2d(torch.cat((zd[:, :ns], z2), 1), winv), bd, ld_)
    out = ops.step_inverse(z.to(dev), h.to(dev), 0, ns, Wm, bias, logs)
    d = maxdiff(out, ref)
    print("step_inverse %s: %.3e (gate %.3e)" % ((C, ns, H, W), d, _vgate(ref)))
    assert d <= _vgate(ref), d
    # forward head: actnorm -> W
    mid = O.invconv_forward(O.actnorm_forward(zd, bd, ld_), Wd)
    o_mid = ops.step_forward_head(z.to(dev), Wm, bias, logs)
    d = maxdiff(o_mid, mid)
    assert d <= _vgate(mid), d
    # forward coupling on the float32 image of mid
    mid32 = mid.float()
    fwd = torch.cat((mid32[:, :ns].double(), (mid32[:, ns:].double() + shift) * torch.exp(ls)), 1)
    o_fwd, ld = ops.step_forward_couple(mid32.to(dev), h.to(dev), 0, ns)
    d = maxdiff(o_fwd, fwd)
    assert d <= _vgate(fwd), d
    _check_sum(ld, ls.sum(dim=(1, 2, 3)), ls.abs().sum(dim=(1, 2, 3)), "logdet %s" % ((C, ns, H, W),))


def test_step_shift3_and_no_perm_multi_block(dev):
    """AffineCoupling3shift without a permutation matrix at 300 px (2 blocks, 44 px in the last)."""
    from hcflow_amd import ops
    C, ns, H, W = 12, 3, 15, 20
    g = _gen(33)
    z = torch.randn(B, C, H, W, generator=g)
    h = torch.randn(B, 3, H, W, generator=g)
    bias = torch.randn(1, C, 1, 1, generator=g) * 0.1
    logs = torch.randn(1, C, 1, 1, generator=g) * 0.1
    zd, hd, bd, ld_ = z.double(), h.double(), bias.double(), logs.double()
    ref = O.actnorm_inverse(torch.cat((zd[:, :3] - hd, zd[:, 3:]), 1), bd, ld_)          # AffineCouplings.py:150-158
    out = ops.step_inverse(z.to(dev), h.to(dev), 1, ns, None, bias, logs)
    assert maxdiff(out, ref) <= _vgate(ref)
    head = O.actnorm_forward(zd, bd, ld_)
    assert maxdiff(ops.step_forward_head(z.to(dev), None, bias, logs), head) <= _vgate(head)
    fwd = torch.cat((zd[:, :3] + hd, zd[:, 3:]), 1)
    o_fwd, ld = ops.step_forward_couple(z.to(dev), h.to(dev), 1, ns)
    assert maxdiff(o_fwd, fwd) <= _vgate(fwd)
    assert float(ld.abs().max()) == 0.0                                                # no scale: sum |logscale| = 0


# (B, C, H, W) of the latent
GAUSS_CASES = [(3, 6, 20, 30), (2, 21, 17, 31), (2, 45, 13, 10)]


def _gauss_inputs(shape, seed):
    b, C, H, W = shape
    g = _gen(seed)
    mean = torch.randn(b, C, H, W, generator=g)
    logs = torch.rand(b, C, H, W, generator=g) * 2 - 1                                  # uniform in +-1
    x = torch.randn(b, C, H, W, generator=g)
    h = torch.stack((mean, logs), 2).reshape(b, 2 * C, H, W)                            # "cross" interleave
    return mean, logs, x, h


@pytest.mark.parametrize("shape", GAUSS_CASES)
def test_gauss_logp_multi_block(dev, shape):
    from hcflow_amd import ops
    mean, logs, x, h = _gauss_inputs(shape, 7 + shape[1])
    md, sd, xd = mean.double(), logs.double(), x.double()
    term = -0.5 * (sd * 2. + ((xd - md) ** 2) / torch.exp(sd * 2.) + O.LOG2PI)          # the terms of O.gaussian_logp
    ref = O.gaussian_logp(md, sd, xd)
    assert maxdiff(ref, term.sum(dim=(1, 2, 3))) <= 1e-9 * float(term.abs().sum())
    lp = ops.gauss_logp(h.to(dev), x.to(dev))
    _check_sum(lp, ref, term.abs().sum(dim=(1, 2, 3)), "gauss_logp %s" % (shape,))


@pytest.mark.parametrize("rescale", [False, True])
@pytest.mark.parametrize("shape", GAUSS_CASES)
def test_gauss_sample_injected_eps_multi_block(dev, shape, rescale):
    """gauss_sample_kernel: one thread per (pixel, channel); the t / C split crosses block boundaries inside a pixel's channel
    run whenever 256 is no multiple of C."""
    from hcflow_amd import ops
    mean, s, eps, h = _gauss_inputs(shape, 11 + shape[1])
    eps = eps * 0.8
    logs = O.logscale_of(s.double()) if rescale else s.double()
    ref = O.gaussian_sample(mean.double(), logs, 0.8, eps.double())
    out = ops.gauss_sample(h.to(dev), eps.to(dev), rescale=rescale)
    d = maxdiff(out, ref)
    print("gauss_sample %s rescale=%s: %.3e (gate %.3e)" % (shape, rescale, d, _vgate(ref)))
    assert d <= _vgate(ref), d


# (3, 6, 34, 22): 187 output px of the squeeze, 4 488 output elements (18 blocks) of its inverse; (2, 3, 36, 30): 270 output px,
# two blocks of the one-thread-per-pixel kernels
SQUEEZE_CASES = [(3, 6, 34, 22), (2, 3, 36, 30)]


@pytest.mark.parametrize("shape", SQUEEZE_CASES)
def test_squeeze_unsqueeze_bit_exact_multi_block(dev, shape):
    from hcflow_amd import ops
    x = torch.randn(*shape, generator=_gen(1))
    sq = ops.squeeze2d(x.to(dev)).cpu()
    assert torch.equal(sq, O.squeeze2d(x))
    assert torch.equal(ops.unsqueeze2d(sq.to(dev)).cpu(), x)
    y = torch.randn(shape[0], 4 * shape[1], shape[2] // 2, shape[3] // 2, generator=_gen(2))
    assert torch.equal(ops.unsqueeze2d(y.to(dev)).cpu(), O.unsqueeze2d(y))


@pytest.mark.parametrize("shape", SQUEEZE_CASES)
def test_haar_multi_block(dev, shape):
    """Inputs uniform in +-1: a sum of four stays below 4, three fp32 additions round by at most 3 * ulp(4) / 2 = 7.2e-7 < 1e-6."""
    from hcflow_amd import ops
    x = torch.rand(*shape, generator=_gen(3)) * 2 - 1
    fwd = ops.squeeze2d(x.to(dev), haar=True)
    assert maxdiff(fwd, O.haar_forward(x.double())) <= 1e-6
    assert maxdiff(ops.unsqueeze2d(fwd, haar=True), x) <= 1e-6
    y = torch.rand(shape[0], 4 * shape[1], shape[2] // 2, shape[3] // 2, generator=_gen(4)) * 2 - 1
    assert maxdiff(ops.unsqueeze2d(y.to(dev), haar=True), O.haar_inverse(y.double())) <= 1e-6
