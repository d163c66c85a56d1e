"""-m gpu: hcflow_amd.lpips.LPIPS (hcf_lpips_alex: the whole AlexNet + LPIPS head as one call on the fp32-MFMA kernels)
against the float64 CPU restatement tests/lpips_oracle.py (total and per-layer terms), its exact properties (LPIPS(x, x) = 0,
bitwise reproducibility, per-image independence of the batch), its failure modes and its use as evaluate_batch's lpips_fn."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hcflow_amd import _lib
from hcflow_amd.lpips import LPIPS
from tests import lpips_oracle as O
from tests.util import load_golden

pytestmark = pytest.mark.gpu

# |d - d_ref| <= ABS + REL * d_ref, per image, for the total and for each layer term
ABS, REL = 1e-6, 1e-4


@pytest.fixture(scope="module")
def model():
    return LPIPS(seed=0).cuda()


def _pair(B, H, W, kind, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    if kind == "random":
        x1 = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    else:                                            # near-identical: where the cancellation in the head is worst
        x1 = (x0 + 1e-3 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
    return x0, x1


def _check(model, x0, x1, normalize=False, tag=""):
    d, per = model(x0.cuda(), x1.cuda(), retPerLayer=True, normalize=normalize)
    assert d.shape == (x0.shape[0], 1, 1, 1) and d.dtype == torch.float32
    ref, ref_per = O.lpips_alex(x0, x1, model.state_dict(), normalize=normalize)
    got = d.reshape(-1).double().cpu()
    got_per = torch.cat([p.reshape(-1, 1) for p in per], 1).double().cpu()
    worst = 0.0
    for g, r in ((got, ref), (got_per, ref_per)):
        err = (g - r).abs()
        assert bool((err <= ABS + REL * r.abs()).all()), (tag, g, r)
        worst = max(worst, float((err / (ABS + REL * r.abs())).max()))
    rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())
    print("lpips-vs-oracle %s: worst |d-ref|/gate %.3f, worst rel(total) %.3e, d in [%.4e, %.4e]"
          % (tag, worst, rel, float(ref.min()), float(ref.max())))
    return d


@pytest.mark.parametrize("B,H,W", [(2, 160, 160), (3, 100, 132), (1, 31, 31)])
@pytest.mark.parametrize("kind", ["random", "near"])
def test_matches_oracle(model, B, H, W, kind):
    x0, x1 = _pair(B, H, W, kind, seed=H * 7 + W)
    _check(model, x0, x1, tag="%s B=%d %dx%d" % (kind, B, H, W))


def test_matches_oracle_b16_640(model):
    x0, x1 = _pair(16, 640, 640, "random", seed=640)
    x1[8:] = (x0[8:] + 1e-3 * torch.randn(8, 3, 640, 640, generator=torch.Generator().manual_seed(1))).clamp(-1, 1)
    _check(model, x0, x1, tag="B=16 640x640 (8 random, 8 near)")


def test_real_image_gt_vs_bicubic(model):
    im = load_golden("real_images")
    gt = torch.from_numpy(np.ascontiguousarray(im["butterfly_hr"])).permute(2, 0, 1)[None].float() / 255.0
    lr = torch.from_numpy(np.ascontiguousarray(im["butterfly_lr"])).permute(2, 0, 1)[None].float() / 255.0
    up = F.interpolate(lr, size=gt.shape[2:], mode="bicubic", align_corners=False).clamp(0, 1)
    d = _check(model, gt, up, normalize=True, tag="butterfly 256x256 GT vs bicubic")
    d2 = model((2 * gt - 1).cuda(), (2 * up - 1).cuda())          # normalize=True == mapping by 2x - 1 first
    assert torch.equal(d, d2)


def test_identity_is_exactly_zero_and_calls_are_bitwise_equal(model):
    x0, x1 = _pair(4, 96, 80, "random", seed=3)
    x0, x1 = x0.cuda(), x1.cuda()
    z, per = model(x0, x0, retPerLayer=True)
    assert bool((z == 0).all()) and all(bool((p == 0).all()) for p in per)
    a, b = model(x0, x1), model(x0, x1)
    assert torch.equal(a, b) and bool((a > 0).all())


def test_image_value_does_not_depend_on_the_batch(model):
    x0, x1 = _pair(16, 72, 90, "random", seed=11)
    x0, x1 = x0.cuda(), x1.cuda()
    full = model(x0, x1)
    for b in (0, 5, 15):
        assert torch.equal(model(x0[b:b + 1], x1[b:b + 1]), full[b:b + 1])


def test_failure_modes(model):
    x = torch.rand(1, 3, 30, 64, device="cuda")
    with pytest.raises(_lib.HcfError):
        model(x, x)
    with pytest.raises(_lib.HcfError):
        model(x.transpose(2, 3), x.transpose(2, 3))
    y = torch.rand(1, 3, 40, 40, device="cuda", requires_grad=True)
    with pytest.raises(_lib.HcfError):
        model(y, y.detach())
    with pytest.raises(_lib.HcfError):
        LPIPS()(y.detach(), y.detach())                            # parameters still on the CPU


def test_runs_on_the_current_stream(model):
    x0, x1 = _pair(2, 64, 64, "random", seed=2)
    x0, x1 = x0.cuda(), x1.cuda()
    want = model(x0, x1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = model(x0, x1)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(got, want)


def test_as_evaluate_batch_lpips_fn(model):
    from hcflow_amd import HCFlowNet_SR, preset, make_params
    from hcflow_amd.loader import batched_test_loader, evaluate_batch
    from tests.test_loader_cpu import FakeSet
    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.cuda().eval()
    b = next(iter(batched_test_loader(FakeSet([(12, 16)] * 3), 3)))
    heats, n_sample, seed = [0.0, 0.8], 2, 5
    res = evaluate_batch(net, b, heats, n_sample=n_sample, scale=4, seed=seed, lpips_fn=model)
    gt = b["GT"].cuda()
    with torch.no_grad():
        for hi, heat in enumerate(heats):
            ds = []
            for s in range(n_sample):
                sr = net(lr=b["LQ"].cuda(), z=None, u=None, eps_std=heat, reverse=True, training=False, cache_cond=True,
                         seed=seed + 1000 * hi + s)
                ds.append(model(2 * gt - 1, 2 * sr - 1).reshape(-1).double().cpu())
            want = torch.stack(ds).mean(0)
            for r, w in zip(res, want.tolist()):
                assert abs(r[heat]["lpips"] - w) <= 1e-7 * max(1.0, abs(w)), (heat, r[heat]["lpips"], w)


@pytest.mark.skipif(not __import__("importlib").util.find_spec("lpips"), reason="the lpips package is not installed")
def test_matches_the_lpips_package(model):
    import lpips
    ref = lpips.LPIPS(net="alex", pnet_rand=True, verbose=False).cuda().eval()
    m = LPIPS().cuda()
    m.load_state_dict(ref.state_dict(), strict=True)
    x0, x1 = _pair(2, 96, 96, "random", seed=9)
    with torch.no_grad():
        want = ref(x0.cuda(), x1.cuda()).reshape(-1).double()
    got = m(x0.cuda(), x1.cuda()).reshape(-1).double()
    assert bool(((got - want).abs() <= ABS + REL * want.abs()).all())
