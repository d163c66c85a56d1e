"""-m gpu: ``metrics.PairMetrics`` (hcf_metric_pair_*) -- PSNR / SSIM of samples against a GT prepared once -- against the metrics
oracle and the reference-generated fixture, its contract (bit-reproducible, images independent of the batch, nothing allocated
per call), the one-shot ``metrics.psnr_ssim`` wrapper over it, the uint8 image output, the sample set and the loaders.

Gates are those of tests/test_gpu_metrics.py: 1e-9 * max(1, |w|) for the full-resolution four, 1e-8 * max(1, |w|) for the
bicubic four. The separable 11 + 11 tap filter differs from the 121-tap float64 sum by rounding alone (measured on a CPU:
9.6e-15 on a random 48x64 pair, 5.0e-13 on a flat image with one changed pixel)."""
import math

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as MO
from tests.util import load_golden

pytestmark = pytest.mark.gpu

FULL, BIC = ["psnr", "ssim", "psnr_y", "ssim_y"], ["bic_psnr", "bic_ssim", "bic_psnr_y", "bic_ssim_y"]


def _pair(tag):
    g = load_golden("metrics")
    return torch.from_numpy(g["gt_" + tag]).unsqueeze(0), torch.from_numpy(g["sr_" + tag]).unsqueeze(0)


def _oracle(gt, sr, crop, scale):
    """The eight numbers of one image pair ([1,3,H,W] host tensors) by oracle.metrics_oracle."""
    g8, s8 = MO.tensor2img(gt.numpy()) / 255.0, MO.tensor2img(sr.numpy()) / 255.0
    want = list(MO.calculate_psnr_ssim(g8, s8, crop))
    if scale > 1:
        want += list(MO.calculate_psnr_ssim(MO.imresize(g8, 1.0 / scale), MO.imresize(s8, 1.0 / scale), 0))
    else:
        want += [0.0] * 4
    return want


def _close(got, want, gate, what):
    print(what, got, want)
    if math.isnan(want):
        assert math.isnan(got), what
    elif math.isinf(want):
        assert got == want, what
    else:
        assert abs(got - want) <= gate * max(1.0, abs(want)), (what, got, want)


def _hold(row, want, what):
    for i, k in enumerate(FULL + BIC):
        _close(row[k], want[i], 1e-9 if i < 4 else 1e-8, (what, k))


def _compare(gt, sr, crop, scale, **kw):
    from hcflow_amd import metrics
    pm = metrics.PairMetrics()
    return pm.compare(pm.embed(gt.cuda(), crop_border=crop, scale=scale), sr.cuda(), **kw)


# ---------------------------------------------------------------- 1. fixtures
@pytest.mark.parametrize("tag", ["a", "b"])
@pytest.mark.parametrize("crop", [0, 4])
def test_fixtures_match_the_oracle_and_the_recorded_reference(tag, crop):
    from hcflow_amd import metrics
    g = load_golden("metrics")
    gt, sr = _pair(tag)
    row = metrics.rows_to_dicts(_compare(gt, sr, crop, 4))[0]
    want = _oracle(gt, sr, crop, 4)
    _hold(row, want, (tag, crop))
    if tag == "b":                                           # 10-row low-resolution image: no valid window position
        assert math.isnan(want[5]) and math.isnan(row["bic_ssim"]) and math.isnan(row["bic_ssim_y"])
    for k, w in zip(FULL, g["psnr_ssim_cb%d_%s" % (crop, tag)]):
        _close(row[k], float(w), 1e-9, (tag, crop, k, "recorded"))
    if crop == 0:
        _close(row["psnr"], float(g["psnr_" + tag]), 1e-9, (tag, "psnr recorded"))
        _close(row["psnr_y"], float(g["psnr_y_" + tag]), 1e-9, (tag, "psnr_y recorded"))


# ---------------------------------------------------------------- 2. edge shapes
def _random_pair(H, W, B=1, seed=0):
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    gt = torch.rand(B, 3, H, W, generator=g)
    sr = (gt + 0.03 * torch.randn(gt.shape, generator=g)).clamp(-0.1, 1.1)
    return gt, sr


# (H, W), crop, scale, the columns the oracle gives nan for
EDGES = [((11, 11), 0, 2, {5, 7}), ((19, 13), 4, 3, {1, 3, 5, 7}), ((21, 75), 5, 4, {5, 7}), ((45, 47), 1, 3, set()),
         ((67, 131), 3, 8, {5, 7}), ((24, 30), 0, 2, set()), ((33, 40), 2, 0, set())]


@pytest.mark.parametrize("hw,crop,scale,nans", EDGES)
def test_edge_shapes_match_the_oracle(hw, crop, scale, nans):
    from hcflow_amd import metrics
    gt, sr = _random_pair(*hw)
    want = _oracle(gt, sr, crop, scale)
    assert {i for i, w in enumerate(want) if math.isnan(w)} == nans
    assert all(math.isfinite(w) for i, w in enumerate(want) if i not in nans)
    m = _compare(gt, sr, crop, scale)
    assert m.dtype == torch.float64 and tuple(m.shape) == (1, 8) and m.is_cuda
    _hold(metrics.rows_to_dicts(m)[0], want, (hw, crop, scale))
    if scale <= 1:
        assert m[0, 4:].tolist() == [0.0] * 4


# ---------------------------------------------------------------- 3. the one-shot wrapper
@pytest.mark.parametrize("case", ["a", "b", "45x47"])
def test_psnr_ssim_is_embed_plus_compare_bit_for_bit(case):
    """``metrics.psnr_ssim`` is a one-shot wrapper over embed + compare: every key equals exactly. (These cases are held to the
    oracle above: the fixtures at crop 4 / scale 4, and 45x47 at crop 1 / scale 3 in EDGES.)"""
    from hcflow_amd import metrics
    (gt, sr), crop, scale = (_random_pair(45, 47), 1, 3) if case == "45x47" else (_pair(case), 4, 4)
    one = metrics.psnr_ssim(gt.cuda(), sr.cuda(), crop, scale)[0]
    row = metrics.rows_to_dicts(_compare(gt, sr, crop, scale))[0]
    for k in metrics.KEYS:
        print(case, k, row[k], one[k])
        assert (math.isnan(one[k]) and math.isnan(row[k])) or one[k] == row[k], (k, row[k], one[k])


# ---------------------------------------------------------------- 4. contract
@pytest.mark.parametrize("hw,crop,scale", [((45, 47), 1, 3), ((48, 64), 4, 4)])      # byte-wise and 16-byte paths; all eight finite
def test_reproducible_batch_independent_and_allocation_free(hw, crop, scale):
    from hcflow_amd import metrics
    gt, sr = _random_pair(*hw, B=3)
    gt, sr = gt.cuda(), sr.cuda()
    pm = metrics.PairMetrics()
    ref = pm.embed(gt, crop_border=crop, scale=scale)
    m1, u1 = pm.compare(ref, sr, image=True)
    m2, u2 = pm.compare(ref, sr, image=True)
    assert torch.equal(m1, m2) and torch.equal(u1, u2) and torch.isfinite(m1).all()
    for b in range(3):
        mb, ub = pm.compare(pm.embed(gt[b:b + 1], crop_border=crop, scale=scale), sr[b:b + 1], image=True)
        assert torch.equal(mb[0], m1[b]) and torch.equal(ub[0], u1[b]), b
    same = pm.compare(ref, gt)
    for b in range(3):
        r = dict(zip(metrics.KEYS, same[b].tolist()))
        assert r["psnr"] == r["psnr_y"] == float("inf") and abs(r["ssim"] - 1.0) <= 1e-12 and abs(r["ssim_y"] - 1.0) <= 1e-12
        assert r["bic_psnr"] == r["bic_psnr_y"] == float("inf")
    out, img = torch.empty_like(m1), torch.empty_like(u1)
    pm.compare(ref, sr, out=out, image_out=img)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got = pm.compare(ref, sr, out=out, image_out=img)
    assert torch.cuda.memory_allocated() == before
    assert got[0] is out and got[1] is img and torch.equal(out, m1) and torch.equal(img, u1)


# ---------------------------------------------------------------- 5. image=True
@pytest.mark.parametrize("tag", ["a", "b"])
def test_image_output_is_tensor2img(tag):
    gt, sr = _pair(tag)
    both = torch.cat([sr, gt], 0)
    _, u8 = _compare(both, both, 4, 4, image=True)
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2,) + tuple(sr.shape[2:]) + (3,)
    for b in range(2):
        assert np.array_equal(u8[b].cpu().numpy(), MO.tensor2img(both[b].numpy())), (tag, b)


def test_image_output_rounds_half_to_even_and_clamps():
    ties = (np.arange(255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)
    assert all(float(np.float32(t) * np.float32(255.0)) == k + 0.5 for k, t in enumerate(ties))     # exact ties in fp32
    g = torch.Generator().manual_seed(4)
    x = torch.rand(3 * 16 * 17, generator=g)
    x[:255] = torch.from_numpy(ties)
    x[255], x[256] = -0.2, 1.3
    x = x[torch.randperm(x.numel(), generator=g)].reshape(1, 3, 16, 17)
    _, u8 = _compare(x, x, 0, 0, image=True)
    want = MO.tensor2img(x.numpy())
    assert np.array_equal(u8[0].cpu().numpy(), want)
    flat = (x.clamp(0, 1) * 255.0).flatten().numpy()
    tie = np.abs(flat - np.floor(flat) - 0.5) == 0
    assert tie.sum() == 255 and (want.transpose(2, 0, 1)[::-1].flatten()[tie] % 2 == 0).all()


# ---------------------------------------------------------------- 6. sample_set
def test_sample_set_rows_mean_best_and_growth():
    from hcflow_amd import _lib, metrics
    gt, _ = _random_pair(48, 64, B=2)
    gt = gt.cuda()
    g = torch.Generator().manual_seed(9)
    samples = [(gt.cpu() + s * torch.randn(gt.shape, generator=g)).clamp(0, 1).cuda() for s in (0.05, 0.01, 0.03)]
    pm = metrics.PairMetrics()
    ref = pm.embed(gt, crop_border=4, scale=4)
    acc = pm.sample_set(gt, crop_border=4, scale=4, capacity=64)
    small = pm.sample_set(gt, crop_border=4, scale=4, capacity=2)
    for sr in samples:
        acc.add(sr)
        small.add(sr)
    with pytest.raises(_lib.HcfError, match="was embedded for"):
        acc.add(samples[0][:, :, :-1])
    with pytest.raises(_lib.HcfError, match="was embedded for"):
        acc.add(samples[0].cpu())
    assert len(acc) == len(small) == 3
    r = acc.result()
    assert tuple(r["per_sample"].shape) == (3, 2, 8) and r["per_sample"].dtype == torch.float64
    for m, sr in enumerate(samples):
        assert torch.equal(r["per_sample"][m], pm.compare(ref, sr)), m
    assert torch.isfinite(r["per_sample"]).all()
    assert torch.equal(r["mean"], r["per_sample"].mean(dim=0))
    assert np.abs(r["mean"].cpu().numpy() - r["per_sample"].cpu().numpy().mean(axis=0)).max() <= 1e-12
    assert r["best_psnr_index"].tolist() == r["per_sample"][:, :, 0].argmax(dim=0).tolist() == [1, 1]
    assert torch.equal(r["best_psnr"], r["per_sample"][1, :, 0])
    assert torch.equal(small.result()["per_sample"], r["per_sample"])


# ---------------------------------------------------------------- 7. loader
def test_loaders_give_every_key_and_finite_numbers():
    """The loaders' dicts with LPIPS: the key sets, and every metric entry finite unless nan (their numbers are pinned to
    ``psnr_ssim`` by tests/test_gpu_sample_sets.py::test_evaluate_sweep_equals_its_defining_scalar_calls)."""
    from hcflow_amd import HCFlowNet_SR, preset, make_params, metrics
    from hcflow_amd.loader import batched_test_loader, evaluate_batch, evaluate_sweep
    from hcflow_amd.lpips import LPIPS
    from tests.test_loader_cpu import FakeSet
    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.cuda().eval()
    lp = LPIPS(seed=0).cuda()
    batch = next(iter(batched_test_loader(FakeSet([(12, 16)] * 2), 2)))
    kw = dict(heats=[0, 0.8], n_sample=2, scale=4, seed=7, lpips_fn=lp)
    for fn, extra in ((evaluate_batch, {}), (evaluate_sweep, {"max_batch": 3})):
        got = fn(net, batch, **kw, **extra)
        assert len(got) == 2
        for b in range(2):
            assert set(got[b].keys()) == {"nll", "lr", 0.0, 0.8}
            assert math.isfinite(got[b]["nll"]) and set(got[b]["lr"].keys()) == set(FULL)
            for ent in (got[b]["lr"], got[b][0.0], got[b][0.8]):
                assert all(math.isnan(v) or math.isfinite(v) for v in ent.values()), (fn.__name__, b, ent)
            for heat in (0.0, 0.8):
                assert set(got[b][heat].keys()) == set(metrics.KEYS) | {"lpips", "diversity"}
