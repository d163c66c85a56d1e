"""-m gpu: hcflow_amd.lpips.LPIPSMap (hcf_lpips_alex_embed / hcf_lpips_alex_map: one input through AlexNet, the head against a
stored reference, the fused upsample + sum + per-pixel-best kernel) against the CPU restatement tests/lpips_map_oracle.py, its
exact properties (bit-equality with the metric, m(x, x) = 0, reproducibility, independence of the batch, of the stream and of the
order of a sample set), the sample-set statistics, the failure modes, and loader.evaluate_sample_set.

Gates. Random pairs: per pixel ``|D - ref| <= 1e-6 + 1e-4 |ref|``, the scalar metric's gate (tests/test_gpu_lpips.py); the
reference's pixels lie in 1.2e-2 .. 3.5e-2 there, so the absolute term is at most 1e-4 relative. Near-identical pairs: the map is
about 1e-7, below that absolute term, so the gate is per image on ``max|D - ref| / max|ref| <= 8 * max(e32, 1e-6)`` with ``e32``
the same measure for the float32 CPU evaluation of the restatement, worst image of the case (the convention of
tests/test_gpu_lpips_loss.py: both are fp32 evaluations that differ in summation order only, the head's cancellation amplifies
both alike, the floor guards against a lucky e32)."""
import functools

import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd.lpips import LPIPS, LPIPSMap
from tests import lpips_map_oracle as MO

pytestmark = pytest.mark.gpu

ABS, REL = 1e-6, 1e-4
GATE_FACTOR, E32_FLOOR = 8.0, 1e-6
SHAPES = [(2, 31, 47), (2, 33, 31), (3, 45, 70), (2, 64, 96), (2, 160, 160)]


@functools.lru_cache(maxsize=None)
def _metric():
    return LPIPS(seed=0).cuda()


@pytest.fixture(scope="module")
def metric():
    return _metric()


@pytest.fixture(scope="module")
def mapper(metric):
    return LPIPSMap(metric)


def _pair(B, H, W, kind, seed):
    """tests/test_gpu_lpips.py: _pair."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    if kind == "random":
        x1 = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    else:                                            # near-identical: where the cancellation in the head is worst
        x1 = (x0 + 1e-3 * torch.randn(B, 3, H, W, generator=g)).clamp(-1, 1)
    return x0, x1


@functools.lru_cache(maxsize=None)
def _case(B, H, W, kind):
    """(x0, x1, the float64 map, the float32 map of the restatement), computed once per case."""
    x0, x1 = _pair(B, H, W, kind, seed=H * 7 + W)
    sd = _metric().state_dict()
    return x0, x1, MO.lpips_map(x0, x1, sd), MO.lpips_map(x0, x1, sd, dtype=torch.float32).double()


def _rel_max(D, ref):
    """max|D - ref| / max|ref| per image."""
    return (D - ref).abs().amax(dim=(1, 2)) / ref.abs().amax(dim=(1, 2))


# ---- 1. the map against the oracle
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_map_matches_oracle_random(mapper, B, H, W):
    x0, x1, ref, ref32 = _case(B, H, W, "random")
    D = mapper(x0.cuda(), x1.cuda())
    assert D.shape == (B, 1, H, W) and D.dtype == torch.float32
    got = D[:, 0].double().cpu()
    gate = ABS + REL * ref.abs()
    share = float(((got - ref).abs() / gate).max())
    share32 = float(((ref32 - ref).abs() / gate).max())
    print("lpips-map-vs-oracle random B=%d %dx%d: worst |D-ref|/gate %.4f (fp32 CPU restatement: %.4f), ref in [%.3e, %.3e]"
          % (B, H, W, share, share32, float(ref.min()), float(ref.max())))
    assert share <= 1.0


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_map_matches_oracle_near(mapper, B, H, W):
    x0, x1, ref, ref32 = _case(B, H, W, "near")
    got = mapper(x0.cuda(), x1.cuda())[:, 0].double().cpu()
    e32 = float(_rel_max(ref32, ref).max())
    gate = GATE_FACTOR * max(e32, E32_FLOOR)
    worst = float(_rel_max(got, ref).max())
    print("lpips-map-vs-oracle near B=%d %dx%d: e32 %.3e, gate %.3e, worst per-image max|D-ref|/max|ref| %.3e (%.3f of the gate), "
          "max ref %.3e" % (B, H, W, e32, gate, worst, worst / gate, float(ref.max())))
    assert worst <= gate


# ---- 2. bit-exactness: no tolerance anywhere
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("normalize", [False, True])
def test_compare_is_the_metric_bit_for_bit(metric, mapper, B, H, W, normalize):
    x0, x1, _, _ = _case(B, H, W, "random")
    if normalize:
        x0, x1 = (x0 + 1) / 2, (x1 + 1) / 2
    x0, x1 = x0.cuda(), x1.cuda()
    want = metric(x0, x1, normalize=normalize)
    ref = mapper.embed(x0, normalize=normalize)
    got = mapper.compare(ref, x1)
    assert got.shape == (B, 1, 1, 1) and torch.equal(got, want) and bool((want > 0).all())
    d, D = mapper.compare(ref, x1, spatial=True)
    assert torch.equal(d, want)
    assert torch.equal(D, mapper(x0, x1, normalize=normalize))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_identity_is_exactly_zero_and_calls_are_bitwise_equal(mapper, B, H, W):
    x0, x1, _, _ = _case(B, H, W, "random")
    x0, x1 = x0.cuda(), x1.cuda()
    assert bool((mapper(x0, x0) == 0).all())
    a, b = mapper(x0, x1), mapper(x0, x1)
    assert torch.equal(a, b) and bool((a > 0).all())


def test_image_value_does_not_depend_on_the_batch(mapper):
    x0, x1, _, _ = _case(3, 45, 70, "random")
    x0, x1 = x0.cuda(), x1.cuda()
    d, D = mapper.compare(mapper.embed(x0), x1, spatial=True)
    acc = mapper.sample_set(x0).add(x1).result()
    for b in range(3):
        d1, D1 = mapper.compare(mapper.embed(x0[b:b + 1]), x1[b:b + 1], spatial=True)
        assert torch.equal(d1, d[b:b + 1]) and torch.equal(D1, D[b:b + 1])
        one = mapper.sample_set(x0[b:b + 1]).add(x1[b:b + 1]).result()
        for k in ("lpips", "map_mean"):
            assert torch.equal(one[k], acc[k][:, b:b + 1]), k
        for k in ("local_best", "global_best", "best_map"):
            assert torch.equal(one[k], acc[k][b:b + 1]), k


def test_runs_on_the_current_stream(mapper):
    x0, x1, _, _ = _case(2, 64, 96, "random")
    x0, x1 = x0.cuda(), x1.cuda()
    want_d, want_D = mapper.compare(mapper.embed(x0), x1, spatial=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got_d, got_D = mapper.compare(mapper.embed(x0), x1, spatial=True)
    torch.cuda.current_stream().wait_stream(s)
    assert torch.equal(got_d, want_d) and torch.equal(got_D, want_D)


# ---- 3. set statistics
def _sample_set(M=3, B=3, H=45, W=70, seed=21):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(B, 3, H, W, generator=g)
    return gt, [(gt + 0.2 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1) for _ in range(M)]


def test_sample_set_statistics(metric, mapper):
    gt, samples = _sample_set()
    sd = metric.state_dict()
    ref = MO.set_stats([MO.lpips_map(gt, s, sd, normalize=True) for s in samples])
    gtc, sc = gt.cuda(), [s.cuda() for s in samples]
    acc = mapper.sample_set(gtc, normalize=True)
    for s in sc:
        acc.add(s)
    r = acc.result()
    M, B, H, W = 3, 3, 45, 70
    assert r["lpips"].shape == (M, B) and r["map_mean"].shape == (M, B) and r["best_map"].shape == (B, 1, H, W)
    assert r["global_best"].shape == (B,) and r["local_best"].shape == (B,) and r["score"].shape == (B,)
    assert r["global_best_index"].dtype == torch.int64 and r["score"].dtype == torch.float64
    maps = []
    for m, s in enumerate(sc):
        assert torch.equal(r["lpips"][m], metric(gtc, s, normalize=True).reshape(-1))
        maps.append(mapper(gtc, s, normalize=True))
        assert bool((r["best_map"] <= maps[-1]).all())
    assert bool((r["local_best"] <= r["global_best"]).all())
    worst = 0.0
    for k in ("map_mean", "global_best", "local_best"):
        got, want = r[k].double().cpu(), ref[k]
        share = float(((got - want).abs() / (ABS + REL * want.abs())).max())
        worst = max(worst, share)
        assert share <= 1.0, (k, got, want)
    # the score is the formula on the returned vectors, exactly
    g64, l64 = r["global_best"].double(), r["local_best"].double()
    assert torch.equal(r["score"], (g64 - l64) / g64) and bool((g64 > 0).all())
    # the index: only where the oracle's two smallest means are apart (they are, for these inputs)
    two = ref["map_mean"].sort(dim=0).values[:2]
    apart = (two[1] - two[0]) > 1e-3 * two[0]
    assert bool(apart.all()), two
    assert torch.equal(r["global_best_index"].cpu(), ref["global_best_index"])
    print("lpips-map sample set M=3 B=3 45x70: worst |stat-ref|/gate %.4f, score %s (oracle %s)"
          % (worst, ["%.4f" % v for v in r["score"].tolist()], ["%.4f" % v for v in ref["score"].tolist()]))
    assert float(ref["score"].min()) > 0.02                      # far from 0: the statistic is exercised

    # another order: the same best_map, global_best and local_best, bit for bit
    acc2 = mapper.sample_set(gtc, normalize=True)
    for s in (sc[2], sc[0], sc[1]):
        acc2.add(s)
    r2 = acc2.result()
    for k in ("best_map", "global_best", "local_best"):
        assert torch.equal(r2[k], r[k]), k
    moved = {0: 1, 1: 2, 2: 0}                                   # sample m of the first run is sample moved[m] of this one
    assert r2["global_best_index"].tolist() == [moved[i] for i in r["global_best_index"].tolist()]

    # M = 1: the best map is the map, local_best its mean, score 0
    one = mapper.sample_set(gtc, normalize=True).add(sc[0]).result()
    assert torch.equal(one["best_map"], maps[0]) and torch.equal(one["local_best"], one["map_mean"][0])
    assert torch.equal(one["global_best"], one["map_mean"][0]) and bool((one["score"] == 0).all())
    assert torch.equal(one["map_mean"][0], r["map_mean"][0])


def test_sample_set_grows_beyond_its_capacity(mapper):
    gt, samples = _sample_set(M=3, B=2, H=33, W=31, seed=4)
    gtc, sc = gt.cuda(), [s.cuda() for s in samples]
    small, big = mapper.sample_set(gtc, normalize=True, capacity=1), mapper.sample_set(gtc, normalize=True)
    for s in sc:
        small.add(s)
        big.add(s)
    a, b = small.result(), big.result()
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---- 4. failure modes
def test_failure_modes(mapper):
    x = torch.rand(1, 3, 30, 64, device="cuda")
    with pytest.raises(_lib.HcfError):
        mapper(x, x)
    with pytest.raises(_lib.HcfError):
        mapper.embed(x)
    y = torch.rand(2, 3, 40, 44, device="cuda")
    yg = y.clone().requires_grad_(True)
    with pytest.raises(_lib.HcfError):
        mapper(yg, y)
    with pytest.raises(_lib.HcfError):
        mapper.embed(yg)
    ref = mapper.embed(y, normalize=True)
    with pytest.raises(_lib.HcfError):
        mapper.compare(ref, yg)
    with pytest.raises(_lib.HcfError):
        mapper.compare(ref, y[:1])                               # another batch
    with pytest.raises(_lib.HcfError):
        mapper.compare(ref, torch.rand(2, 3, 44, 40, device="cuda"))
    with pytest.raises(_lib.HcfError):
        mapper.compare(ref, y, normalize=False)                  # embedded with normalize=True
    assert mapper.compare(ref, y, normalize=True).shape == (2, 1, 1, 1)
    acc = mapper.sample_set(y, normalize=True)
    with pytest.raises(_lib.HcfError):
        acc.result()                                             # nothing added
    with pytest.raises(_lib.HcfError):
        acc.add(torch.rand(2, 3, 40, 48, device="cuda"))
    with pytest.raises(_lib.HcfError):
        acc.result()                                             # the refused sample does not count
    assert acc.add(y).result()["lpips"].shape == (1, 2)


# ---- 5. loader.evaluate_sample_set
def test_evaluate_sample_set(metric, mapper):
    from hcflow_amd import HCFlowNet_SR, preset, make_params
    from hcflow_amd.loader import batched_test_loader, evaluate_batch, evaluate_sample_set
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
    res = evaluate_sample_set(net, b, heats, n_sample, mapper, seed=seed)
    want = evaluate_batch(net, b, heats, n_sample=n_sample, scale=4, seed=seed, lpips_fn=metric)
    gt = b["GT"].cuda()
    with torch.no_grad():
        for hi, heat in enumerate(heats):
            acc = mapper.sample_set(gt, normalize=True)
            for s in range(n_sample):
                acc.add(net(lr=b["LQ"].cuda(), z=None, u=None, eps_std=heat, reverse=True, training=False, cache_cond=True,
                            seed=seed + 1000 * hi + s))
            r = acc.result()
            for i in range(3):
                ent, w = res[i][heat], want[i][heat]["lpips"]
                assert set(ent) == {"lpips", "lpips_best", "local_best", "score"}
                assert abs(ent["lpips"] - w) <= 1e-7 * max(1.0, abs(w)), (heat, ent["lpips"], w)
                assert ent["lpips_best"] == float(r["global_best"][i]) and ent["local_best"] == float(r["local_best"][i])
                assert ent["score"] == float(r["score"][i])
