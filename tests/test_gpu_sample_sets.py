"""-m gpu: judging a model by the SET of samples it draws -- one temperature per sample through the inverse pass
(hcf_inverse_taus, ``eps_std`` as a vector), the streaming per-pixel statistics ``metrics.SampleStats`` (hcf_metric_stats_*) and
``loader.evaluate_sweep``, whose calls the heats of a sweep share."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TAUS = [0.0, 0.3, 0.8, 0.8, 1.0]


def _net(name, seed, precision):
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling
    from hcflow_amd.config import preset
    from tests.util import cached_params
    cfg = preset(name)
    net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(cached_params(name, seed), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    return cfg, net.to("cuda:0").eval().set_precision(precision)


# ---------------------------------------------------------------- 1. rows of a vector call are the scalar calls
@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", ["SR_4X_tiny", "SR_8X_tiny", "Rescaling_4X_tiny"])
def test_rows_of_a_temperature_vector_equal_the_scalar_calls(name, precision):
    """Row b of ``eps_std=[t0 .. t4]`` holds the bits of the B = 1 call with ``eps_std=t_b``, the same seed and
    ``sample_offset=b`` (tiny nets: the same kernel schedule at every batch size, as in
    test_shards_with_sample_offsets_reproduce_the_full_batch); a constant vector is the scalar call on the batch, zeros are
    ``eps_std=0``; rows 2 and 3 share a temperature but not a sample index, so they differ."""
    cfg, net = _net(name, 11, precision)
    g = torch.Generator().manual_seed(3)
    lr = torch.rand(5, 3, 12, 16, generator=g).cuda()
    with torch.no_grad():
        full = net(lr=lr, eps_std=TAUS, reverse=True, seed=1234)
        for b, t in enumerate(TAUS):
            row = net(lr=lr[b:b + 1].contiguous(), eps_std=t, reverse=True, seed=1234, sample_offset=b)
            assert torch.equal(row, full[b:b + 1]), (b, t)
        # the vector may be a tensor, on the host or on the device, and cache_cond / sample_offset work as with a scalar
        again = net(lr=lr, eps_std=torch.tensor(TAUS).cuda(), reverse=True, seed=1234, cache_cond=True)
        hit = net(lr=lr, eps_std=torch.tensor(TAUS, dtype=torch.float64), reverse=True, seed=1234, cache_cond=True)
        assert torch.equal(again, full) and torch.equal(hit, full)
        tail = net(lr=lr[2:].contiguous(), eps_std=TAUS[2:], reverse=True, seed=1234, sample_offset=2)
        assert torch.equal(tail, full[2:])
        assert torch.equal(net(lr=lr, eps_std=[0.8] * 5, reverse=True, seed=1234), net(lr=lr, eps_std=0.8, reverse=True, seed=1234))
        assert torch.equal(net(lr=lr, eps_std=[0.0] * 5, reverse=True, seed=1234), net(lr=lr, eps_std=0, reverse=True, seed=99))
        same_lr = lr[:1].expand(5, -1, -1, -1).contiguous()
        out = net(lr=same_lr, eps_std=TAUS, reverse=True, seed=1234)
        assert not torch.equal(out[2], out[3])                    # same image, same temperature, another sample index
        # injected eps: the level ignores the vector, as it ignores tau
        from hcflow_amd.config import eps_shapes
        eps = [torch.randn(s, generator=g).cuda() * 0.6 for s in eps_shapes(cfg, 5, 12, 16)]
        assert torch.equal(net(lr=lr, eps_std=TAUS, reverse=True, eps=eps), net(lr=lr, eps_std=0.6, reverse=True, eps=eps))


# ---------------------------------------------------------------- 2. the two-stream split slices the vector
@pytest.mark.parametrize("name", ["SR_4X_tiny", "Rescaling_4X_tiny"])
def test_two_stream_split_gives_each_half_its_slice(name):
    """The default two-stream call (B = 4: two halves on two engines) equals the one-stream call bit for bit, also when a
    sample of the second half leaves the f16 range and is re-run exactly with ITS temperature."""
    cfg, net = _net(name, 11, "f16x3")
    g = torch.Generator().manual_seed(8)
    lr = torch.rand(4, 3, 12, 16, generator=g).cuda()
    taus = [0.2, 0.9, 0.0, 0.6]
    with torch.no_grad():
        net.set_streams(1)
        one = net(lr=lr, eps_std=taus, reverse=True, seed=21)
        assert len(net.engines()) == 1
        net.set_streams(2)
        try:
            two = net(lr=lr, eps_std=taus, reverse=True, seed=21)
            assert len(net.engines()) == 2
            assert torch.equal(one, two)
            bad = lr.clone()
            bad[3, 0, 3, 3] = 9.0e4                               # second half: flagged by the twin engine
            n0 = sum(e.fallback_count() for e in net.engines())
            out = net(lr=bad, eps_std=taus, reverse=True, seed=21)
            assert sum(e.fallback_count() for e in net.engines()) == n0 + 1
            net.set_precision("exact")
            ex = net(lr=bad, eps_std=taus, reverse=True, seed=21)
            net.set_precision("f16x3")
            assert torch.equal(out[3].view(torch.int32), ex[3].view(torch.int32))
            assert torch.equal(out[:3], two[:3])
        finally:
            net.set_streams(2)


# ---------------------------------------------------------------- 3. refusals
def test_refusals():
    from hcflow_amd import _lib, dist
    refused = (_lib.HcfError, ValueError)
    cfg, net = _net("SR_4X_tiny", 11, "f16x3")
    lr = torch.rand(3, 3, 8, 8, device="cuda")
    with torch.no_grad():
        for bad in ([0.5, 0.5], [0.5] * 4, [0.5, -0.1, 0.5], [0.5, float("nan"), 0.5], [0.5, float("inf"), 0.5],
                    torch.full((3, 1), 0.5), torch.tensor([0.5, -1.0, 0.5]).cuda()):
            with pytest.raises(refused):
                net(lr=lr, eps_std=bad, reverse=True, seed=1)
        with pytest.raises(refused):
            dist.sharded_inverse(net, lr, [0.5] * 3, seed=1)
        assert dist.sharded_inverse(net, lr, 0.5, seed=1).shape == (3, 3, 32, 32)
    # the differentiable (taped) inverse: trainable parameters, or frozen ones with an input that requires grad
    with pytest.raises(refused):
        net(lr=lr, eps_std=[0.5] * 3, reverse=True, seed=1)
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(refused):
        net(lr=lr.clone().requires_grad_(True), eps_std=[0.5] * 3, reverse=True, seed=1)
    assert net(lr=lr, eps_std=[0.5] * 3, reverse=True, seed=1).shape == (3, 3, 32, 32)     # frozen and plain: inference


# ---------------------------------------------------------------- 4. SampleStats against float64
def _samples(M, near):
    g = torch.Generator().manual_seed(40 + M + (100 if near else 0))
    if near:
        x = torch.rand(2, 3, 5, 7, generator=g)
        return [(x + 1e-7 * torch.randn(x.shape, generator=g)).clamp(0, 1) for _ in range(M)]
    return [torch.rand(2, 3, 5, 7, generator=g) for _ in range(M)]


def _gate(got, ref, f32):
    """The share of the gate max(8 e32, 2^-23 |ref|) per output that ``got`` uses: e32 = the deviation of the same formula in
    fp32 CPU torch from the float64 result, the floor covers the one fp32 store of the value. <= 1 passes."""
    got, ref, f32 = (torch.as_tensor(v).double().reshape(-1) for v in (got, ref, f32))
    bound = torch.maximum(8 * (f32 - ref).abs(), 2.0 ** -23 * ref.abs())
    err = (got - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    share = float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    return share


@pytest.mark.parametrize("near", [False, True])
@pytest.mark.parametrize("M", [1, 2, 3, 7])
def test_sample_stats_against_float64(M, near):
    from hcflow_amd import metrics
    xs = _samples(M, near)
    st = metrics.SampleStats(2, 5, 7, "cuda")
    for x in xs:
        st.add(x.cuda())
    assert st.count == M
    r = st.result()
    assert r["mean"].dtype == r["std"].dtype == torch.float32 and r["diversity"].dtype == torch.float64
    assert r["mean"].shape == r["std"].shape == (2, 3, 5, 7) and r["diversity"].shape == (2,) and r["diversity"].is_cuda
    stack = torch.stack(xs)
    ref_mean = stack.double().mean(0)
    s_mean = _gate(r["mean"].cpu(), ref_mean, stack.mean(0))
    if M == 1:
        assert torch.equal(r["mean"].cpu(), xs[0])
        assert float(r["std"].abs().max()) == 0.0 and float(r["diversity"].abs().max()) == 0.0
        print("M=1 near=%s: mean uses %.3f of the gate" % (near, s_mean))
        assert s_mean <= 1.0
        return
    s_std = _gate(r["std"].cpu(), stack.double().std(0), stack.std(0))
    ref_div = (stack.double() * 255).std(0).mean(dim=(1, 2, 3))
    f32_div = torch.tensor([metrics.diversity([x[b:b + 1] for x in xs]) for b in range(2)], dtype=torch.float64)
    s_div = _gate(r["diversity"].cpu(), ref_div, f32_div)
    print("M=%d near=%s: share of the gate: mean %.3f, std %.3f, diversity %.3f" % (M, near, s_mean, s_std, s_div))
    assert s_mean <= 1.0 and s_std <= 1.0 and s_div <= 1.0


def test_sample_stats_exact_properties():
    from hcflow_amd import metrics
    xs = [x.cuda() for x in _samples(7, False)]
    # identical samples: std == 0 and mean == x exactly
    st = metrics.SampleStats.like(xs[0])
    for _ in range(5):
        st.add(xs[0])
    r = st.result()
    assert torch.equal(r["mean"], xs[0]) and float(r["std"].abs().max()) == 0.0 and float(r["diversity"].abs().max()) == 0.0
    # an image's results do not depend on the rest of the batch; two runs agree bit for bit
    def run(sel, upto=7):
        s = metrics.SampleStats(len(sel), 5, 7, "cuda")
        for x in xs[:upto]:
            s.add(x[sel].contiguous())
        return s, s.result()
    _, both = run([0, 1])
    _, again = run([0, 1])
    _, alone = run([0])
    _, other = run([1, 0])
    for k in ("mean", "std", "diversity"):
        assert torch.equal(both[k], again[k]), k
        assert torch.equal(both[k][:1], alone[k]), k
        assert torch.equal(both[k][:1], other[k][1:]), k
    # result() after 3 adds, 4 more adds, result() again == a fresh accumulator over all 7
    s, first = run([0, 1], upto=3)
    _, three = run([0, 1], upto=3)
    for x in xs[3:]:
        s.add(x)
    late = s.result()
    for k in ("mean", "std", "diversity"):
        assert torch.equal(first[k], three[k]) and torch.equal(late[k], both[k]), k
    assert s.count == 7 and not torch.equal(first["std"], late["std"])
    # a shape the accumulator was not made for, and an empty one
    with pytest.raises(ValueError):
        s.add(xs[0][:1])
    with pytest.raises(ValueError):
        metrics.SampleStats(1, 5, 7, "cuda").result()


def test_sample_stats_several_blocks_per_image():
    """3 * 19 * 37 = 2109 elements per image: three blocks of the finishing pass, the last one partly filled."""
    from hcflow_amd import metrics
    g = torch.Generator().manual_seed(9)
    xs = [torch.rand(3, 3, 19, 37, generator=g) for _ in range(4)]
    st = metrics.SampleStats(3, 19, 37, "cuda")
    for x in xs:
        st.add(x.cuda())
    r = st.result()
    stack = torch.stack(xs)
    ref_div = (stack.double() * 255).std(0).mean(dim=(1, 2, 3))
    f32_div = torch.tensor([metrics.diversity([x[b:b + 1] for x in xs]) for b in range(3)], dtype=torch.float64)
    shares = (_gate(r["mean"].cpu(), stack.double().mean(0), stack.mean(0)), _gate(r["std"].cpu(), stack.double().std(0), stack.std(0)),
              _gate(r["diversity"].cpu(), ref_div, f32_div))
    print("share of the gate: mean %.3f, std %.3f, diversity %.3f" % shares)
    assert max(shares) <= 1.0
    one = metrics.SampleStats(1, 19, 37, "cuda")
    for x in xs:
        one.add(x[2:3].cuda())
    assert torch.equal(one.result()["diversity"], r["diversity"][2:])


# ---------------------------------------------------------------- 5. evaluate_sweep
def _assert_same(a, b, path=""):
    """Two result dicts of the same samples: "nll", "lpips" and "diversity" bit for bit (fixed-order sums); the PSNR / SSIM
    entries to 1e-12 relative -- each sample's row is bit-reproducible too (fixed-order sums, an image's row independent of its
    batch), so the gate only has to cover the order in which a float64 mean over the samples is taken."""
    assert type(a) is type(b), (path, a, b)
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (path, a.keys(), b.keys())
        for k in a:
            _assert_same(a[k], b[k], "%s/%s" % (path, k))
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, "%s/%d" % (path, i))
    elif path.rsplit("/", 1)[-1] in ("nll", "lpips", "diversity"):
        assert a == b, (path, a, b)
    else:
        assert abs(a - b) <= 1e-12 * abs(b), (path, a, b)


def test_evaluate_sweep_equals_its_defining_scalar_calls():
    """Row r = b * len(heats) + hi of sample s is net(lr=lq[b:b+1], eps_std=heats[hi], seed=seed + s, sample_offset=r): every
    entry equals what those calls give through metrics.psnr_ssim / metrics.diversity / the LPIPS metric, whatever max_batch."""
    from hcflow_amd import metrics
    from hcflow_amd.loader import batched_test_loader, evaluate_batch, evaluate_sweep
    from hcflow_amd.lpips import LPIPS
    from tests.test_loader_cpu import FakeSet
    cfg, net = _net("SR_4X_tiny", 11, "f16x3")
    lp = LPIPS(seed=0).cuda()
    batch = next(iter(batched_test_loader(FakeSet([(12, 16)] * 2), 2)))
    heats, n_sample, seed = [0, 0.5, 0.9], 3, 7
    torch.manual_seed(5)
    got = evaluate_sweep(net, batch, heats, n_sample, scale=4, seed=seed, lpips_fn=lp)
    torch.manual_seed(5)
    small = evaluate_sweep(net, batch, heats, n_sample, scale=4, seed=seed, lpips_fn=lp, max_batch=4)
    _assert_same(got, small)
    torch.manual_seed(5)
    base = evaluate_batch(net, batch, [], 0, scale=4)
    lq, gt = batch["LQ"].cuda(), batch["GT"].cuda()
    worst = 0.0
    with torch.no_grad():
        for b in range(2):
            _assert_same({k: got[b][k] for k in ("nll", "lr")}, base[b], "/%d" % b)
            assert set(got[b].keys()) == {"nll", "lr", 0.0, 0.5, 0.9}
            for hi, heat in enumerate(heats):
                r = b * len(heats) + hi
                samples = [net(lr=lq[b:b + 1], eps_std=heat, seed=seed + s, sample_offset=r, reverse=True, training=False)
                           for s in range(n_sample)]
                want = dict.fromkeys(metrics.KEYS, 0.0)
                want_lp = 0.0
                for sr in samples:
                    m = metrics.psnr_ssim(gt[b:b + 1], sr, 4, 4)[0]
                    for k in metrics.KEYS:
                        want[k] += m[k] / n_sample
                    want_lp += float(lp(2 * gt[b:b + 1] - 1, 2 * sr - 1).double().mean()) / n_sample
                ent = got[b][float(heat)]
                assert set(ent.keys()) == set(metrics.KEYS) | {"lpips", "diversity"}
                for k in metrics.KEYS:
                    assert abs(ent[k] - want[k]) <= 1e-12 * abs(want[k]), (b, heat, k, ent[k], want[k])
                assert abs(ent["lpips"] - want_lp) <= 1e-12 * abs(want_lp), (b, heat, ent["lpips"], want_lp)
                stack = torch.stack([s.cpu() for s in samples])
                ref = float((stack.double() * 255).std(0).mean())
                f32 = metrics.diversity([s.cpu() for s in samples])
                bound = max(8 * abs(f32 - ref), 2.0 ** -23 * abs(ref))
                assert abs(ent["diversity"] - ref) <= bound, (b, heat, ent["diversity"], ref, bound)
                if heat == 0:
                    assert ent["diversity"] == 0.0
                else:
                    assert ent["diversity"] > 0.0
                    worst = max(worst, abs(ent["diversity"] - ref) / bound)
    print("diversity: %.3f of the gate at worst" % worst)
    # without GT only the diversity is left; one sample reports 0, as evaluate_batch does
    no_gt = evaluate_sweep(net, {"LQ": batch["LQ"]}, heats, 1, scale=4, seed=seed)
    assert no_gt[0] == {0.0: {"diversity": 0.0}, 0.5: {"diversity": 0.0}, 0.9: {"diversity": 0.0}}
