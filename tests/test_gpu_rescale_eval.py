"""-m gpu: the rescaling family's test loop and codec surface -- metrics.quantize / metrics.from_image (hcf_image_codec.hip) bit for
bit against numpy / torch on the CPU, HCFlowNet_Rescaling.downscale / upscale as compositions, the loader's evaluate_* functions
on a rescaling net against the same numbers written out from public calls, and the pipeline against the reference's recorded
tensors. Expected values come from the CPU or the recorded fixtures, never from the code under test."""
import functools

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd import metrics as M
from tests.test_rescale_eval_cpu import BOUNDARY_CAP, near_rounding_boundary
from tests.util import load_golden, params_for, t, maxdiff, cached_params

pytestmark = pytest.mark.gpu

NETS = ["net_rescale_tiny", "net_rescale_tiny_lu"]
_nets = {}


def build_net(name, precision):
    """The fixture's seeded tiny rescaling net in eval() mode (tests/test_gpu_nets.py: build_net)."""
    from hcflow_amd import HCFlowNet_Rescaling
    if name not in _nets:
        cfg, p = params_for(load_golden(name))
        net = HCFlowNet_Rescaling(opt=cfg.to_opt(), step=0)
        net.load_state_dict(p, strict=True)
        for m in net.modules():
            if "ActNorm" in type(m).__name__:
                m.inited = True
        _nets[name] = net.to("cuda:0").eval()
    return _nets[name].set_precision(precision)


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def assert_bit_equal(got, want):
    """float32 tensors equal as bit patterns; where ``want`` is NaN, ``got`` is NaN (a NaN's payload is not the test's business)."""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = (bits(got) != bits(want)) & ~nan
    assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])


def ulp_moved(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return x


@functools.lru_cache(maxsize=None)
def value_pool(with_nan=True):
    """Every value class of the quantiser: the 256 grid points k / 255 and the half-way points (k + 0.5) / 255, each moved by 0,
    +-1 and +-2 ulp; values outside [0, 1]; -0.0, denormals, +-inf and (optionally) NaN."""
    k = np.arange(256, dtype=np.float32)
    grid, half = k / np.float32(255.0), (k + np.float32(0.5)) / np.float32(255.0)
    vals = [ulp_moved(v, d) for v in (grid, half) for d in (0, 1, -1, 2, -2)]
    extra = [-1.0, -1e-3, -0.5 / 255, 1.0 + 1e-6, 1.0001, 1.5, 2.0, 255.0, -255.0, 1e30, -1e30, 3.4e38, -0.0, 0.0, 1e-45, -1e-45, 1e-39,
             -1e-39, 1.1754942e-38, np.inf, -np.inf]
    if with_nan:
        extra += [np.nan, -np.nan]
    return np.concatenate(vals + [np.array(extra, dtype=np.float32)]).astype(np.float32)


def pool_tensor(shape, with_nan=True, shift=0):
    """``shape`` filled from the value pool (rotated by ``shift``, repeated as needed)."""
    pool = np.roll(value_pool(with_nan), -shift)
    return torch.from_numpy(np.resize(pool, int(np.prod(shape))).reshape(shape).copy())


def quant_cpu(x):
    return (torch.clamp(x, 0, 1) * 255.).round() / 255.                  # Basic.Quant.forward, on the CPU


def image_cpu(x):
    """np.round(np.clip(x, 0, 1) * 255).astype(np.uint8) in BGR HWC order (util.tensor2img); a NaN is byte 0 (include/hcflow.h)."""
    a = np.nan_to_num(x.numpy(), nan=0.0, posinf=np.inf, neginf=-np.inf)
    q = np.round(np.clip(a, 0, 1) * 255).astype(np.uint8)
    return np.ascontiguousarray(q[:, ::-1].transpose(0, 2, 3, 1))


def whole(x):
    return x


def quantize_inputs():
    """(label, base CPU tensor, view): the caller's tensor is ``view(base)`` on either device (a view taken AFTER the copy keeps
    its offset into the allocation): contiguous shapes on both kernel forms, offset slices, a channels-last tensor."""
    return [("1x1", pool_tensor((1, 3, 1, 1), shift=7), whole), ("5x7", pool_tensor((2, 3, 5, 7), shift=300), whole),
            ("33x65", pool_tensor((1, 3, 33, 65)), whole), ("32x36 quads", pool_tensor((1, 3, 32, 36)), whole),
            ("two blocks of quads", pool_tensor((2, 3, 40, 52), shift=11), whole),
            ("slice of odd size", pool_tensor((3, 3, 5, 7), shift=1000), lambda x: x[1:]),
            ("slice of even size", pool_tensor((3, 3, 6, 10), shift=1500), lambda x: x[1:]),
            ("channels last", pool_tensor((2, 3, 6, 10), shift=2000), lambda x: x.contiguous(memory_format=torch.channels_last)),
            # H * W a multiple of 4 on a base that is not 16-byte aligned
            ("offset view", pool_tensor((1 + 2 * 3 * 8 * 10,), shift=600), lambda x: x[1:].view(2, 3, 8, 10))]


# ---------------------------------------------------------------- 1. quantize
def test_quantize_is_bit_equal_to_the_reference_expression():
    assert value_pool().size >= 2560 and not cases_are_trivial()
    for label, base, view in quantize_inputs():
        x, xd = view(base), view(base.cuda())
        assert xd.stride() == x.stride() and xd.storage_offset() == x.storage_offset(), label
        q = M.quantize(xd)
        assert q.is_contiguous() and q.dtype == torch.float32 and tuple(q.shape) == tuple(x.shape), label
        assert_bit_equal(q, quant_cpu(x.contiguous()))
        q2, img = M.quantize(xd, image=True)
        assert_bit_equal(q2, quant_cpu(x.contiguous()))
        assert img.dtype == torch.uint8 and tuple(img.shape) == (x.shape[0], x.shape[2], x.shape[3], 3), label
        assert np.array_equal(img.cpu().numpy(), image_cpu(x.contiguous())), label
        # the image holds q's integers: q * 255 is exact (NaN aside)
        back = img.cpu().permute(0, 3, 1, 2).flip(1).float()
        ok = ~torch.isnan(x)
        assert torch.equal((q2.cpu() * 255.)[ok], back[ok]), label


def cases_are_trivial():
    """The case list must reach both kernel forms: H * W a multiple of 4 on an aligned base, and not."""
    hw = [view(base).shape[2] * view(base).shape[3] for _, base, view in quantize_inputs()]
    return not (any(v % 4 == 0 for v in hw) and any(v % 4 for v in hw))


def test_quantize_image_is_tensor2img_and_the_pair_metrics_image():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(3, 3, 16, 20, generator=g) * 1.4 - 0.2                        # some values beyond both ends
    n = value_pool(False).size
    x.view(-1)[torch.randperm(x.numel(), generator=g)[:n]] = pool_tensor((n,), with_nan=False)      # and every special value
    ref = torch.rand(3, 3, 16, 20, generator=g)
    pm = M.PairMetrics()
    rows, want = pm.compare(pm.embed(ref.cuda(), 0, 0), x.cuda(), image=True)
    q, img = M.quantize(x.cuda(), image=True)
    assert torch.equal(img, want)
    assert np.array_equal(img.cpu().numpy(), image_cpu(x))
    assert_bit_equal(q, quant_cpu(x))
    # image only, q only, and the caller's own tensors filled in place
    xd = x.cuda()
    only = torch.full((3, 16, 20, 3), 7, dtype=torch.uint8, device="cuda")
    _lib.launch("hcf_metric_quantize", xd.device, xd, 3, 16, 20, None, only)
    assert torch.equal(only, want)
    out = torch.full((3, 3, 16, 20), -5.0, device="cuda")
    image_out = torch.zeros(3, 16, 20, 3, dtype=torch.uint8, device="cuda")
    r = M.quantize(x.cuda(), out=out, image_out=image_out)
    assert r[0] is out and r[1] is image_out and torch.equal(out, q) and torch.equal(image_out, want)
    assert M.quantize(x.cuda(), out=out) is out
    for bad in (dict(out=out[:1]), dict(out=out.double()), dict(image_out=image_out.float()), dict(image_out=image_out[:, :, :, :2])):
        with pytest.raises(_lib.HcfError):
            M.quantize(x.cuda(), **bad)
    for bad in (x.cuda().double(), x.cuda()[:, :2], x.cuda()[0], x.cuda()[:0]):
        with pytest.raises(_lib.HcfError):
            M.quantize(bad)


# ---------------------------------------------------------------- 2. from_image
def image_inputs():
    g = torch.Generator().manual_seed(9)

    def rnd(*shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    all256 = torch.stack([torch.arange(256)[torch.randperm(256, generator=g)] for _ in range(3)], -1).to(torch.uint8).view(1, 16, 16, 3)
    return [("1x1", rnd(1, 1, 1, 3), whole), ("5x7", rnd(2, 5, 7, 3), whole), ("33x65", rnd(1, 33, 65, 3), whole),
            ("all 256 values", all256, whole), ("two blocks of quads", rnd(2, 40, 52, 3), whole),
            ("slice of odd size", rnd(3, 5, 7, 3), lambda x: x[1:]), ("planar storage", rnd(2, 3, 6, 10), lambda x: x.permute(0, 2, 3, 1)),
            ("offset view", rnd(1 + 2 * 8 * 10 * 3), lambda x: x[1:].view(2, 8, 10, 3))]


def test_from_image_bits_and_the_round_trip():
    for label, base, view in image_inputs():
        u8 = view(base)
        want = np.ascontiguousarray((u8.contiguous().numpy().astype(np.float32) / 255.)[..., ::-1].transpose(0, 3, 1, 2))
        ud = view(base.cuda())
        assert ud.stride() == u8.stride() and ud.storage_offset() == u8.storage_offset(), label
        x = M.from_image(ud)
        assert x.is_contiguous() and tuple(x.shape) == want.shape, label
        assert_bit_equal(x, want)
        q, back = M.quantize(x, image=True)
        assert torch.equal(back.cpu(), u8.contiguous()), label               # stored images are fixed points
        assert_bit_equal(q, want)
    u8 = image_inputs()[3][1]
    assert all(len(torch.unique(u8[..., c])) == 256 for c in range(3))
    out = torch.empty(1, 3, 16, 16, device="cuda")
    assert M.from_image(u8.cuda(), out=out) is out and torch.equal(out, M.from_image(u8.cuda()))
    for bad in (u8.cuda().float(), u8.cuda()[..., :2], u8.cuda()[0], u8.cuda()[:0]):
        with pytest.raises(_lib.HcfError):
            M.from_image(bad)
    with pytest.raises(_lib.HcfError):
        M.from_image(u8.cuda(), out=out.double())


# ---------------------------------------------------------------- 3. downscale / upscale
def psnr64(a, b):
    mse = float(((a.detach().cpu().double() - b.detach().cpu().double()) ** 2).mean())
    return float("inf") if mse == 0 else 10 * np.log10(1.0 / mse)


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", NETS)
def test_downscale_and_upscale_are_compositions(name, precision):
    net = build_net(name, precision)
    hr = torch.rand(2, 3, 32, 40, generator=torch.Generator().manual_seed(21)).cuda()
    try:
        with torch.no_grad():
            lr_hat, z1, z2 = net(hr=hr, reverse=False)
            q, u8 = M.quantize(lr_hat, image=True)
            got = net.downscale(hr, image=True)
            assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, (q, u8, z1, z2)))
            got3 = net.downscale(hr)
            assert len(got3) == 3 and all(torch.equal(a, b) for a, b in zip(got3, (q, z1, z2)))
            assert_bit_equal(q, quant_cpu(lr_hat.cpu()))
            for tau in (0.0, 0.8, torch.tensor([0.0, 0.8]), [0.3, 0.0]):
                want = net(lr=M.from_image(u8), z=None, u=None, eps_std=tau, reverse=True, seed=17)
                assert torch.equal(net.upscale(u8, eps_std=tau, seed=17), want), tau
                assert torch.equal(net.upscale(q, eps_std=tau, seed=17), want), tau          # the image and the tensor are one LR
            raw = net.upscale(u8, eps_std=0.8, seed=17, clamp=False, cache_cond=True)
            assert torch.equal(raw.clamp(0, 1), net.upscale(u8, eps_std=0.8, seed=17))
            back = net.upscale(net.downscale(hr)[0], eps_std=0)
            print("%s %s: codec round trip at heat 0, PSNR %.2f dB (random tiny weights: a record, not a gate)"
                  % (name, precision, psnr64(back, hr)))
        # inference only: a gradient wanted by hr or by a parameter is refused while grad mode is on
        with pytest.raises(NotImplementedError):
            net.downscale(hr)                                                # the parameters require grad
        flags = {k: p.requires_grad for k, p in net.named_parameters()}
        for p in net.parameters():
            p.requires_grad_(False)
        try:
            with pytest.raises(NotImplementedError):
                net.downscale(hr.clone().requires_grad_(True))
            assert torch.equal(net.downscale(hr)[0], q)                     # nothing wants a gradient: grad mode alone is fine
        finally:
            for k, p in net.named_parameters():
                p.requires_grad_(flags[k])
    finally:
        net.set_precision("exact")


# ---------------------------------------------------------------- 4. evaluate_batch
def rescale_batch(B=2, H=64, W=80, seed=31):
    g = torch.Generator().manual_seed(seed)
    return {"GT": torch.rand(B, 3, H, W, generator=g), "LQ": torch.rand(B, 3, H // 4, W // 4, generator=g)}


def written_out(net, batch, heats, n_sample, seed, lpips_fn=None):
    """evaluate_batch on a rescaling net, from public calls: forward pass, quantize, the inverse from lr_q per heat and sample,
    PairMetrics.embed / compare, metrics.diversity, the mean of z1."""
    gt = batch["GT"].cuda()
    B = gt.shape[0]
    pm = M.PairMetrics()
    res = [dict() for _ in range(B)]
    with torch.no_grad():
        lr_hat, z1, _ = net(hr=gt, reverse=False)
        lr_q = M.quantize(lr_hat)
        for b in range(B):
            res[b]["nll"] = float(z1[b:b + 1].mean())
        if "LQ" in batch:
            rows = pm.compare(pm.embed(batch["LQ"].cuda(), 0, 0), lr_q).cpu().tolist()
            for b in range(B):
                res[b]["lr"] = dict(zip(M.KEYS[:4], rows[b][:4]))
        ref = pm.embed(gt, 4, 4)
        for hi, heat in enumerate(heats):
            samples = [net(lr=lr_q, z=None, u=None, eps_std=heat, reverse=True, training=False, seed=seed + 1000 * hi + s, cache_cond=True)
                       for s in range(n_sample)]
            rows = torch.stack([pm.compare(ref, sr) for sr in samples], 0).mean(dim=0).cpu().tolist()
            for b in range(B):
                ent = dict(zip(M.KEYS, rows[b]))
                ent["diversity"] = M.diversity([s[b:b + 1] for s in samples]) if n_sample > 1 else 0.0
                res[b][float(heat)] = ent
    return res, lr_q


def same_numbers(a, b):
    """dicts of floats equal with ==, NaN matching NaN"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_numbers(a[k], b[k]) for k in a)
    return type(a) is float and type(b) is float and (a == b or (a != a and b != b))


@pytest.mark.parametrize("name", NETS)
def test_evaluate_batch_on_a_rescaling_net_equals_its_parts(name):
    from hcflow_amd.loader import evaluate_batch
    net = build_net(name, "f16x3")
    try:
        batch = rescale_batch()
        heats, n_sample, seed = [0.0, 0.7], 2, 5
        got = evaluate_batch(net, batch, heats, n_sample=n_sample, scale=4, seed=seed)
        want, _ = written_out(net, batch, heats, n_sample, seed)
        assert len(got) == 2
        for b in range(2):
            assert set(got[b]) == {"nll", "lr", 0.0, 0.7} and set(got[b][0.7]) == set(M.KEYS) | {"diversity"}
            assert same_numbers(got[b], want[b]), (b, got[b], want[b])
            assert all(np.isfinite(v) for v in got[b]["lr"].values()) and all(np.isfinite(v) for v in got[b][0.7].values())
            assert got[b][0.0]["diversity"] == 0.0 and got[b][0.7]["diversity"] > 0.0
        # an image's numbers do not depend on the batch: fed alone it gives the same "nll", "lr" and heat-0 entry; image 0 (whose
        # draws are those of sample index 0 either way) also the same sampled entry
        for b in range(2):
            alone = evaluate_batch(net, {k: v[b:b + 1] for k, v in batch.items()}, heats, n_sample=n_sample, scale=4, seed=seed)[0]
            for k in ("nll", "lr", 0.0) + ((0.7,) if b == 0 else ()):
                assert same_numbers(alone[k], got[b][k]), (b, k, alone[k], got[b][k])
        no_lq = evaluate_batch(net, {"GT": batch["GT"]}, [0.0], n_sample=1, scale=4, seed=seed)
        assert all(set(e) == {"nll", 0.0} for e in no_lq) and all(no_lq[b]["nll"] == got[b]["nll"] for b in range(2))
        assert same_numbers(no_lq[0][0.0], {**{k: got[0][0.0][k] for k in M.KEYS}, "diversity": 0.0})
        with pytest.raises(ValueError, match="GT"):
            evaluate_batch(net, {"LQ": batch["LQ"]}, heats, n_sample=1, scale=4)
    finally:
        net.set_precision("exact")


def test_evaluate_batch_on_an_sr_net_is_unchanged():
    """The SR branch restated from public calls (HCFlowSRModel.test(): NLL pass of (GT, LQ), samples from the LQ)."""
    from hcflow_amd import HCFlowNet_SR, preset
    from hcflow_amd.loader import evaluate_batch
    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(cached_params("SR_4X_tiny", 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(41)
    batch = {"LQ": torch.rand(2, 3, 16, 20, generator=g), "GT": torch.rand(2, 3, 64, 80, generator=g)}
    noise = torch.rand(2, 3, 64, 80, generator=g).cuda()
    heats, n_sample, seed = [0.0, 0.7], 2, 5
    got = evaluate_batch(net, batch, heats, n_sample=n_sample, scale=4, seed=seed, noise=noise)
    lq, gt = batch["LQ"].cuda(), batch["GT"].cuda()
    pm = M.PairMetrics()
    with torch.no_grad():
        lr_hat, _, obj, _ = net.normal_flow_diracLR(gt, lq, noise=noise, return_internals=True)
        lr_rows = pm.compare(pm.embed(lq, 0, 0), lr_hat).cpu().tolist()
        ref = pm.embed(gt, 4, 4)
        for b in range(2):
            assert set(got[b]) == {"nll", "lr", 0.0, 0.7}
            assert got[b]["nll"] == -float(obj[b].double()) / (0.6931471805599453 * 64 * 80)
            assert same_numbers(got[b]["lr"], dict(zip(M.KEYS[:4], lr_rows[b][:4])))
        for hi, heat in enumerate(heats):
            samples = [net(lr=lq, z=None, u=None, eps_std=heat, reverse=True, training=False, seed=seed + 1000 * hi + s) for s in range(n_sample)]
            rows = torch.stack([pm.compare(ref, sr) for sr in samples], 0).mean(dim=0).cpu().tolist()
            for b in range(2):
                want = dict(zip(M.KEYS, rows[b]))
                want["diversity"] = M.diversity([s[b:b + 1] for s in samples])
                assert same_numbers(got[b][heat], want), (b, heat, got[b][heat], want)


# ---------------------------------------------------------------- 5. evaluate_sweep
@pytest.mark.parametrize("max_batch", [16, 3])
def test_evaluate_sweep_rows_on_a_rescaling_net(max_batch):
    from hcflow_amd.loader import evaluate_sweep, evaluate_batch
    net = build_net("net_rescale_tiny", "f16x3")
    try:
        batch = rescale_batch()
        heats, n_sample, seed = [0.0, 0.7], 2, 5
        got = evaluate_sweep(net, batch, heats, n_sample, scale=4, seed=seed, max_batch=max_batch)
        base = evaluate_batch(net, batch, [], 0, scale=4)
        gt = batch["GT"].cuda()
        pm = M.PairMetrics()
        with torch.no_grad():
            lr_q = M.quantize(net(hr=gt, reverse=False)[0])
            for b in range(2):
                assert set(got[b]) == {"nll", "lr", 0.0, 0.7}
                assert same_numbers({k: got[b][k] for k in ("nll", "lr")}, base[b])
                ref = pm.embed(gt[b:b + 1], 4, 4)
                for hi, heat in enumerate(heats):
                    r = b * len(heats) + hi
                    samples = [net(lr=lr_q[b:b + 1], eps_std=heat, seed=seed + s, sample_offset=r, reverse=True, training=False)
                               for s in range(n_sample)]
                    rows = [pm.compare(ref, sr).cpu().tolist()[0] for sr in samples]
                    want = dict(zip(M.KEYS, [(u + v) / 2 for u, v in zip(*rows)]))        # the float64 mean of two is exact
                    stats = M.SampleStats.like(samples[0])
                    for sr in samples:
                        stats.add(sr)
                    want["diversity"] = float(stats.result()["diversity"][0])
                    assert same_numbers(got[b][heat], want), (b, heat, got[b][heat], want)
                    assert (want["diversity"] > 0.0) == (heat > 0)
    finally:
        net.set_precision("exact")


# ---------------------------------------------------------------- 6. evaluate_sample_set
def test_evaluate_sample_set_on_a_rescaling_net():
    from hcflow_amd.loader import evaluate_sample_set
    from hcflow_amd.lpips import LPIPS, LPIPSMap
    mapper = LPIPSMap(LPIPS(seed=0).cuda())
    net = build_net("net_rescale_tiny", "f16x3")
    try:
        batch = rescale_batch(B=1, H=32, W=48, seed=51)
        heats, n_sample, seed = [0.0, 0.7], 2, 5
        got = evaluate_sample_set(net, batch, heats, n_sample, mapper, seed=seed)
        gt = batch["GT"].cuda()
        with torch.no_grad():
            lr_q = M.quantize(net(hr=gt, reverse=False)[0])
            for hi, heat in enumerate(heats):
                acc = mapper.sample_set(gt, normalize=True)
                for s in range(n_sample):
                    acc.add(net(lr=lr_q, z=None, u=None, eps_std=heat, reverse=True, training=False, cache_cond=True,
                                seed=seed + 1000 * hi + s))
                r = acc.result()
                lp = r["lpips"].double().cpu().tolist()
                ent = got[0][heat]
                assert set(ent) == {"lpips", "lpips_best", "local_best", "score"}
                assert ent["lpips"] == lp[0][0] / 2 + lp[1][0] / 2
                assert ent["lpips_best"] == float(r["global_best"][0]) and ent["local_best"] == float(r["local_best"][0])
                assert ent["score"] == float(r["score"][0])
    finally:
        net.set_precision("exact")


# ---------------------------------------------------------------- 7. against the reference
@pytest.mark.parametrize("name", NETS)
def test_quantize_reproduces_the_reference_quantization_pairs(name):
    """(a) the reference's recorded Quantization input -> its recorded output, bit for bit."""
    g = load_golden(name)
    assert_bit_equal(M.quantize(t(g["fwd_lr"]).cuda()), g["rt_lrq"])
    q, img = M.quantize(t(g["rt_lrq"]).cuda(), image=True)
    assert_bit_equal(q, g["rt_lrq"])                                             # a quantised tensor is a fixed point
    assert_bit_equal(M.from_image(img), g["rt_lrq"])


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", NETS)
def test_pipeline_against_the_reference(name, precision):
    """(b) downscale(hr) against the reference's quantised LR^: equal wherever the reference's value is not within 1e-3 of a
    rounding boundary (at most 1 % of the elements: tests/test_rescale_eval_cpu.py holds the fixtures to that cap).
    (c) the inverse at heat 0 from the REFERENCE's quantised LR^ against its recorded HR^, within test_gpu_nets.py's gate for the
    rescaling fixtures (1e-4 on the clamped output, 1e-4 * max(1, max|raw|) on the raw one)."""
    g, e = load_golden(name), load_golden("rescale_eval_tiny")
    net = build_net(name, precision)
    try:
        with torch.no_grad():
            lr_q, u8, z1, z2 = net.downscale(t(g["hr"]).cuda(), image=True)
            skip = near_rounding_boundary(g["fwd_lr"])
            assert skip.mean() <= BOUNDARY_CAP
            same = lr_q.cpu().numpy() == g["rt_lrq"]
            print("%s %s: %d of %d elements left out, %d of them differ" % (name, precision, skip.sum(), skip.size, (~same & skip).sum()))
            assert same[~skip].all(), (int((~same & ~skip).sum()), lr_q.cpu().numpy()[~same & ~skip][:4], g["rt_lrq"][~same & ~skip][:4])
            assert maxdiff(z1, g["fwd_z1"]) <= 1e-4 * max(1.0, float(np.abs(g["fwd_z1"]).max()))
            for b in range(z1.shape[0]):
                assert abs(float(z1[b:b + 1].mean()) - float(e[name + "_z1_mean_b1"][b])) <= 1e-4
            ref_q = t(g["rt_lrq"]).cuda()
            out = net.upscale(ref_q, eps_std=0.0)
            assert maxdiff(out, e[name + "_q0_out"]) <= 1e-4
            raw = net.upscale(ref_q, eps_std=0.0, clamp=False)
            assert maxdiff(raw, e[name + "_q0_raw"]) <= 1e-4 * max(1.0, float(np.abs(e[name + "_q0_raw"]).max()))
            # the stored image is the same LR
            assert torch.equal(net.upscale(M.quantize(ref_q, image=True)[1], eps_std=0.0), out)
    finally:
        net.set_precision("exact")
