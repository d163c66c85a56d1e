"""-m gpu: sampling that returns the density of what it drew -- HCFlowNet_SR.sample_with_logp (hcf_inverse_logp),
latent.sample_nll, loader.most_likely_samples -- against the CPU oracle's encode of the unclamped sample (tests/encode_oracle.py),
the engine's own encode, and the untouched plain sampling call. Both conv precisions (conftest.py parametrises only its listed
modules, so the modes are spelled out here). Every test prints the figure it asserts on.

LR shapes: the smallest that cross each reduction's block boundary. 12 x 20 = 240 pixels: one partly filled 256-pixel block, several
4- and 8-row tiles; 20 x 28 = 560 pixels: three blocks with the last one partial, tiles cut in both directions; 9 x 11 = 99 pixels
for x8: two 64-pixel blocks of the 48-channel tail kernel. The sampler's element grid (256 elements of a sample per block) is
ragged at every one of them."""
import ctypes as C

import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd.config import preset, eps_shapes
from tests import encode_oracle as EO
from tests.util import cached_params, maxdiff

pytestmark = pytest.mark.gpu
PRECISIONS = ["f16x3", "exact"]
_cache = {}


def _net(name, seed, precision):
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling
    cfg = preset(name)
    p = cached_params(name, seed)
    key = (name, seed)
    if key not in _cache:
        net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
        net.load_state_dict(p, strict=True)
        for m in net.modules():
            if "ActNorm" in type(m).__name__:
                m.inited = True
        _cache.clear()
        _cache[key] = net.to("cuda:0").eval()
    return cfg, p, _cache[key].set_precision(precision)


def _rel(tag, got, ref, rel):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().cpu().double().reshape(-1)
    d = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
    print("%s: max relative diff %.3e (gate %.1e)" % (tag, d, rel))
    assert d <= rel, (tag, d, rel)


# ---------------------------------------------------------------- 1. the definition, and the image unchanged
CASES = [("SR_4X_tiny", 11, 12, 20), ("SR_4X_tiny", 11, 20, 28), ("SR_8X_tiny", 12, 9, 11), ("SR_8X_tiny", 12, 12, 20),
         ("SR_4X_tiny_LU", 14, 12, 20), ("SR_4X_tiny_LU", 14, 20, 28)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,seed,h,w", CASES)
def test_logp_is_the_encode_of_the_unclamped_sample_and_the_image_is_unchanged(name, seed, h, w, precision):
    """B = 2, tau in {0, 0.8}, injected eps and device draws. logp against encode_oracle.encode(x_unclamped.cpu(), noise=None)
    at 1e-5 relative to max(|ref|, 1) -- the gate tests/test_gpu_encode.py applies to this quantity -- and against the engine's
    own encode of the same image at 2e-5 (both hold 1e-5 to the same oracle value). The image is the plain call's, bit for bit,
    clamped and unclamped."""
    cfg, p, net = _net(name, seed, precision)
    g = torch.Generator().manual_seed(400 + seed)
    B = 2
    lr = torch.rand(B, 3, h, w, generator=g).cuda()
    for tau in (0.0, 0.8):
        for injected in (True, False):
            eps = [(torch.randn(s, generator=g) * tau).cuda() for s in eps_shapes(cfg, B, h, w)] if injected else None
            kw = dict(eps=eps, seed=17)
            with torch.no_grad():
                x, logp = net.sample_with_logp(lr, tau, clamp=False, **kw)
                xc, logp_c = net.sample_with_logp(lr, tau, **kw)
                plain = net.reverse_flow_diracLR(lr, None, None, eps_std=tau, clamp=False, **kw)
                plain_c = net(lr=lr, eps_std=tau, reverse=True, **kw)
                enc = net.encode(x)[2]
                ref = EO.encode(x.cpu(), p, cfg, noise=None)[2]
            tag = "%s %s %dx%d tau %.1f %s" % (name, precision, h, w, tau, "injected" if injected else "drawn")
            assert tuple(logp.shape) == (B,) and logp.dtype == torch.float32 and not logp.requires_grad
            assert torch.equal(x, plain) and torch.equal(xc, plain_c), tag
            assert torch.equal(xc, x.clamp(0, 1)) and torch.equal(logp, logp_c), tag      # the density is the unclamped sample's
            _rel(tag + " vs the oracle", logp, ref, 1e-5)
            _rel(tag + " vs net.encode", logp, enc, 2e-5)


# ---------------------------------------------------------------- 2. per sample, deterministic, stream split
# 44 x 52 (f16x3): the fused tail's grid at level 0 is 88 tiles of 4 rows per sample, so the 3-sample half of the split runs the
# 8-row tiles (264 > 256 blocks) while the 2-sample half and every single sample run the 4-row ones: the slot layout per 4-row
# band is what keeps the sums bit-equal between them
INDEP = [("SR_4X_tiny", 11, 12, 20), ("SR_8X_tiny", 12, 9, 11), ("SR_4X_tiny", 11, 44, 52)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,seed,h,w", INDEP)
def test_rows_do_not_depend_on_the_batch(name, seed, h, w, precision):
    """Row b of a B = 5 call (two-stream split: 3 + 2) equals the B = 1 call at sample_offset = b, image and logp, bit for bit --
    with a scalar temperature and with a length-5 eps_std vector -- and two identical calls give identical bits."""
    cfg, p, net = _net(name, seed, precision)
    g = torch.Generator().manual_seed(500 + seed)
    lr = torch.rand(5, 3, h, w, generator=g).cuda()
    taus = [0.0, 0.3, 0.8, 1.0, 0.5]
    with torch.no_grad():
        net.set_streams(2)
        for eps_std in (0.8, taus):
            full = net.sample_with_logp(lr, eps_std, seed=23, clamp=False)
            again = net.sample_with_logp(lr, eps_std, seed=23, clamp=False)
            assert len(net.engines()) == 2
            assert torch.equal(full[0], again[0]) and torch.equal(full[1], again[1])
            for b in range(5):
                t_b = eps_std if isinstance(eps_std, float) else taus[b]
                one = net.sample_with_logp(lr[b:b + 1].contiguous(), t_b, seed=23, sample_offset=b, clamp=False)
                same_x, same_lp = torch.equal(full[0][b:b + 1], one[0]), torch.equal(full[1][b:b + 1], one[1])
                print("%s %s %dx%d eps_std %s row %d: image %s, logp %.9g vs %.9g" % (
                    name, precision, h, w, "vector" if isinstance(eps_std, list) else "scalar", b, same_x, float(full[1][b]), float(one[1])))
                assert same_x and same_lp, (b, eps_std)


# ---------------------------------------------------------------- 3. f16-range re-run
def test_a_rerun_sample_gets_the_logp_of_its_exact_pass():
    """An activation beyond the f16 range, made the way tests/test_gpu_encode.py::test_encode_reruns_an_f16_overflow_exactly makes
    one (a single finite element of 1e6, nothing faults) -- here in the injected eps of sample 1 of a batch of 3 at the LAST level
    drawn, so that the split half the prior hands to the conditional coupling nets carries 4.6e5 (beyond the f16 range) while the
    image and every term of the density stay finite (-0.5 eps^2 = -5e11; figures from the CPU oracle; the same element at the
    deepest level would also feed the next level's feature extractor and end in NaN). The fallback counter rises by one, that row's image and logp are the exact mode's bit for bit, and the
    other rows keep the bits of the call without the element."""
    cfg, p, net = _net("SR_4X_tiny", 11, "exact")
    g = torch.Generator().manual_seed(8)
    lr = torch.rand(3, 3, 12, 20, generator=g).cuda()
    eps = [torch.randn(s, generator=g).cuda() * 0.8 for s in eps_shapes(cfg, 3, 12, 20)]
    big = [e.clone() for e in eps]
    big[1][1, 2, 7, 9] = 1.0e6
    with torch.no_grad():
        eb = net.sample_with_logp(lr, 0.8, eps=big, clamp=False)
        net.set_precision("f16x3")
        try:
            clean = net.sample_with_logp(lr, 0.8, eps=eps, clamp=False)
            n0 = net.engine().fallback_count()
            fb = net.sample_with_logp(lr, 0.8, eps=big, clamp=False)
            assert net.engine().fallback_count() == n0 + 1
        finally:
            net.set_precision("exact")
    print("re-run row: logp %.9g (exact %.9g); rows 0, 2: %s vs %s" % (float(fb[1][1]), float(eb[1][1]), fb[1][[0, 2]].tolist(),
                                                                      clean[1][[0, 2]].tolist()))
    assert bool(torch.isfinite(eb[1]).all()) and bool(torch.isfinite(eb[0]).all())
    for a, b in zip(fb, eb):
        assert torch.equal(a[1:2], b[1:2])                              # bit-identical re-run
    for a, b in zip(fb, clean):
        assert torch.equal(a[[0, 2]], b[[0, 2]])


# ---------------------------------------------------------------- 4. kept conditional features
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,seed,h,w,B", [("SR_4X_tiny", 11, 12, 20, 2), ("SR_8X_tiny", 12, 9, 11, 5)])
def test_cache_cond_gives_the_same_logp(name, seed, h, w, B, precision):
    cfg, p, net = _net(name, seed, precision)
    lr = torch.rand(B, 3, h, w, generator=torch.Generator().manual_seed(61)).cuda()
    with torch.no_grad():
        ref = net.sample_with_logp(lr, 0.8, seed=5)
        first = net.sample_with_logp(lr, 0.8, seed=5, cache_cond=True)       # fills the cache
        second = net.sample_with_logp(lr, 0.8, seed=5, cache_cond=True)      # reads it
        plain = net(lr=lr, eps_std=0.8, reverse=True, seed=5, cache_cond=True)      # a plain call reads the same cache
        other = net.sample_with_logp(lr, 0.8, seed=6, cache_cond=True)
    print("logp %s / %s / %s; another seed %s" % (ref[1].tolist(), first[1].tolist(), second[1].tolist(), other[1].tolist()))
    for r in (first, second):
        assert torch.equal(r[0], ref[0]) and torch.equal(r[1], ref[1])
    assert torch.equal(plain, ref[0]) and not torch.equal(other[1], ref[1])


# ---------------------------------------------------------------- 5. refusals
def test_refusals():
    cfg, p, net = _net("SR_4X_tiny", 11, "f16x3")
    lr = torch.rand(2, 3, 12, 20).cuda()
    with pytest.raises(NotImplementedError, match=r"encode\(.*param_grad=True\)"):
        net.sample_with_logp(lr, 0.8)                                  # grad mode on, trainable parameters
    with torch.no_grad():
        x, logp = net.sample_with_logp(lr, 0.8)                        # ... and the same call under no_grad runs
    assert bool(torch.isfinite(logp).all())
    cfg_r, p_r, rs = _net("Rescaling_4X_tiny", 13, "f16x3")
    assert not hasattr(rs, "sample_with_logp")
    with torch.no_grad():
        rs(lr=lr, eps_std=0.8, reverse=True)                           # (builds and finalizes the engine)
    eng = rs.engine()
    out = torch.empty(2, 3, 48, 80, device="cuda")
    lp = torch.full((2,), 7.0, device="cuda")
    rc = eng.lib.hcf_inverse_logp(eng.handle, lr.data_ptr(), None, 0, 0.8, None, 1, 0, out.data_ptr(), lp.data_ptr(), 2, 12, 20, 0,
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert _lib.ERR_NAMES[rc] == "HCF_ERR_UNSUPPORTED"
    with pytest.raises(_lib.HcfError, match="rescaling engine"):
        _lib.check(rc, eng.handle, "hcf_inverse_logp")
    torch.cuda.synchronize()
    assert lp.tolist() == [7.0, 7.0]                                   # nothing was enqueued


# ---------------------------------------------------------------- 6. the helpers above the call
@pytest.mark.parametrize("precision", PRECISIONS)
def test_most_likely_samples_is_the_argmax_over_separate_calls(precision):
    from hcflow_amd import loader
    cfg, p, net = _net("SR_4X_tiny", 11, precision)
    lq = torch.rand(3, 3, 12, 20, generator=torch.Generator().manual_seed(71)).cuda()
    n_sample, seed = 4, 9
    got = loader.most_likely_samples(net, {"LQ": lq.cpu()}, 0.8, n_sample, seed=seed)
    with torch.no_grad():
        draws = [net.sample_with_logp(lq, 0.8, seed=seed + s) for s in range(n_sample)]
    lps = torch.stack([d[1] for d in draws], 0)                        # [M, B]
    index = lps.argmax(dim=0)
    print("logp per draw %s -> index %s (got %s)" % (lps.tolist(), index.tolist(), got["index"].tolist()))
    assert got["index"].dtype == torch.int64 and torch.equal(got["index"], index)
    assert torch.equal(got["logp"], lps.max(dim=0).values)
    for b in range(3):
        assert torch.equal(got["sr"][b], draws[int(index[b])][0][b])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sample_nll_is_the_nll_of_the_forward_pass_on_the_sample(precision):
    """latent.sample_nll(...).mean() with eps taken from an encode equals the nll net(hr=sample, lr=lq) returns without
    dequantisation noise, within the 1e-5 relative tests/test_gpu_encode.py::test_latent_module_end_to_end applies. lq sits on the
    8-bit grid, as a dataset's LQ does, so Quant of the recovered LR latent is lq itself."""
    from hcflow_amd import latent
    cfg, p, net = _net("SR_4X_tiny", 11, precision)
    g = torch.Generator().manual_seed(81)
    lq = (torch.rand(3, 3, 12, 20, generator=g) * 255.).round().div(255.).cuda()
    hr0 = torch.rand(3, 3, 48, 80, generator=g).cuda()
    with torch.no_grad():
        eps = net.encode(hr0)[1]
        sr, eps_back, nll = latent.sample_nll(net, lq, None, eps=eps)
        x = net.sample_with_logp(lq, 1.0, eps=eps, clamp=False)[0]
        _, want = net(hr=x, lr=lq, noise=torch.zeros_like(x))
    assert tuple(nll.shape) == (3,) and nll.dtype == torch.float64 and eps_back is eps and torch.equal(sr, x.clamp(0, 1))
    d = abs(float(nll.mean()) - float(want)) / abs(float(want))
    print("sample_nll mean %.7f vs forward nll %.7f (rel %.2e, gate 1e-5)" % (float(nll.mean()), float(want), d))
    assert d <= 1e-5
    with torch.no_grad():                                              # drawn on the device: no eps comes back, the seed repeats
        a, b = latent.sample_nll(net, lq, 0.8, seed=3), latent.sample_nll(net, lq, 0.8, seed=3)
    assert a[1] is None and torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
