"""-m gpu: SR latent encoding -- HCFlowNet_SR.encode (hcf_encode_sr) / decode, hcflow_amd.latent and the rescaling net's
aliases -- against the reference's fixtures (tests/golden/encode_*.npz), the CPU oracle composition (tests/encode_oracle.py) and
the untouched forward / inverse passes. Both conv precisions (conftest.py parametrises only its listed modules, so the modes are
spelled out here). Every test prints the figure it asserts on."""
import pytest
import torch

from hcflow_amd.config import preset, eps_shapes
from tests import encode_oracle as EO
from tests.util import load_golden, params_for, cached_params, t, maxdiff

pytestmark = pytest.mark.gpu
PRECISIONS = ["f16x3", "exact"]
_cache = {}


def _net(cfg, p, precision):
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling
    key = id(p)
    if key not in _cache:
        net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
        net.load_state_dict(p, strict=True)
        for m in net.modules():
            if "ActNorm" in type(m).__name__:
                m.inited = True
        _cache.clear()
        _cache[key] = net.to("cuda:0").eval()
    return _cache[key].set_precision(precision)


def _close(tag, got, ref, rel):
    ref = ref if torch.is_tensor(ref) else t(ref)
    d, tol = maxdiff(got, ref), rel * max(1.0, float(ref.abs().max()))
    print("%s: max|diff| %.3e (gate %.3e)" % (tag, d, tol))
    assert d <= tol, (tag, d, tol)


def _rel(tag, got, ref, rel):
    got, ref = got.detach().cpu().double().reshape(-1), (ref if torch.is_tensor(ref) else t(ref)).detach().cpu().double().reshape(-1)
    d = float(((got - ref).abs() / ref.abs()).max())
    print("%s: max relative diff %.3e (gate %.1e)" % (tag, d, rel))
    assert d <= rel, (tag, d, rel)


# ---------------------------------------------------------------- 1. reference parity
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["encode_sr4_tiny", "encode_sr8_tiny"])
def test_encode_matches_the_reference_fixture(name, precision):
    """z, eps_i within 1e-4 * max(1, max|ref|), logp within 1e-5 relative: the gates tests/test_gpu_nets.py applies to fwd_z,
    fwd_z1/2 and fwd_nll."""
    g = load_golden(name)
    cfg, p = params_for(g)
    net = _net(cfg, p, precision)
    with torch.no_grad():
        z, eps, logp = net.encode(t(g["hr"]).cuda(), noise=t(g["fwd_noise"]).cuda())
        back = net.decode(z, eps)
    assert len(eps) == cfg.L and not z.requires_grad and not logp.requires_grad
    _close(name + " z", z, g["z"], 1e-4)
    for i, e in enumerate(eps):
        _close("%s eps%d" % (name, i), e, g["eps%d" % i], 1e-4)
    _rel(name + " logp", logp, g["logp"], 1e-5)
    _close(name + " decode vs the reference's own reverse_flow", back, g["rt_raw"], 2e-4)


# ---------------------------------------------------------------- 2. oracle parity on fresh inputs
FRESH = [("SR_4X_tiny", 11, 12, 20), ("SR_8X_tiny", 12, 5, 9), ("SR_4X_tiny@K=1,3,2;after=0,3;nb=0,1", 101, 10, 14)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("name,seed,h,w", FRESH)
def test_encode_matches_the_oracle_on_fresh_inputs(name, seed, h, w, with_noise, precision):
    cfg = preset(name)
    p = cached_params(name, seed)
    net = _net(cfg, p, precision)
    g = torch.Generator().manual_seed(100 + seed)
    hr = torch.rand(3, 3, h * cfg.scale, w * cfg.scale, generator=g)
    noise = torch.rand(hr.shape, generator=g) if with_noise else None
    with torch.no_grad():
        z_o, eps_o, logp_o = EO.encode(hr, p, cfg, noise=noise)
        z, eps, logp = net.encode(hr.cuda(), noise=None if noise is None else noise.cuda())
    assert [tuple(e.shape) for e in eps] == [tuple(s) for s in eps_shapes(cfg, 3, h, w)]
    _close("z", z, z_o, 1e-4)
    for i, (a, b) in enumerate(zip(eps, eps_o)):
        _close("eps%d" % i, a, b, 1e-4)
    _rel("logp", logp, logp_o, 1e-5)


# ---------------------------------------------------------------- 3. round trip
ROUND_TRIP = [("SR_4X_tiny", 11, 2, 48, 64), ("SR_8X_tiny", 12, 2, 64, 96), ("SR_DF2K_4X", 21, 2, 160, 160),
              ("SR_CelebA_8X", 22, 2, 160, 160)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,seed,B,H,W", ROUND_TRIP)
def test_decode_of_encode_returns_the_image(name, seed, B, H, W, precision):
    """decode(*encode(hr)[:2]) == hr within 2e-4, the gate of test_rescale_encode_decode_roundtrip_property, on the tiny nets and
    on the full-depth nets (seeded weights)."""
    cfg = preset(name)
    p = cached_params(name, seed)
    net = _net(cfg, p, precision)
    hr = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(7)).cuda()
    with torch.no_grad():
        z, eps, logp = net.encode(hr)
        back = net.decode(z, eps)
    d = maxdiff(back, hr)
    print("round trip %s %s B=%d %dx%d: max|diff| %.3e (gate 2e-4); max|eps| %.2f, z in [%.2f, %.2f]" % (
        name, precision, B, H, W, d, max(float(e.abs().max()) for e in eps), float(z.min()), float(z.max())))
    assert bool(torch.isfinite(logp).all()) and d <= 2e-4


# ---------------------------------------------------------------- 4. consistency with the untouched forward pass
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,seed", [("SR_4X_tiny", 11), ("SR_8X_tiny", 12)])
def test_encode_is_consistent_with_the_forward_pass_and_leaks_no_state(name, seed, precision):
    cfg = preset(name)
    p = cached_params(name, seed)
    net = _net(cfg, p, precision)
    g = torch.Generator().manual_seed(31)
    h, w = 6, 10
    hr = torch.rand(3, 3, h * cfg.scale, w * cfg.scale, generator=g).cuda()
    noise = torch.rand(hr.shape, generator=g).cuda()
    lr_q = torch.rand(3, 3, h, w, generator=g).cuda()
    with torch.no_grad():
        before = net.normal_flow_diracLR(hr, lr_q, noise=noise, return_internals=True)
        inv_before = net(lr=lr_q, eps_std=0.7, reverse=True, seed=5, cache_cond=True)
        z, eps, logp = net.encode(hr, noise=noise)
        inv_after = net(lr=lr_q, eps_std=0.7, reverse=True, seed=5, cache_cond=True)      # the kept cond features were dropped
        after = net.normal_flow_diracLR(hr, lr_q, noise=noise, return_internals=True)
    out_lr, nll, objective, zraw = before
    assert torch.equal(z, zraw)
    assert all(torch.equal(a, b) for a, b in zip(before, after)) and torch.equal(inv_before, inv_after)
    want = logp.detach().cpu().double() + EO.dirac_logp(lr_q, z)
    _rel("objective = logp + dirac", objective, want, 1e-5)


# ---------------------------------------------------------------- 5. per sample, deterministic, stream split
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,seed", [("SR_4X_tiny", 11), ("SR_8X_tiny", 12)])
def test_encode_is_per_sample_deterministic_and_split_invariant(name, seed, precision):
    cfg = preset(name)
    p = cached_params(name, seed)
    net = _net(cfg, p, precision)
    g = torch.Generator().manual_seed(41)
    hr = torch.rand(4, 3, 6 * cfg.scale, 8 * cfg.scale, generator=g).cuda()
    noise = torch.rand(hr.shape, generator=g).cuda()

    def flat(r):
        return [r[0]] + list(r[1]) + [r[2]]
    with torch.no_grad():
        net.set_streams(2)
        try:
            two = flat(net.encode(hr, noise=noise))
            again = flat(net.encode(hr, noise=noise))
            assert len(net.engines()) == 2
            net.set_streams(1)
            one = flat(net.encode(hr, noise=noise))
            single = [flat(net.encode(hr[b:b + 1].contiguous(), noise=noise[b:b + 1].contiguous())) for b in range(4)]
        finally:
            net.set_streams(2)
    assert all(torch.equal(a, b) for a, b in zip(two, again))
    assert all(torch.equal(a, b) for a, b in zip(two, one))
    for b in range(4):
        assert all(torch.equal(a[b:b + 1], s) for a, s in zip(one, single[b])), b


# ---------------------------------------------------------------- 6. overflow re-run
def test_encode_reruns_an_f16_overflow_exactly():
    """The input construction of tests/test_gpu_f16x3.py::test_f16x3_vs_exact_full_size_and_fallback applied to encode: one element
    of the bench-size input pushed beyond the f16 range, the same two assertions (the fallback counter rises by one, the result is
    the exact mode's bit for bit). The element is 1e6 here, not that test's 7e4: in the FORWARD direction the first thing an input
    meets is ActNorm and the invertible 1x1 conv (an orthogonal 12 x 12 mix, |w| < 0.56 for this seed), which leaves at most
    3.9e4 of a 7e4 element in any channel -- no conv input leaves the f16 range and a re-run would be wrong; 1e6 leaves 4.8e5 in
    the coupling net's input half (both figures from the CPU oracle)."""
    cfg = preset("SR_4X_tiny")
    p = cached_params("SR_4X_tiny", 11)
    net = _net(cfg, p, "exact")
    g = torch.Generator().manual_seed(8)
    hr = torch.rand(1, 3, 640, 640, generator=g).cuda()

    def flat(r):
        return [r[0]] + list(r[1]) + [r[2]]
    with torch.no_grad():
        ex = flat(net.encode(hr))
        net.set_precision("f16x3")
        try:
            fa = flat(net.encode(hr))
            for a, b in zip(fa[:-1], ex[:-1]):
                assert maxdiff(a, b) <= 2e-5 * max(1.0, float(b.abs().max()))
            n0 = net.engine().fallback_count()
            big = hr.clone()
            big[0, 1, 7, 9] = 1.0e6                      # -> 4.8e5 at the first coupling net's input: not representable by the f16 hi part
            fb = flat(net.encode(big))
            assert net.engine().fallback_count() == n0 + 1
            net.set_precision("exact")
            eb = flat(net.encode(big))
            assert all(torch.allclose(a, b, rtol=0, atol=0, equal_nan=True) for a, b in zip(fb, eb))      # bit-identical re-run
        finally:
            net.set_precision("exact")


# ---------------------------------------------------------------- 7. latent semantics end to end
@pytest.mark.parametrize("precision", PRECISIONS)
def test_latent_module_end_to_end(precision):
    from hcflow_amd import latent
    cfg = preset("SR_4X_tiny")
    p = cached_params("SR_4X_tiny", 11)
    net = _net(cfg, p, precision)
    g = torch.Generator().manual_seed(51)
    hr = torch.rand(3, 3, 48, 64, generator=g).cuda()
    noise = torch.rand(hr.shape, generator=g).cuda()
    lq = torch.rand(3, 3, 12, 16, generator=g).cuda()
    with torch.no_grad():
        eps, nll = latent.get_encode_z_and_nll(net, lq, hr, noise=noise)
        assert tuple(nll.shape) == (3,)
        for b in range(3):
            _, want = net(hr=hr[b:b + 1].contiguous(), lr=lq[b:b + 1].contiguous(), noise=noise[b:b + 1].contiguous())
            d = abs(float(nll[b]) - float(want)) / abs(float(want))
            print("nll sample %d: %.6f vs %.6f (rel %.2e)" % (b, float(nll[b]), float(want), d))
            assert d <= 1e-5
        _, want_mean = net(hr=hr, lr=lq, noise=noise)
        assert abs(float(nll.mean()) - float(want_mean)) <= 1e-5 * abs(float(want_mean))
        sr0, e0 = latent.get_sr_with_z(net, lq, eps=latent.scale(eps, 0.0))
        assert torch.equal(sr0, net(lr=lq, eps_std=0.0, reverse=True))
        # drawn here: the same seed gives the same image, the draws come back with it, and feeding them again reproduces it
        sr1, e1 = latent.get_sr_with_z(net, lq, heat=0.8, seed=4)
        sr2, e2 = latent.get_sr_with_z(net, lq, heat=0.8, seed=4)
        assert torch.equal(sr1, sr2) and all(torch.equal(a, b) for a, b in zip(e1, e2))
        assert torch.equal(latent.get_sr_with_z(net, lq, eps=e1)[0], sr1)
        assert [tuple(e.shape) for e in e1] == [tuple(s) for s in eps_shapes(cfg, 3, 12, 16)]
        # an interpolation path between two encoded images ends in the two images
        z, eps_i, _ = net.encode(hr)
        path = [net.decode(z[:1], latent.slerp([e[:1] for e in eps_i], [e[1:2] for e in eps_i], tt)) for tt in (0.0, 0.5)]
        assert maxdiff(path[0], hr[:1]) <= 2e-4 and bool(torch.isfinite(path[1]).all())


# ---------------------------------------------------------------- 8. the rescaling net's aliases
@pytest.mark.parametrize("precision", PRECISIONS)
def test_rescaling_encode_decode_aliases(precision):
    cfg = preset("Rescaling_4X_tiny")
    p = cached_params("Rescaling_4X_tiny", 13)
    net = _net(cfg, p, precision)
    hr = torch.rand(2, 3, 96, 128, generator=torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        lr_raw, eps = net.encode(hr)
        back = net.decode(lr_raw, eps)
        lr2, z1, z2 = net.normal_flow_diracLR(hr, clamp=False)
        back2 = net.reverse_flow_diracLR(lr2, None, None, eps_std=1.0, eps=[z2, z1], clamp=False)
    assert torch.equal(lr_raw, lr2) and torch.equal(eps[0], z2) and torch.equal(eps[1], z1) and torch.equal(back, back2)
    d = maxdiff(back, hr)
    print("rescaling round trip max|diff| %.3e (gate 2e-4)" % d)
    assert d <= 2e-4
