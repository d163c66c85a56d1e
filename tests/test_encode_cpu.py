"""CPU checks of the encode feature: the oracle composition (tests/encode_oracle.py) against the fixtures the REFERENCE wrote
(tests/golden/make_encode_golden.py), the API surface of encode / decode / hcflow_amd.latent, and the argument checks
hcf_encode_sr makes before it touches a device."""
import ctypes as C

import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd.config import preset, eps_shapes
from tests import encode_oracle as EO
from tests.util import load_golden, params_for, t, maxdiff

FIXTURES = ["encode_sr4_tiny", "encode_sr8_tiny"]


@pytest.mark.parametrize("name", FIXTURES)
def test_encode_oracle_matches_the_reference_fixture(name):
    """CPU fp32 against CPU fp32 of the same arithmetic: z, every eps_i and logp within 1e-5 * max(1, max|ref|); the oracle's
    inverse pass fed the encoded latents returns hr + noise / quant within 1e-5."""
    g = load_golden(name)
    cfg, p = params_for(g)
    hr, noise = t(g["hr"]), t(g["fwd_noise"])
    with torch.no_grad():
        z, eps, logp = EO.encode(hr, p, cfg, noise=noise)
        rt = EO.decode(z, eps, p, cfg)
    n = len(eps)
    assert n == cfg.L and [tuple(e.shape) for e in eps] == [tuple(s) for s in eps_shapes(cfg, hr.shape[0], z.shape[2], z.shape[3])]
    for key, got in [("z", z), ("logp", logp)] + [("eps%d" % i, e) for i, e in enumerate(eps)]:
        ref = t(g[key])
        d, tol = maxdiff(got, ref), 1e-5 * max(1.0, float(ref.abs().max()))
        print("%s %s: max|diff| %.3e (tol %.3e)" % (name, key, d, tol))
        assert d <= tol, (key, d, tol)
    x = hr + noise / cfg.quant
    d = maxdiff(rt, x)
    print("%s oracle round trip max|diff| %.3e; reference's own %.3e" % (name, d, maxdiff(t(g["rt_raw"]), x)))
    assert d <= 1e-5
    # the stored log-density is the reference's objective minus its Dirac-LR term
    pixels = hr.shape[2] * hr.shape[3]
    obj = t(g["logp"]).double() + t(g["dirac"]).double()
    assert abs(float((-obj / (0.6931471805599453 * pixels)).mean()) - float(g["nll"])) <= 1e-5 * abs(float(g["nll"]))
    assert maxdiff(EO.dirac_logp(t(g["lr"]), z), t(g["dirac"])) <= 1e-5 * float(t(g["dirac"]).abs().max())


def _net(name):
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling, make_params
    cfg = preset(name)
    net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 1), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    return cfg, net.eval()


def test_encode_decode_surface_and_loud_failure_without_gpu():
    import hcflow_amd
    from hcflow_amd import latent
    assert hcflow_amd.latent is latent
    for name in ("SR_4X_tiny", "SR_8X_tiny", "Rescaling_4X_tiny"):
        cfg, net = _net(name)
        assert callable(net.encode) and callable(net.decode)
        if not torch.cuda.is_available():
            with torch.no_grad(), pytest.raises(_lib.HcfError):
                net.encode(torch.rand(1, 3, 4 * cfg.scale, 4 * cfg.scale))
            with torch.no_grad(), pytest.raises(_lib.HcfError):
                net.decode(torch.rand(1, 3, 4, 4), [torch.zeros(s) for s in eps_shapes(cfg, 1, 4, 4)])
    for fn in ("scale", "lerp", "slerp", "get_encode_z_and_nll", "get_sr_with_z", "dirac_logp"):
        assert callable(getattr(latent, fn))


def test_latent_helpers():
    from hcflow_amd import latent
    cfg = preset("SR_8X_tiny")
    g = torch.Generator().manual_seed(3)
    shapes = eps_shapes(cfg, 3, 4, 6)
    a = [torch.randn(s, generator=g) for s in shapes]
    b = [torch.randn(s, generator=g) for s in shapes]
    for fn in (latent.lerp, latent.slerp):
        for tt in (0.0, 0.3, 1.0):
            out = fn(a, b, tt)
            assert [tuple(o.shape) for o in out] == [tuple(s) for s in shapes] and all(o.dtype == torch.float32 for o in out)
        assert all(torch.equal(x, y) for x, y in zip(fn(a, b, 0.0), a))
        assert all(torch.equal(x, y) for x, y in zip(fn(a, b, 1.0), b))
        assert all(torch.equal(x, y) for x, y in zip(fn(a, a, 0.37), a))
    assert all(torch.equal(x, y) for x, y in zip(latent.scale(a, 1.0), a))
    assert all(float(x.abs().max()) == 0.0 for x in latent.scale(a, 0.0))
    assert all(torch.equal(x, 0.5 * y) for x, y in zip(latent.scale(a, 0.5), a))
    assert all(torch.allclose(x, 0.5 * (y + z), rtol=0, atol=1e-6) for x, y, z in zip(latent.lerp(a, b, 0.5), a, b))   # (fp32 rounding at |x| < 6)
    # slerp is per sample over all levels jointly: for orthogonal unit-norm latents the midpoint keeps the norm (lerp would lose
    # a factor sqrt(2)), and a sample's path does not depend on the other samples of the batch
    def joint_norm(e):
        return sum((x.double() ** 2).reshape(x.shape[0], -1).sum(1) for x in e).sqrt()
    mid = latent.slerp(a, b, 0.5)
    na, nb, nm = joint_norm(a), joint_norm(b), joint_norm(mid)
    assert torch.all(nm > 0.9 * torch.minimum(na, nb)) and torch.all(nm < 1.1 * torch.maximum(na, nb))
    assert torch.all(joint_norm(latent.lerp(a, b, 0.5)) < 0.8 * torch.minimum(na, nb))
    one = latent.slerp([x[1:2] for x in a], [x[1:2] for x in b], 0.5)
    assert all(torch.allclose(x[1:2], y, rtol=0, atol=1e-6) for x, y in zip(mid, one))
    # the Dirac term: zero distance leaves the normalisation constant alone
    z = torch.rand(2, 3, 4, 6, generator=g)
    lq = (torch.clamp(z, 0, 1) * 255.).round() / 255.
    want = -0.5 * (-12.0 + 1.8378770664093453) * 3 * 4 * 6
    assert torch.allclose(latent.dirac_logp(lq, z), torch.full((2,), want, dtype=torch.float64))
    assert maxdiff(latent.dirac_logp(lq * 0.5, z), EO.dirac_logp(lq * 0.5, z)) <= 1e-9 * float(EO.dirac_logp(lq * 0.5, z).abs().max())


def test_hcf_encode_sr_rejects_bad_calls_before_touching_a_device():
    """A rescaling engine, a wrong eps count and a ragged size are refused by the argument checks -- on engines that were never
    finalised (hcf_create touches no device), so no device call can have been made."""
    lib = _lib.load()
    buf = torch.zeros(2 * 3 * 32 * 32)
    ptr = C.c_void_p(buf.data_ptr())
    arr3 = (C.c_void_p * 3)(ptr, ptr, ptr)
    rs = _lib.Engine(preset("Rescaling_4X_tiny"))
    rc = lib.hcf_encode_sr(rs.handle, ptr, None, ptr, arr3, 2, ptr, 1, 16, 16, 0, None)
    assert _lib.ERR_NAMES[rc] == "HCF_ERR_STATE" and b"rescaling engine" in lib.hcf_last_error(rs.handle)
    sr = _lib.Engine(preset("SR_4X_tiny"))
    for n in (1, 3):
        rc = lib.hcf_encode_sr(sr.handle, ptr, None, ptr, arr3, n, ptr, 1, 16, 16, 0, None)
        assert _lib.ERR_NAMES[rc] == "HCF_ERR_ARG" and b"n_eps" in lib.hcf_last_error(sr.handle)
    rc = lib.hcf_encode_sr(sr.handle, ptr, None, ptr, arr3, 2, ptr, 1, 18, 16, 0, None)
    assert _lib.ERR_NAMES[rc] == "HCF_ERR_SHAPE" and b"divisible" in lib.hcf_last_error(sr.handle)
    sr8 = _lib.Engine(preset("SR_8X_tiny"))
    assert _lib.ERR_NAMES[lib.hcf_encode_sr(sr8.handle, ptr, None, ptr, arr3, 2, ptr, 1, 16, 16, 0, None)] == "HCF_ERR_ARG"
    # a well-formed call on an engine without weights stops at the state check (nothing was finalised)
    rc = lib.hcf_encode_sr(sr.handle, ptr, None, ptr, arr3, 2, ptr, 1, 16, 16, 0, None)
    assert _lib.ERR_NAMES[rc] == "HCF_ERR_STATE" and b"hcf_finalize" in lib.hcf_last_error(sr.handle)
    with pytest.raises(_lib.HcfError):
        _lib.check(rc, sr.handle, "hcf_encode_sr")
