"""Host-side checks of sampling with the density (hcf_inverse_logp, HCFlowNet_SR.sample_with_logp): the DEFINITION -- the closed
form the inverse pass accumulates equals the log-density the encode assigns to the unclamped sample -- on the CPU oracle in
float64, the C ABI, and the refusals that are decided before a device is touched."""
import os
import re

import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd.config import preset, eps_shapes
from tests import encode_oracle as EO
from tests import sample_logp_oracle as SO
from tests.util import cached_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the tiny SR presets tests/test_gpu_encode.py parametrises (name, weight seed, h, w), and the LU-decomposed x4 net
PRESETS = [("SR_4X_tiny", 11, 12, 20), ("SR_8X_tiny", 12, 5, 9), ("SR_4X_tiny@K=1,3,2;after=0,3;nb=0,1", 101, 10, 14),
           ("SR_4X_tiny_LU", 14, 6, 10)]


@pytest.mark.parametrize("tau", [0.0, 0.8])
@pytest.mark.parametrize("name,seed,h,w", PRESETS)
def test_closed_form_of_the_inverse_pass_is_the_encode_of_its_sample(name, seed, h, w, tau):
    """logp of ``sample_logp_oracle.inverse_with_logp`` (prior term of the eps used + sum of logscale on the inverse path + the
    data-independent terms) against ``encode_oracle.encode(oracle_inverse(lr, eps, clamp=False), noise=None)``'s, gate 1e-5
    relative to max(|ref|, 1) -- the gate tests/test_gpu_encode.py applies to this quantity. The image is ``O.sr_inverse``'s bit
    for bit (the oracle's inverse runs in float32 only); the encode of it runs in float64, the widest the oracle's blocks take.
    Measured: max relative deviation 1.5e-9 .. 1.6e-8 over the eight cases (the float32 rounding of the inverse pass's terms,
    and of the z1 the encode recovers from the float32 image)."""
    from oracle import hcflow_oracle as O
    cfg = preset(name)
    p = cached_params(name, seed)
    g = torch.Generator().manual_seed(300 + seed)
    B = 2
    lr = torch.rand(B, 3, h, w, generator=g)
    eps = [torch.randn(s, generator=g) * tau for s in eps_shapes(cfg, B, h, w)]
    with torch.no_grad():
        x, logp = SO.inverse_with_logp(lr, p, cfg, eps)
        assert torch.equal(x, O.sr_inverse(lr, p, cfg, 1.0, eps, clamp=False))
        z, eps_back, ref = EO.encode(x.double(), SO.widen(p), cfg, noise=None)
    assert logp.dtype == torch.float64 and ref.dtype == torch.float64 and tuple(logp.shape) == (B,)
    d = float(((logp - ref).abs() / ref.abs().clamp_min(1.0)).max())
    print("%s tau %.1f: logp %s, max relative deviation %.3e (gate 1e-5)" % (name, tau, logp.tolist(), d))
    assert d <= 1e-5
    # the encode finds the latents the sample was made from (what makes the two numbers the same quantity)
    assert float((z - lr).abs().max()) <= 1e-4
    for a, b in zip(eps_back, eps):
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max()))


def test_new_entry_is_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    assert "hcf_inverse_logp" in declared, "include/hcflow.h does not declare hcf_inverse_logp"
    assert "hcf_inverse_logp" in _lib.SYMBOLS and hasattr(lib, "hcf_inverse_logp"), "libhcflow_hip.so does not export hcf_inverse_logp"
    # the definition is stated where the entry is declared
    doc = hdr[:hdr.index("int hcf_inverse_logp(")].rsplit("/*", 1)[1]
    assert "hcf_encode_sr" in doc and "UNCLAMPED" in doc and "Dirac" in doc and "temperature 1" in doc


def test_entry_checks_its_arguments_without_a_device():
    import ctypes as C
    lib = _lib.load()
    n = None
    buf = (C.c_float * 4)()                                        # never dereferenced: every call below is refused first
    ptr = C.cast(buf, C.c_void_p)
    assert lib.hcf_inverse_logp(n, n, n, 0, 0.5, n, 0, 0, n, n, 1, 4, 4, 0, n) == -1
    sr = _lib.Engine(preset("SR_4X_tiny"))                         # hcf_create touches no device
    assert lib.hcf_inverse_logp(sr.handle, ptr, n, 0, 0.5, n, 0, 0, ptr, n, 1, 4, 4, 0, n) == -1      # no out_logp
    assert lib.hcf_inverse_logp(sr.handle, ptr, n, 0, 0.5, n, 0, 0, n, ptr, 1, 4, 4, 0, n) == -1      # no out_hr
    assert lib.hcf_inverse_logp(sr.handle, ptr, n, 0, 0.5, n, 0, -1, ptr, ptr, 1, 4, 4, 0, n) == -1
    assert lib.hcf_inverse_logp(sr.handle, ptr, n, 0, 0.5, n, 0, 0, ptr, ptr, 0, 4, 4, 0, n) == -1
    # a rescaling engine: refused by kind, with a message, before anything else
    rs = _lib.Engine(preset("Rescaling_4X_tiny"))
    rc = lib.hcf_inverse_logp(rs.handle, ptr, n, 0, 0.5, n, 0, 0, ptr, ptr, 1, 4, 4, 0, n)
    assert _lib.ERR_NAMES[rc] == "HCF_ERR_UNSUPPORTED"
    with pytest.raises(_lib.HcfError, match="rescaling engine"):
        _lib.check(rc, rs.handle, "hcf_inverse_logp")
    # an SR engine that was never finalized: a state error, not a crash
    rc = lib.hcf_inverse_logp(sr.handle, ptr, n, 0, 0.5, n, 0, 0, ptr, ptr, 1, 4, 4, 0, n)
    assert _lib.ERR_NAMES[rc] == "HCF_ERR_STATE"


def _cpu_net(name):
    from hcflow_amd.arch import HCFlowNet_SR, HCFlowNet_Rescaling
    from hcflow_amd.params import make_params
    cfg = preset(name)
    net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 1), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    return net.eval()


def test_python_surface_and_refusals_before_a_device_is_touched(monkeypatch):
    from hcflow_amd import latent, loader
    from hcflow_amd.arch import _EngineModule, HCFlowNet_Rescaling
    sr, rs = _cpu_net("SR_4X_tiny"), _cpu_net("Rescaling_4X_tiny")
    assert callable(sr.sample_with_logp) and not hasattr(HCFlowNet_Rescaling, "sample_with_logp") and not hasattr(rs, "sample_with_logp")
    assert callable(latent.sample_nll) and callable(loader.most_likely_samples)

    def no_engine(*a, **k):
        raise AssertionError("the call reached the engine")
    monkeypatch.setattr(_EngineModule, "_engine_for", no_engine)
    lr = torch.rand(2, 3, 4, 4)
    # grad mode on and something requires grad: inference only, and the message names the differentiable route
    with pytest.raises(NotImplementedError, match=r"encode\(.*param_grad=True\)"):
        sr.sample_with_logp(lr, 0.8)
    for prm in sr.parameters():
        prm.requires_grad_(False)
    with pytest.raises(NotImplementedError, match=r"encode\(.*param_grad=True\)"):
        sr.sample_with_logp(lr.clone().requires_grad_(True), 0.8)
    with torch.no_grad():
        with pytest.raises(ValueError):
            sr.sample_with_logp(lr, [0.5, 0.5, 0.5])                # a temperature vector of the wrong length
        with pytest.raises(ValueError):
            loader.most_likely_samples(rs, {"LQ": lr}, 0.8, 2)      # rescaling nets have no density
        with pytest.raises(ValueError):
            loader.most_likely_samples(sr, {"LQ": lr}, 0.8, 0)


def test_loud_failure_without_a_gpu():
    """No CPU fallback: on a host without a GPU the call is an error, as the plain sampling call is."""
    net = _cpu_net("SR_4X_tiny")
    if not torch.cuda.is_available():
        with torch.no_grad(), pytest.raises(_lib.HcfError):
            net.sample_with_logp(torch.rand(1, 3, 4, 4), 0.8)
