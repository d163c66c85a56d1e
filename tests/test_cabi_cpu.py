"""CPU checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/hcflow.h declares, and agrees with the Python side (and hence with the reference, see
tests/golden/make_golden.py::build) on the state_dict key/shape table. No compute calls."""
import os
import re

import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd.config import NetConfig, preset, param_spec, param_count, eps_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = ["SR_DF2K_4X", "SR_CelebA_8X", "Rescaling_DF2K_4X", "SR_4X_tiny", "SR_8X_tiny", "Rescaling_4X_tiny"]


def test_header_symbols_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = sorted(set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), "libhcflow_hip.so does not export %s" % name
    assert sorted(_lib.SYMBOLS) == declared


def test_backward_op_entries_reject_null_tensors_without_a_device():
    """The per-op entries of the backward kernels check their arguments before they touch the device."""
    lib = _lib.load()
    n = None
    assert lib.hcf_op_step_forward_backward(n, n, n, n, n, n, n, n, 1, 8, 4, 4, 8, 0, 4, n, n, 1.0, n) == -1
    assert lib.hcf_op_step_inverse_backward(n, n, n, n, n, n, n, n, n, n, 1, 8, 4, 4, 8, 0, 4, n, n, n, n) == -1
    assert lib.hcf_op_prior_backward(0, n, n, n, n, n, 1, 4, 4, 4, 0, 1.0, n) == -1
    assert lib.hcf_op_quant_logp_backward(n, n, n, 1, 4, 4, 1.0, n) == -1
    for kind in range(4):
        assert lib.hcf_op_output_grad_backward(kind, n, n, n, 1, 3, 4, 4, n) == -1
    assert lib.hcf_op_conv_epilogue_backward(n, n, n, 0, 0, 1.0, n, 0, 1.0, n, n, n, n, 1.0, n, n, n, 1, 8, 4, 4, 8, 0, n) == -1
    assert lib.hcf_op_lu_chain(n, n, n, n, n, n, n, 3, n) == -1


def test_view_entries_refuse_malformed_descriptors_before_the_device():
    """hcf_op_*_views (include/hcflow.h: hcf_view): every malformed descriptor is HCF_ERR_ARG, nothing is dereferenced."""
    import ctypes as C
    lib = _lib.load()
    n = None
    info = (C.c_int32 * 16)()
    w = torch.zeros(32 * 64 * 9)
    buf = (C.c_float * 4)()                                            # never dereferenced: every call below is refused first
    p = C.cast(buf, C.c_void_p).value

    def V(cs, c0, nn, up=0, ptr=p):
        return (_lib.hcf_view * 1)(_lib.hcf_view(ptr, cs, c0, nn, up))
    good_s, good_o = V(64, 0, 64), V(32, 0, 32)
    wp = C.c_void_p(w.data_ptr())

    def conv(src=good_s, n_src=1, B=1, H=4, W=4, wt=wp, k=3, act=0, r1=None, r2=None, out=good_o, inf=info):
        return lib.hcf_op_conv2d_views(src, n_src, B, H, W, wt, n, n, k, act, r1, 0.2, r2, 0.2, out, 0, inf, n)
    assert conv(src=n) == -1 and conv(out=n) == -1 and conv(wt=n) == -1 and conv(inf=n) == -1
    assert conv(n_src=0) == -1 and conv(n_src=4) == -1 and conv(k=2) == -1 and conv(act=3) == -1 and conv(B=0) == -1
    assert conv(src=V(64, 0, 64, ptr=None)) == -1                      # null base
    assert conv(src=V(64, 1, 64)) == -1                                # c0 + n > cs
    assert conv(src=V(64, -1, 4)) == -1 and conv(src=V(64, 0, 0)) == -1
    assert conv(src=V(64, 0, 64, up=1), H=5) == -1                     # the upsample does not divide H
    assert conv(src=V(64, 0, 64, up=9)) == -1
    assert conv(out=V(32, 0, 32, up=1)) == -1                          # only sources are upsampled
    assert conv(out=V(128, 0, 97)) == -1                               # > 96 output channels
    assert conv(r1=V(32, 0, 31)) == -1 and conv(r2=V(64, 8, 32, ptr=None)) == -1
    dw = C.c_void_p(w.data_ptr())

    def wgrad(src=good_s, n_src=1, g=good_o, taps=9, out=dw, inf=info, W=4):
        return lib.hcf_op_conv2d_wgrad_views(src, n_src, 1, 4, W, g, taps, out, inf, n)
    assert wgrad(src=n) == -1 and wgrad(g=n) == -1 and wgrad(out=n) == -1 and wgrad(inf=n) == -1 and wgrad(taps=4) == -1
    assert wgrad(g=V(32, 4, 32)) == -1 and wgrad(src=V(64, 0, 64, up=1), W=3) == -1 and wgrad(n_src=0) == -1

    def epi(gy=good_o, y=None, act=0, g1=None, g2=None, gpre=good_o, sum_zy=None, absmax2=None, inf=info):
        return lib.hcf_op_conv_epilogue_backward_views(gy, y, n, act, 1, 0.2, g1, 1, 0.3, g2, gpre, n, sum_zy, 1.0, n, absmax2, n, 1, 4, 4, inf, n)
    assert epi(gy=n) == -1 and epi(gpre=n) == -1 and epi(inf=n) == -1
    assert epi(gpre=V(32, 0, 28)) == -1 and epi(y=V(32, 0, 28)) == -1 and epi(g1=V(32, 4, 32)) == -1 and epi(g2=V(32, 0, 32, up=1)) == -1
    assert epi(act=1) == -1 and epi(act=5, y=good_o) == -1             # an activation needs y
    assert epi(sum_zy=dw) == -1 and epi(absmax2=dw) == -1              # sum_zy needs y, absmax2 needs absmax
    assert epi(gy=V(512, 0, 257), gpre=V(512, 0, 257)) == -1


@pytest.mark.parametrize("name", PRESETS)
def test_engine_param_table_matches_python(name):
    cfg = preset(name)
    eng = _lib.Engine(cfg)                       # hcf_create touches no device
    want = [(k, tuple(s)) for k, s, _ in param_spec(cfg)]
    assert eng.param_spec() == want


def test_published_param_counts():
    # SR x4 23 232 539, Face x8 27 017 723, Rescale 4 396 350 parameters
    assert param_count(preset("SR_DF2K_4X")) == 23232539
    assert param_count(preset("SR_CelebA_8X")) == 27017723
    assert param_count(preset("Rescaling_DF2K_4X")) == 4396350
    assert len(param_spec(preset("SR_DF2K_4X"))) == 1478


def test_set_param_rejects_bad_keys_and_shapes():
    eng = _lib.Engine(preset("SR_4X_tiny"))
    with pytest.raises(_lib.HcfError):
        eng.set_param("flow.layers.1.nope", torch.zeros(3))
    with pytest.raises(_lib.HcfError):
        eng.set_param("flow.layers.1.actnorm.bias", torch.zeros(1, 13, 1, 1))
    eng.set_param("flow.layers.1.actnorm.bias", torch.zeros(1, 12, 1, 1))


def test_module_surface_and_loud_failure_without_gpu():
    from hcflow_amd.arch import HCFlowNet_SR, HCFlowNet_Rescaling, ActNorm2d
    from hcflow_amd.params import make_params
    for name, cls in (("SR_4X_tiny", HCFlowNet_SR), ("Rescaling_4X_tiny", HCFlowNet_Rescaling)):
        cfg = preset(name)
        net = cls(opt=cfg.to_opt(), step=0)
        sd = net.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, tuple(s)) for k, s, _ in param_spec(cfg)]
        net.load_state_dict(make_params(cfg, 1), strict=True)
        an = [m for n_, m in net.named_modules() if "ActNorm" in type(m).__name__]
        assert an and all(hasattr(m, "inited") for m in an)
        for m in an:
            m.inited = True                       # HCFlow_SR_model.set_actnorm_init
        net.eval()
        if not torch.cuda.is_available():
            with torch.no_grad(), pytest.raises(_lib.HcfError):
                net(lr=torch.rand(1, 3, 4, 4), eps_std=0.0, reverse=True)
    # frozen Haar weights are not trainable (Basic.py:467-468)
    assert not net.flow.layers[0].haar_weights.requires_grad


def test_from_opt_roundtrip_and_eps_shapes():
    import yaml
    for name in PRESETS:
        cfg = preset(name)
        cfg2 = NetConfig.from_opt(cfg.to_opt())
        assert param_spec(cfg) == param_spec(cfg2)
    assert eps_shapes(preset("SR_DF2K_4X"), 16, 160, 160) == [(16, 21, 160, 160), (16, 6, 320, 320)]
    assert eps_shapes(preset("SR_CelebA_8X"), 2, 20, 20) == [(2, 45, 20, 20), (2, 12, 40, 40), (2, 6, 80, 80)]


def test_default_precision_and_policies(monkeypatch):
    """The drop-in default is the mode bench.py reports as its headline: f16x3 with the synchronous range check (an
    overflowed pass is re-run exactly); HCFLOW_PRECISION / HCFLOW_RANGE_CHECK override it for unmodified driver scripts."""
    from hcflow_amd.arch import HCFlowNet_SR
    cfg = preset("SR_4X_tiny")
    monkeypatch.delenv("HCFLOW_PRECISION", raising=False)
    monkeypatch.delenv("HCFLOW_RANGE_CHECK", raising=False)
    monkeypatch.delenv("HCFLOW_STREAMS", raising=False)
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    assert net._precision[0] == "f16x3" and net._range_check[0] == "sync"
    # batched inference calls run as two half batches on the process' two side streams by default; B < 4 never splits
    assert net._nstreams[0] == 2 and net._parts(None, 0, None, 3) is None
    assert net.set_streams(1)._parts(None, 0, None, 16) is None
    monkeypatch.setenv("HCFLOW_STREAMS", "1")
    assert HCFlowNet_SR(opt=cfg.to_opt(), step=0)._nstreams[0] == 1
    # the per-call parameter stamp is two flat lists of ints (no per-parameter containers for the garbage collector)
    st = net._stamp_of(net._tensor_list())
    assert len(st) == 2 and all(isinstance(v, int) for v in st[0] + st[1]) and len(st[0]) == len(net._tensors())
    monkeypatch.setenv("HCFLOW_PRECISION", "exact")
    assert HCFlowNet_SR(opt=cfg.to_opt(), step=0)._precision[0] == "exact"
    net.set_precision("exact").set_range_check("lazy")
    assert net._precision[0] == "exact" and net._range_check[0] == "lazy"
    with pytest.raises(AssertionError):
        net.set_range_check("sometimes")


def test_parameters_resolve_through_attributes_on_dataparallel_replicas():
    """nn.DataParallel replicas (torch >= 1.5) have no registered parameters: the module must find its tensors through the
    attribute tree (hcflow_amd/arch.py: _tensors), in state_dict order, and see requires_grad on them."""
    from hcflow_amd.arch import HCFlowNet_SR
    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    keys = [k for k, _, _ in param_spec(cfg)]
    got = net._tensors()
    assert [k for k, _ in got] == keys
    sd = dict(net.named_parameters())
    assert all(t is sd[k] for k, t in got)
    replica = net._replicate_for_data_parallel()          # what torch.nn.parallel.replicate starts from
    for m in replica.modules():                           # ... and then strips, re-attaching plain tensors
        for name, p_ in list(m._parameters.items()):
            if p_ is not None:
                m._parameters[name] = None
                object.__setattr__(m, name, p_.detach().clone().requires_grad_(p_.requires_grad) * 1.0)
    assert len(list(replica.parameters())) == 0
    rt = replica._tensors()
    assert [k for k, _ in rt] == keys and all(torch.is_tensor(t) for _, t in rt)
    assert replica._wants_grad() and rt[0][1].device.type == "cpu"
