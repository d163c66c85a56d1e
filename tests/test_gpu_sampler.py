"""-m gpu: the device sampler (gauss_sample_kernel -> philox_normal, hcflow_amd/csrc/hcf_flow.hip) against the host Philox
reference of tests/philox_ref.py, draw by draw, and the engine's draw protocol (stream d for draw d, NCHW element counter,
global sample rows for shards, the taped pass) against the same reference injected as eps.

Draw gate 1e-5 * tau: rounding 2 pi u2 to float32 moves a draw by at most ulp(6.28) / 2 * 5.9 = 1.4e-6, the float32 log /
sqrt / cos of either side add a few ulp of |draw| <= 5.9 (tests/test_sampler_cpu.py bounds the host side by 3e-6 against
float64); a wrong counter word, key word, round constant or stream moves draws by O(1)."""
import functools

import numpy as np
import pytest
import torch

from oracle import hcflow_oracle as O
from tests import philox_ref as R
from tests.util import cached_params

pytestmark = pytest.mark.gpu

SHAPES = [
    (3, 6, 20, 24),       # 2 880 elements per sample: 12 blocks, the last one partly filled
    (2, 21, 9, 13),       # odd C: 2 457 elements, 10 ragged blocks, pixels split across block boundaries
    (2, 45, 5, 7),        # the widest latent (x8 net, deepest level)
    (4, 12, 1, 1),        # one pixel per sample: the sample term of the counter alone
]
SEEDS = [0, 123, 2 ** 32 + 5, 2 ** 62 - 1, 2 ** 63 + 12345]      # arch.py draws seeds below 2^62: the key's high word is live
TAUS = [0.8, 1.0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _unit(shape, seed):
    """normal(seed, 0, NCHW index) for a whole tensor, float32, read-only."""
    x = R.sample_eps(shape, 1.0, seed)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_draws_match_the_host_reference(dev, shape, seed):
    from hcflow_amd import ops
    b, C, H, W = shape
    h = torch.zeros(b, 2 * C, H, W, device=dev)                      # mean 0, logs 0: out = tau * draw
    unit = _unit(shape, seed).astype(np.float64)
    for tau in TAUS:
        out = ops.gauss_sample(h, None, tau=tau, seed=seed).cpu().numpy().astype(np.float64)
        err = float(np.abs(out - tau * unit).max())
        print("draws %s seed %d tau %.1f: max error %.3e (gate %.3e)" % (shape, seed, tau, err, 1e-5 * tau))
        assert err <= 1e-5 * tau, "worst draw error %.3e at shape %s seed %d tau %s" % (err, shape, seed, tau)


@pytest.mark.parametrize("rescale", [False, True])
def test_draws_scaled_by_the_prior(dev, rescale):
    """out = mean + exp(logs) * eps with device draws; rescale: logs = 0.318 atan(2 s) (ConditionalFlow.py:88-91)."""
    from hcflow_amd import ops
    shape, seed, tau = (2, 21, 9, 13), 2 ** 32 + 5, 0.8
    b, C, H, W = shape
    g = torch.Generator().manual_seed(17)
    mean = torch.rand(b, C, H, W, generator=g) * 2 - 1
    s = torch.rand(b, C, H, W, generator=g) * 2 - 1
    h = torch.stack((mean, s), 2).reshape(b, 2 * C, H, W)
    logs = O.logscale_of(s.double()) if rescale else s.double()
    eps = torch.from_numpy(np.float32(tau) * _unit(shape, seed)).double()
    ref = mean.double() + torch.exp(logs) * eps
    out = ops.gauss_sample(h.to(dev), None, tau=tau, seed=seed, rescale=rescale).cpu().double()
    gate = 2e-6 * max(1.0, float(ref.abs().max())) + 1e-5 * tau * float(torch.exp(logs).max())
    err = float((out - ref).abs().max())
    print("scaled draws rescale=%s: max error %.3e (gate %.3e)" % (rescale, err, gate))
    assert err <= gate, "worst error %.3e, gate %.3e" % (err, gate)


# ---------------------------------------------------------------------------------------------- engine protocol
NETS = ["SR_4X_tiny", "SR_8X_tiny", "Rescaling_4X_tiny"]
BATCH, LR_H, LR_W, TAU = 3, 9, 35, 0.8
ENGINE_SEEDS = [21, 2 ** 40 + 7]


@functools.lru_cache(maxsize=None)
def _net(name, precision):
    from hcflow_amd import HCFlowNet_SR, HCFlowNet_Rescaling
    from hcflow_amd.config import preset
    cfg = preset(name)
    net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(cached_params(name, 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    return cfg, net.to("cuda:0").eval().set_precision(precision)


@functools.lru_cache(maxsize=None)
def _lr():
    return torch.rand(BATCH, 3, LR_H, LR_W, generator=torch.Generator().manual_seed(6)).cuda()


@functools.lru_cache(maxsize=None)
def _ref_eps(name, seed, batch, first_sample):
    """level_eps on the device, computed once per (net, seed, rows) and shared by the tests below."""
    from hcflow_amd.config import preset
    return tuple(torch.from_numpy(e).cuda() for e in R.level_eps(preset(name), batch, LR_H, LR_W, TAU, seed, first_sample))


def _check(what, out, ref):
    gate = 1e-4 * max(1.0, float(ref.abs().max()))                 # the suite's inverse gate (test_inverse_matches_reference)
    err = float((out.double() - ref.double()).abs().max())
    print("%s: device draws vs injected reference draws %.3e (gate %.3e, |ref|max %.3f)" % (what, err, gate, float(ref.abs().max())))
    assert bool(torch.isfinite(ref).all()) and err <= gate, "%s: deviation %.3e, gate %.3e" % (what, err, gate)


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", NETS)
def test_engine_draws_follow_the_level_protocol(name, precision):
    """Draw d of the pass comes from stream d, element by NCHW index: the sampled output equals the pass on the host
    reference's eps. Two levels sharing a stream, a missing channel term or a dropped seed word move the output by ~ tau."""
    cfg, net = _net(name, precision)
    with torch.no_grad():
        for seed in ENGINE_SEEDS:
            out = net.reverse_flow_diracLR(_lr(), None, None, eps_std=TAU, seed=seed, clamp=False)
            ref = net.reverse_flow_diracLR(_lr(), None, None, eps_std=TAU, eps=list(_ref_eps(name, seed, BATCH, 0)), clamp=False)
            _check("%s %s seed %d" % (name, precision, seed), out, ref)


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", NETS)
def test_engine_shard_draws_the_rows_of_its_global_samples(name, precision):
    cfg, net = _net(name, precision)
    part = _lr()[1:3].contiguous()
    with torch.no_grad():
        for seed in ENGINE_SEEDS:
            out = net.reverse_flow_diracLR(part, None, None, eps_std=TAU, seed=seed, clamp=False, sample_offset=1)
            ref = net.reverse_flow_diracLR(part, None, None, eps_std=TAU, eps=list(_ref_eps(name, seed, 2, 1)), clamp=False)
            _check("%s %s seed %d rows 1..2" % (name, precision, seed), out, ref)


@pytest.mark.parametrize("precision", ["exact", "f16x3"])
@pytest.mark.parametrize("name", ["SR_4X_tiny", "SR_8X_tiny"])
def test_taped_pass_draws_the_same_streams(name, precision):
    """The taped inverse pass (train(), gradients enabled: hcf_train_inverse) fills its own GaussArgs."""
    cfg, net = _net(name, precision)
    net.train()
    try:
        with torch.enable_grad():
            for seed in ENGINE_SEEDS:
                out = net.reverse_flow_diracLR(_lr(), None, None, eps_std=TAU, seed=seed, clamp=False)
                assert out.requires_grad, "the call did not take the taped path"
                ref = net.reverse_flow_diracLR(_lr(), None, None, eps_std=TAU, eps=list(_ref_eps(name, seed, BATCH, 0)),
                                               clamp=False)
                _check("%s %s seed %d taped" % (name, precision, seed), out.detach(), ref.detach())
    finally:
        net.eval()
