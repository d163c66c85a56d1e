"""Host-side checks of the sample-set path: the row / chunk plan of ``loader.evaluate_sweep``, the C ABI of the per-sample
temperature and of the streaming statistics, and the refusals that are decided before a device is touched."""
import os
import re

import pytest
import torch

from hcflow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hcf_inverse_taus", "hcf_metric_stats_bytes", "hcf_metric_stats_add", "hcf_metric_stats_finish"]


@pytest.mark.parametrize("B,n_heats,max_batch", [(1, 1, 16), (1, 11, 16), (2, 3, 4), (2, 3, 16), (4, 4, 16), (8, 4, 16),
                                                 (5, 7, 16), (3, 5, 1), (16, 11, 16), (0, 3, 16), (2, 0, 16)])
def test_sweep_chunks_cover_every_row_once_in_order(B, n_heats, max_batch):
    from hcflow_amd.loader import sweep_chunks
    chunks = sweep_chunks(B, n_heats, max_batch)
    R = B * n_heats
    rows = [r for r0, n in chunks for r in range(r0, r0 + n)]
    assert rows == list(range(R))
    assert all(1 <= n <= max_batch for _, n in chunks)
    assert len(chunks) == -(-R // max_batch)                      # no chunk is cut short but the last
    with pytest.raises(ValueError):
        sweep_chunks(B, n_heats, 0)


def test_new_entries_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, "include/hcflow.h does not declare %s" % name
        assert name in _lib.SYMBOLS and hasattr(lib, name), "libhcflow_hip.so does not export %s" % name


def test_stats_entries_check_their_arguments_without_a_device():
    lib = _lib.load()
    n = None
    # 16 bytes per element + one double per 1024 elements of an image (the finishing pass's partial sums)
    assert lib.hcf_metric_stats_bytes(2, 5, 7) == 2 * 105 * 16 + 2 * 8
    assert lib.hcf_metric_stats_bytes(3, 19, 37) == 3 * 2109 * 16 + 3 * 3 * 8
    assert lib.hcf_metric_stats_bytes(16, 640, 640) == 16 * 3 * 640 * 640 * 16 + 16 * 1200 * 8
    assert lib.hcf_metric_stats_bytes(0, 5, 7) == 0 and lib.hcf_metric_stats_bytes(1, 0, 7) == 0
    assert lib.hcf_metric_stats_add(n, 0, n, 2, 5, 7, 1, n) == -1
    assert lib.hcf_metric_stats_finish(n, 0, 2, 5, 7, 1, n, n, n, n) == -1
    assert lib.hcf_inverse_taus(n, n, n, 0, n, 0, 0, n, 1, 4, 4, 0, n) == -1


def _cpu_net(name="SR_4X_tiny"):
    from hcflow_amd.arch import HCFlowNet_SR, HCFlowNet_Rescaling
    from hcflow_amd.config import preset
    from hcflow_amd.params import make_params
    cfg = preset(name)
    net = (HCFlowNet_SR if cfg.sr else HCFlowNet_Rescaling)(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 1), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    return net.eval()


def test_tau_vector_parsing():
    from hcflow_amd.arch import is_tau_vector, tau_vector
    for scalar in (None, 0, 0.8, torch.tensor(0.8)):
        assert not is_tau_vector(scalar) and tau_vector(scalar, 3) is None
    for vec in ([0, 0.3, 1], (0.0, 0.3, 1.0), torch.tensor([0, 0.3, 1]), torch.tensor([0, 0.3, 1], dtype=torch.float64)):
        t = tau_vector(vec, 3)
        assert t.dtype == torch.float32 and t.tolist() == torch.tensor([0, 0.3, 1]).tolist()
    assert tau_vector([], 0).numel() == 0


@pytest.mark.parametrize("name", ["SR_4X_tiny", "Rescaling_4X_tiny"])
def test_bad_vectors_raise_before_a_device_is_touched(name, monkeypatch):
    """A wrong length, a negative or non-finite entry and the out-of-scope uses (taped inverse, dist sharding) are ValueError /
    HcfError from the host-side check: the engine is never asked for."""
    from hcflow_amd import dist
    from hcflow_amd.arch import _EngineModule
    net = _cpu_net(name)

    def no_engine(*a, **k):
        raise AssertionError("the call reached the engine")
    monkeypatch.setattr(_EngineModule, "_engine_for", no_engine)
    lr = torch.rand(3, 3, 4, 4)
    refused = (_lib.HcfError, ValueError)
    with torch.no_grad():
        for bad in ([0.5, 0.5], [0.5] * 4, [0.5, -0.1, 0.5], [0.5, float("nan"), 0.5], [0.5, float("inf"), 0.5],
                    torch.full((3, 1), 0.5), ["a", "b", "c"]):
            with pytest.raises(refused):
                net(lr=lr, eps_std=bad, reverse=True)
        with pytest.raises(refused):
            dist.sharded_inverse(net, lr, [0.5] * 3)
    with pytest.raises(refused):                                  # trainable parameters, grad mode on: the taped inverse
        net(lr=lr, eps_std=[0.5] * 3, reverse=True)


def test_loud_failure_without_a_gpu():
    """No CPU fallback: a CPU device is refused everywhere, and on a host without a GPU so are the device and a valid vector."""
    from hcflow_amd import metrics
    with pytest.raises(_lib.HcfError):
        metrics.SampleStats(2, 5, 7, "cpu")
    with pytest.raises(_lib.HcfError):
        metrics.SampleStats.like(torch.rand(2, 3, 5, 7))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HcfError):
            metrics.SampleStats(2, 5, 7, "cuda")
        net = _cpu_net()
        with torch.no_grad(), pytest.raises(_lib.HcfError):
            net(lr=torch.rand(3, 3, 4, 4), eps_std=[0.0, 0.5, 1.0], reverse=True)
