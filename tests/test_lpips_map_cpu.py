"""CPU checks of hcflow_amd.lpips.LPIPSMap (no GPU): the explicit bilinear upsampling of tests/lpips_map_oracle.py against
``F.interpolate``, the loud failures off-GPU and for a foreign metric, and the C ABI of the map path (declared, exported,
registered; its size functions)."""
import os

import pytest
import torch
import torch.nn.functional as F

from hcflow_amd import _lib
from hcflow_amd.lpips import LPIPS, LPIPSLoss, LPIPSMap
from tests import lpips_map_oracle as MO

SHAPES = [(2, 31, 47), (2, 33, 31), (3, 45, 70), (2, 64, 96), (2, 160, 160)]      # those of tests/test_gpu_lpips_map.py
NEW_SYMBOLS = ("hcf_lpips_embed_bytes", "hcf_lpips_alex_embed", "hcf_lpips_map_workspace", "hcf_lpips_alex_map")


def _layer_grids(H, W):
    h1, w1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    h2, w2 = (h1 - 3) // 2 + 1, (w1 - 3) // 2 + 1
    h3, w3 = (h2 - 3) // 2 + 1, (w2 - 3) // 2 + 1
    return [(h1, w1), (h2, w2), (h3, w3)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_explicit_upsampling_is_f_interpolate(B, H, W):
    g = torch.Generator().manual_seed(H * 7 + W)
    for h, w in _layer_grids(H, W):
        d = torch.rand(B, h, w, generator=g, dtype=torch.float64)
        want = F.interpolate(d[:, None], size=(H, W), mode="bilinear", align_corners=False)[:, 0]
        got = MO.upsample(d, H, W)
        assert got.shape == (B, H, W)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (h, w)


def test_layer_maps_average_to_the_scalar_oracle():
    from tests import lpips_oracle as O
    sd = LPIPS(seed=0).state_dict()
    g = torch.Generator().manual_seed(1)
    x0, x1 = torch.rand(2, 3, 45, 70, generator=g) * 2 - 1, torch.rand(2, 3, 45, 70, generator=g) * 2 - 1
    _, per = O.lpips_alex(x0, x1, sd)
    maps = MO.layer_maps(x0, x1, sd)
    assert [tuple(m.shape[1:]) for m in maps] == [(10, 16), (4, 7), (1, 3), (1, 3), (1, 3)]
    got = torch.stack([m.mean(dim=(1, 2)) for m in maps], 1)
    assert float((got - per).abs().max()) <= 1e-15


def test_off_gpu_raises():
    m = LPIPSMap(LPIPS())
    x = torch.rand(1, 3, 64, 64)
    with pytest.raises(_lib.HcfError):
        m(x, x)
    with pytest.raises(_lib.HcfError):
        m.embed(x)
    with pytest.raises(_lib.HcfError):
        m.sample_set(x)


def test_foreign_metric_is_refused():
    metric = LPIPS()
    for bad in (torch.nn.Identity(), LPIPSLoss(metric), None):
        with pytest.raises(TypeError):
            LPIPSMap(bad)


def test_symbols_declared_exported_registered():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "hcflow.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None, name
    assert lib.hcf_lpips_embed_bytes.restype is lib.hcf_lpips_workspace.restype
    assert lib.hcf_lpips_map_workspace.restype is lib.hcf_lpips_workspace.restype


def test_size_functions():
    lib = _lib.load()
    for fn in (lib.hcf_lpips_embed_bytes, lib.hcf_lpips_map_workspace):
        assert fn(2, 30, 64) == 0 and fn(2, 64, 30) == 0 and fn(0, 64, 64) == 0
        sizes = [fn(B, 45, 70) for B in (1, 2, 3, 8)]
        assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # one embedded input takes no more than the metric's stacked pair; the map call adds its layer maps and partials
    assert lib.hcf_lpips_embed_bytes(4, 64, 64) <= lib.hcf_lpips_workspace(4, 64, 64)
    assert lib.hcf_lpips_map_workspace(4, 64, 64) > lib.hcf_lpips_embed_bytes(4, 64, 64)
