"""CPU checks of the PairMetrics boundary (include/hcflow.h: hcf_metric_pair_* and the one-shot hcf_metric_psnr_ssim /
hcf_metric_imresize_down over them): the symbols, the size queries, the argument checks that run before anything touches a device,
and the Python surface. No compute calls."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from hcflow_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hcf_metric_pair_ref_bytes", "hcf_metric_pair_workspace", "hcf_metric_pair_embed", "hcf_metric_pair_compare"]
ERR_ARG, ERR_SHAPE = -1, -5


def test_symbols_declared_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name


@pytest.mark.parametrize("query", NAMES[:2])
def test_size_queries(query):
    fn = getattr(_lib.load(), query)
    for bad in [(0, 8, 8, 4), (1, 0, 8, 4), (1, 8, 0, 4), (-1, 8, 8, 0), (1, 8, 8, -1)]:
        assert fn(*bad) == 0, bad
    for H, W, s in [(48, 64, 4), (37, 53, 4), (11, 11, 2), (33, 40, 0), (640, 640, 4)]:
        sizes = [fn(B, H, W, s) for B in (1, 2, 3, 16)]
        assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:])), (H, W, s, sizes)


def test_workspace_of_an_image_does_not_depend_on_the_batch():
    fn = _lib.load().hcf_metric_pair_workspace
    for H, W, s in [(48, 64, 4), (37, 53, 3), (33, 40, 0)]:
        assert fn(5, H, W, s) == 5 * fn(1, H, W, s)


def test_entries_check_their_arguments_before_any_device_call():
    lib = _lib.load()
    B, H, W, s = 2, 24, 32, 4
    rb, wb = lib.hcf_metric_pair_ref_bytes(B, H, W, s), lib.hcf_metric_pair_workspace(B, H, W, s)
    p = C.c_void_p(4096)                       # never dereferenced: every call below is refused first
    n = None
    assert lib.hcf_metric_pair_embed(n, B, H, W, 4, s, p, rb, n) == ERR_ARG
    assert lib.hcf_metric_pair_embed(p, B, H, W, 4, s, n, rb, n) == ERR_ARG
    assert lib.hcf_metric_pair_embed(p, B, H, W, -1, s, p, rb, n) == ERR_ARG
    assert lib.hcf_metric_pair_embed(p, B, H, W, 4, -1, p, rb, n) == ERR_ARG
    assert lib.hcf_metric_pair_embed(p, 0, H, W, 4, s, p, rb, n) == ERR_ARG
    assert lib.hcf_metric_pair_embed(p, B, H, W, 4, s, p, rb - 1, n) == ERR_SHAPE
    assert lib.hcf_metric_pair_embed(p, B, H, W, 12, s, p, rb, n) == ERR_SHAPE          # H - 2 crop = 0
    for args in [(n, rb, p, B, H, W, 4, s, p, n, p, wb), (p, rb, n, B, H, W, 4, s, p, n, p, wb),
                 (p, rb, p, B, H, W, 4, s, n, n, p, wb), (p, rb, p, B, H, W, 4, s, p, n, n, wb),
                 (p, rb, p, B, H, W, -1, s, p, n, p, wb), (p, rb, p, B, H, W, 4, -2, p, n, p, wb)]:
        assert lib.hcf_metric_pair_compare(*args, n) == ERR_ARG, args
    for args in [(p, rb - 1, p, B, H, W, 4, s, p, n, p, wb), (p, rb, p, B, H, W, 4, s, p, n, p, wb - 1),
                 (p, rb, p, B, H, W, 12, s, p, n, p, wb), (p, rb, p, B, H, W, 16, s, p, n, p, wb)]:
        assert lib.hcf_metric_pair_compare(*args, n) == ERR_SHAPE, args
    # the one-shots (gt, sr, B, H, W, crop, scale, out) / (x, B, H, W, scale, out): here any device call would fail differently
    for args in [(n, p, B, H, W, 4, s, p), (p, n, B, H, W, 4, s, p), (p, p, B, H, W, 4, s, n), (p, p, 0, H, W, 4, s, p),
                 (p, p, B, H, W, -1, s, p), (p, p, B, H, W, 4, -1, p)]:
        assert lib.hcf_metric_psnr_ssim(*args, n) == ERR_ARG, args
    assert lib.hcf_metric_psnr_ssim(p, p, B, H, W, 12, s, p, n) == ERR_SHAPE            # H - 2 crop = 0
    for args in [(n, B, H, W, s, p), (p, B, H, W, s, n), (p, B, H, W, 1, p)]:
        assert lib.hcf_metric_imresize_down(*args, n) == ERR_ARG, args


def test_cpu_tensors_are_refused_and_the_loaders_have_no_path_option():
    from hcflow_amd import loader, metrics
    pm = metrics.PairMetrics()
    with pytest.raises(_lib.HcfError, match="no CPU fallback"):
        pm.embed(torch.rand(1, 3, 16, 16), crop_border=4, scale=4)
    with pytest.raises(TypeError):
        pm.compare(object(), torch.rand(1, 3, 16, 16))
    for fn in (loader.evaluate_batch, loader.evaluate_sweep):
        assert "pair_metrics" not in inspect.signature(fn).parameters         # removed, not defaulted: there is one path
