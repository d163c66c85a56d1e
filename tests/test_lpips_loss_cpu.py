"""CPU part of the LPIPSLoss checks: the class imports and constructs without a GPU, the two C-ABI entries of its backward are
declared, exported and registered, and the workspace query rejects what the forward's rejects."""
import os
import re

import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd.lpips import LPIPS, LPIPSLoss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hcf_lpips_backward_workspace", "hcf_lpips_alex_backward")


def test_constructs_on_the_cpu_and_refuses_cpu_inputs():
    metric = LPIPS(seed=0)
    for red in ("mean", "sum", "none"):
        assert LPIPSLoss(metric, reduction=red).reduction == red
    assert LPIPSLoss(metric).reduction == "mean" and LPIPSLoss(metric).metric is metric
    assert not any(p.requires_grad for p in LPIPSLoss(metric).parameters())
    with pytest.raises(ValueError):
        LPIPSLoss(metric, reduction="batchmean")
    with pytest.raises(TypeError):
        LPIPSLoss(torch.nn.Identity())
    x = torch.rand(1, 3, 40, 40, requires_grad=True)
    with pytest.raises(_lib.HcfError):
        LPIPSLoss(metric)(x, x.detach())


def test_backward_entries_are_declared_exported_and_registered():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in include/hcflow.h" % name
        assert hasattr(lib, name) and name in _lib.SYMBOLS
        assert getattr(lib, name).argtypes is not None
    assert lib.hcf_lpips_backward_workspace.restype is _lib.C.c_size_t
    # the guarantee the backward rests on is part of the header: the forward's workspace is the tape
    assert "GUARANTEE" in hdr[hdr.index("LPIPS as a loss"):hdr.index("hcf_lpips_backward_workspace(")]


def test_backward_workspace_query():
    ws = _lib.load().hcf_lpips_backward_workspace
    assert ws(1, 30, 64, 1) == 0 and ws(1, 64, 30, 3) == 0 and ws(0, 64, 64, 1) == 0      # the forward's limits
    assert ws(2, 64, 64, 0) == 0 and ws(2, 64, 64, 4) == 0                                 # which: 1, 2 or 3
    sizes = [ws(B, 33, 47, 1) for B in (1, 2, 3, 8)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)       # monotone in B
    assert ws(2, 33, 47, 1) == ws(2, 33, 47, 2) < ws(2, 33, 47, 3)                         # one half is cheaper than both
    assert ws(1, 31, 31, 1) > 0


def test_backward_entry_rejects_null_tensors_without_a_device():
    lib, n = _lib.load(), None
    assert lib.hcf_lpips_alex_backward(1, 40, 40, 0, n, n, 1, n, n, n, 0, n, 0, n) == -1
