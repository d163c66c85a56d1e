"""CPU checks of the latent-gradient interface: the three C entries are declared and registered, reject null required tensors
before they touch a device, and hcflow_amd.latent.optimise has its documented signature and leaves a module as it found it."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from hcflow_amd import _lib, latent
from hcflow_amd.config import preset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hcf_train_backward_inverse_ex", "hcf_train_backward_counts", "hcf_op_prior_sample_backward"]


def test_new_symbols_declared_registered_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, "%s is not declared in include/hcflow.h" % name
        assert name in _lib.SYMBOLS, "%s is not registered in hcflow_amd/_lib.py" % name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int


def test_new_entries_reject_null_tensors_without_a_device():
    """As test_cabi_cpu.py::test_backward_op_entries_reject_null_tensors_without_a_device: arguments are checked first."""
    lib = _lib.load()
    n = None
    assert lib.hcf_op_prior_sample_backward(n, n, n, n, n, 1, 4, 4, 4, 0, n) == -1
    assert lib.hcf_train_backward_inverse_ex(n, n, n, 0, n, n, 0, n) == -1
    assert lib.hcf_train_backward_counts(n, n) == -1
    eng = _lib.Engine(preset("SR_4X_tiny"))                   # hcf_create touches no device
    assert lib.hcf_train_backward_inverse_ex(eng.handle, n, n, 0, n, n, 0, n) == -1          # null output gradient
    one = (C.c_void_p * 1)()
    assert lib.hcf_train_backward_inverse_ex(eng.handle, one, n, 0, n, n, 2, n) == -1        # n_eps without the array
    assert lib.hcf_train_backward_inverse_ex(eng.handle, one, n, -1, n, n, 0, n) == -1
    assert lib.hcf_train_backward_counts(eng.handle, n) == -1
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.hcf_train_backward_counts(eng.handle, out) == 0 and list(out) == [0, 0, 0, 0]  # no backward pass yet
    # a backward without a taped pass is refused before anything is launched, with or without a gradient buffer
    assert lib.hcf_train_backward_inverse_ex(eng.handle, one, n, 0, n, n, 0, n) == -3


def test_optimise_signature():
    sig = inspect.signature(latent.optimise)
    assert list(sig.parameters) == ["net", "z_lr", "eps", "loss_fn", "steps", "lr", "optimise_lr", "optimizer"]
    assert sig.parameters["optimise_lr"].default is False and sig.parameters["optimizer"].default is None
    assert isinstance(sig.parameters["lr"].default, float)


class _Toy(torch.nn.Module):
    """decode(z, eps) = w * (z + sum of eps): enough to drive optimise() without the engine."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(2.0))
        self.b = torch.nn.Parameter(torch.tensor(0.5), requires_grad=False)

    def decode(self, z, eps, clamp=False):
        assert not any(p.requires_grad for p in self.parameters()), "the weights are frozen while the latents move"
        return self.w * (z + sum(e for e in eps if e is not None)) + self.b


@pytest.mark.parametrize("optimise_lr", [False, True])
def test_optimise_moves_latents_only_and_restores_flags(optimise_lr):
    net = _Toy()
    z = torch.zeros(2, 3)
    eps = [torch.ones(2, 3), None, torch.full((2, 3), -0.5)]
    target = torch.full((2, 3), 3.0)
    made = []

    def sgd(tensors):
        made.append(tensors)
        return torch.optim.SGD(tensors, lr=0.05)

    z2, eps2, losses = latent.optimise(net, z, eps, lambda out: ((out - target) ** 2).mean(), 25, optimise_lr=optimise_lr,
                                       optimizer=sgd)
    assert len(made) == 1 and len(made[0]) == (3 if optimise_lr else 2)
    assert len(losses) == 25 and all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < 0.5 * losses[0]
    assert eps2[1] is None and not any(e.requires_grad for e in eps2 if e is not None) and not z2.requires_grad
    assert torch.equal(z2, z) != optimise_lr
    assert torch.equal(eps[0], torch.ones(2, 3)) and torch.equal(z, torch.zeros(2, 3))        # the caller's tensors are not written
    assert [p.requires_grad for p in net.parameters()] == [True, False]
    assert float(net.w) == 2.0 and float(net.b) == 0.5 and net.w.grad is None
    # default optimiser: Adam
    _, _, l2 = latent.optimise(net, z, eps, lambda out: ((out - target) ** 2).mean(), 3, lr=0.1)
    assert len(l2) == 3 and l2[-1] < l2[0]


def test_optimise_restores_flags_on_error():
    net = _Toy()

    def boom(out):
        raise RuntimeError("loss failed")

    with pytest.raises(RuntimeError):
        latent.optimise(net, torch.zeros(1, 2), [torch.zeros(1, 2)], boom, 2)
    assert [p.requires_grad for p in net.parameters()] == [True, False]
