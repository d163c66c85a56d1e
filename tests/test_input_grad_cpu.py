"""CPU checks of the image-gradient interface (the forward passes differentiated w.r.t. hr / lr): the new C entries are declared,
registered and exported, reject null tensors before they touch a device and refuse to run without a taped pass; the inputs of the
GPU NLL tests keep their margin from Quant's rounding steps (oracle only); hcflow_amd.latent.refine_image leaves a module and the
caller's tensors as it found them."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from hcflow_amd import _lib, latent
from hcflow_amd.config import preset
from tests import input_grad_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hcf_train_backward_ex", "hcf_train_backward_rescale_ex", "hcf_train_encode_sr", "hcf_train_backward_encode",
       "hcf_op_quant_logp_backward_lr", "hcf_op_prior_encode_logp_backward", "hcf_op_input_grad"]


def test_new_symbols_declared_registered_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, "%s is not declared in include/hcflow.h" % name
        assert name in _lib.SYMBOLS, "%s is not registered in hcflow_amd/_lib.py" % name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int


def test_new_op_entries_reject_null_tensors_without_a_device():
    """As test_cabi_cpu.py::test_backward_op_entries_reject_null_tensors_without_a_device: arguments are checked first."""
    lib = _lib.load()
    n = None
    one = (C.c_void_p * 1)()
    assert lib.hcf_op_quant_logp_backward_lr(n, n, n, n, 1, 4, 4, 1.0, n) == -1
    assert lib.hcf_op_prior_encode_logp_backward(n, n, n, n, n, n, 1, 4, 4, 4, 0, 1.0, n) == -1
    assert lib.hcf_op_input_grad(n, n, 1, 3, 4, 4, 0, n) == -1
    assert lib.hcf_op_input_grad(one, one, 1, 3, 4, 4, 2, n) == -1                            # haar is 0 or 1
    assert lib.hcf_op_input_grad(one, one, 1, 0, 4, 4, 0, n) == -1


def test_training_entries_check_arguments_and_need_a_taped_pass():
    lib = _lib.load()
    n = None
    one = (C.c_void_p * 1)()
    assert lib.hcf_train_backward_ex(n, 1.0, n, 0, n, n, n) == -1
    assert lib.hcf_train_backward_rescale_ex(n, n, n, n, n, 0, n, n) == -1
    assert lib.hcf_train_backward_encode(n, n, n, 0, n, n, 0, n, n) == -1
    assert lib.hcf_train_encode_sr(n, n, n, n, n, 0, n, 1, 8, 8, 0, n) == -1
    eng = _lib.Engine(preset("SR_4X_tiny"))                   # hcf_create touches no device
    assert lib.hcf_train_backward_ex(eng.handle, 1.0, n, -1, n, n, n) == -1
    assert lib.hcf_train_backward_encode(eng.handle, n, n, 2, n, n, 0, one, n) == -1          # n_eps without the array
    assert lib.hcf_train_encode_sr(eng.handle, one, n, n, n, 2, n, 1, 8, 8, 0, n) == -1       # null outputs
    # no taped pass on the slot: a state error before anything is launched, with or without a gradient buffer
    assert lib.hcf_train_backward_ex(eng.handle, 1.0, n, 0, one, one, n) == -3
    assert lib.hcf_train_backward_ex(eng.handle, 1.0, one, 5, one, n, n) == -3
    assert lib.hcf_train_backward_encode(eng.handle, n, n, 0, one, n, 0, one, n) == -3
    assert lib.hcf_train_backward_encode(eng.handle, n, n, 0, one, one, 5, one, n) == -3
    assert b"taped pass" in lib.hcf_last_error(eng.handle)
    res = _lib.Engine(preset("Rescaling_4X_tiny"))
    assert lib.hcf_train_backward_rescale_ex(res.handle, n, n, n, n, 0, one, n) == -3
    # a taped encode needs a finalized engine
    arr = (C.c_void_p * 2)(1, 1)
    assert lib.hcf_train_encode_sr(eng.handle, one, n, one, arr, 2, one, 1, 8, 8, 0, n) == -3


@pytest.mark.parametrize("name", sorted(K.NLL_SEEDS))
def test_nll_inputs_stay_clear_of_the_rounding_steps(name):
    """The condition tests/test_gpu_input_grad.py puts on its NLL inputs, on the oracle alone."""
    z = K.raw_lr_latent(name)
    inside = float(((z > 0) & (z < 1)).float().mean())
    m = K.rounding_margin(z)
    print("%s seed %d: margin %.3e (required %.1e), %.0f %% of the LR latent inside (0, 1)" % (name, K.NLL_SEEDS[name], m, K.MARGIN,
                                                                                              100 * inside))
    assert inside > 0.05 and m >= K.MARGIN


def test_rounding_margin_measures_the_distance_to_a_half_step():
    z = torch.tensor([-3.0, 2.0, 10.0 / 255, (7.5 + 0.25) / 255, (100.5 - 0.125) / 255], dtype=torch.float64)
    assert abs(K.rounding_margin(z) - 0.125 / 255) < 1e-12


def test_refine_image_signature():
    sig = inspect.signature(latent.refine_image)
    assert list(sig.parameters)[:7] == ["net", "hr0", "lq", "data_loss", "steps", "lr", "weight"]
    assert sig.parameters["data_loss"].default is None and isinstance(sig.parameters["lr"].default, float)
    assert sig.parameters["weight"].default == 1.0


class _Toy(torch.nn.Module):
    """nll(hr | lq) = w * mean((pool4(hr) - lq)^2) + b: enough to drive refine_image() without the engine."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.tensor(2.0))
        self.b = torch.nn.Parameter(torch.tensor(0.5), requires_grad=False)
        self.noises = []

    def forward(self, hr=None, lr=None, reverse=False, noise=None):
        assert not reverse and not any(p.requires_grad for p in self.parameters()), "the weights are frozen while the image moves"
        self.noises.append(noise)
        low = torch.nn.functional.avg_pool2d(hr, 4)
        return low.detach(), self.w * ((low - lr) ** 2).mean() + self.b


def test_refine_image_moves_the_image_only_and_restores_flags():
    net = _Toy()
    hr0 = torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(3))
    lq = torch.rand(2, 3, 2, 2, generator=torch.Generator().manual_seed(4))
    hr0_c, lq_c = hr0.clone(), lq.clone()
    hr, losses, nlls = latent.refine_image(net, hr0, lq, steps=25, lr=0.02)
    assert len(losses) == len(nlls) == 25 and losses == nlls                                  # no data term, weight 1
    assert all(b < a for a, b in zip(nlls, nlls[1:])) and nlls[-1] < nlls[0]
    assert not hr.requires_grad and not torch.equal(hr, hr0)
    assert torch.equal(hr0, hr0_c) and torch.equal(lq, lq_c) and hr0.grad is None             # the caller's tensors are not written
    assert [p.requires_grad for p in net.parameters()] == [True, False]
    assert float(net.w.detach()) == 2.0 and float(net.b) == 0.5 and net.w.grad is None
    assert all(n is net.noises[0] for n in net.noises) and tuple(net.noises[0].shape) == tuple(hr0.shape)   # one draw, held
    # a data term, a weight and an optimiser factory
    made = []

    def sgd(tensors):
        made.append(tensors)
        return torch.optim.SGD(tensors, lr=0.5)

    target = torch.full_like(hr0, 0.25)
    nz = torch.zeros_like(hr0)
    hr2, l2, n2 = latent.refine_image(net, hr0, lq, data_loss=lambda x: ((x - target) ** 2).mean(), steps=5, weight=0.5, noise=nz,
                                      optimizer=sgd)
    assert len(made) == 1 and len(made[0]) == 1 and net.noises[-1] is nz
    d0 = float(((hr0 - target) ** 2).mean())
    assert abs(l2[0] - (0.5 * n2[0] + d0)) <= 1e-6 * abs(l2[0]) and l2[-1] < l2[0]
    assert latent.refine_image(net, hr0, lq, steps=0)[1:] == ([], [])


def test_refine_image_restores_flags_on_error():
    net = _Toy()

    def boom(x):
        raise RuntimeError("data term failed")

    with pytest.raises(RuntimeError):
        latent.refine_image(net, torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 1, 1), data_loss=boom, steps=2)
    assert [p.requires_grad for p in net.parameters()] == [True, False]
