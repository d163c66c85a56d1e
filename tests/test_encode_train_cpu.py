"""CPU checks of the trainable encode (parameter gradients of z, eps and logp): the decomposition the GPU cross-path test relies on
-- the mean over the samples of -(logp + Dirac-LR term) / (ln 2 * pixels) has the parameter gradients of the NLL -- on the oracle
alone; the C entries are declared, registered and exported and check their arguments before they touch a device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from hcflow_amd import _lib, latent
from tests import encode_train_cases as T
from tests import input_grad_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hcf_op_seed_sum", "hcf_op_axpy_job", "hcf_train_backward_encode_ex"]


@pytest.mark.parametrize("name", sorted(K.NLL_SEEDS))
def test_nll_decomposition_has_the_nll_parameter_gradients(name):
    """Reference: float64 autograd through O.sr_forward. e32 = the deviation of the same function in fp32 from it (worst tensor,
    relative norm, floor 1e-6 * gmax), measured here; the fp32 decomposition over tests.encode_oracle.encode is held to 8 * e32."""
    margin = K.rounding_margin(K.raw_lr_latent(name))
    print("%s: rounding margin of the oracle's LR latent %.3e, required %.1e" % (name, margin, K.MARGIN))
    assert margin >= K.MARGIN
    nll64, ref = T.nll_param_oracle(name, True)
    nll32, g32 = T.nll_param_oracle(name, False)
    nll_d, g_d = T.nll_decomposed_oracle(name)
    e32, k32, gmax = T.worst(g32, ref)
    e_d, k_d, _ = T.worst(g_d, ref)
    print("%s: nll %.9f (float64) %.9f (fp32) %.9f (decomposed fp32)" % (name, nll64, nll32, nll_d))
    print("%s: e32 %.3e (%s), decomposition %.3e (%s), gate 8 * e32 = %.3e, gmax %.3e" % (name, e32, k32, e_d, k_d, 8 * e32, gmax))
    assert abs(nll_d - nll64) <= 1e-5 * abs(nll64)
    assert e32 > 0 and e_d <= 8 * e32, (e_d, k_d, e32)


def test_new_symbols_declared_registered_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW:
        assert name in declared, "%s is not declared in include/hcflow.h" % name
        assert name in _lib.SYMBOLS, "%s is not registered in hcflow_amd/_lib.py" % name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int


def test_entries_check_arguments_without_a_device():
    lib = _lib.load()
    n = None
    one = (C.c_void_p * 1)()
    assert lib.hcf_train_backward_encode(n, n, n, 0, n, n, 0, n, n) == -1                     # null engine
    assert lib.hcf_train_backward_encode_ex(n, n, n, 0, one, one, 5, n, n) == -1
    assert lib.hcf_op_seed_sum(n, 4, one, n) == -1
    assert lib.hcf_op_seed_sum(one, 4, n, n) == -1
    assert lib.hcf_op_seed_sum(one, 0, one, n) == -1
    assert lib.hcf_op_axpy_job(n, n, 4, 1.0, n, n) == -1
    assert lib.hcf_op_axpy_job(n, one, 0, 1.0, n, n) == -1
    # no taped pass on the slot: a state error before anything is launched, with a gradient buffer and without the hr gradient
    from hcflow_amd.config import preset
    eng = _lib.Engine(preset("SR_4X_tiny"))                   # hcf_create touches no device
    assert lib.hcf_train_backward_encode_ex(eng.handle, n, n, 2, n, n, 0, n, n) == -1         # n_eps without the array
    assert lib.hcf_train_backward_encode_ex(eng.handle, n, n, 0, one, one, 5, n, n) == -3
    assert b"taped pass" in lib.hcf_last_error(eng.handle)


def test_nll_per_sample_signature():
    sig = inspect.signature(latent.nll_per_sample)
    assert list(sig.parameters) == ["net", "hr", "lq", "noise", "add_gt_noise"]
    assert sig.parameters["noise"].default is None and sig.parameters["add_gt_noise"].default is True
    from hcflow_amd import HCFlowNet_SR
    enc = inspect.signature(HCFlowNet_SR.encode)
    assert list(enc.parameters)[1:] == ["hr", "noise", "add_gt_noise", "param_grad"] and enc.parameters["param_grad"].default is False
