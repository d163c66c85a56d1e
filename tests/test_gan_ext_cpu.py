"""Discriminator_VGG_128 and PatchGANDiscriminator (hcflow_amd/gan.py) on the CPU side: state-dict tables and seeded default
initialisation against the reference's classes (fixtures generated from the reference, tests/golden/make_discriminator_golden.py),
the integration shim's exports, the new C entries, loud failure without a GPU."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from hcflow_amd import gan
from hcflow_amd._lib import HcfError
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [("gan_vgg128", lambda: gan.Discriminator_VGG_128(3, 64)),
         ("gan_patchgan35", lambda: gan.PatchGANDiscriminator(3, 64, 35)),
         ("gan_patchgan3", lambda: gan.PatchGANDiscriminator(3, 64, 3))]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_state_dict_table_and_seeded_init_equal_the_reference(name, make):
    g = load_golden(name)
    torch.manual_seed(int(g["seed"]))
    net = make()
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [",".join(str(v) for v in t.shape) for t in sd.values()] == [str(s) for s in g["shapes"]]
    dig = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])
    assert np.allclose(dig, g["param_digest"], rtol=1e-9, atol=1e-12)     # same modules, same order -> same default init
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["grad_keys"]]


def test_patchgan_module_indices_and_bias_layout():
    net = gan.PatchGANDiscriminator(3, 64, 4)
    m = net.model
    assert len(m) == 2 + 3 * 4 + 1
    assert isinstance(m[1], torch.nn.LeakyReLU) and m[1].negative_slope == 0.2
    assert m[0].bias is not None and all(m[2 + 3 * i].bias is None for i in range(5))
    assert all(isinstance(m[3 + 3 * i], torch.nn.BatchNorm2d) for i in range(4))
    assert m[2 + 3 * 4].out_channels == 1 and all(c.padding == (0, 0) for c in m if isinstance(c, torch.nn.Conv2d))


def test_patchgan_rejects_inputs_too_small_and_other_norm_layers():
    net = gan.PatchGANDiscriminator(3, 64, 35)
    with pytest.raises(ValueError, match="larger than 74 x 74"):
        net(torch.rand(1, 3, 74, 200))
    with pytest.raises(NotImplementedError):
        gan.PatchGANDiscriminator(3, 8, 2, norm_layer=torch.nn.InstanceNorm2d)


def test_vgg128_reset_parameters_reinitialises_every_layer():
    net = gan.Discriminator_VGG_128(3, 64)
    before = {k: v.clone() for k, v in net.named_parameters()}
    net.reset_parameters()
    assert all(not torch.equal(before[k], v) for k, v in net.named_parameters() if "conv" in k or "linear" in k)


def test_integration_shim_exports_every_discriminator():
    sys.path.insert(0, os.path.join(ROOT, "integration"))
    try:
        shim = importlib.import_module("discriminator_vgg_arch")
    finally:
        sys.path.pop(0)
    for name in ("Discriminator_VGG_128", "Discriminator_VGG_160", "PatchGANDiscriminator", "VGGFeatureExtractor"):
        assert getattr(shim, name) is getattr(gan, name)


def test_bn_entries_in_the_header_and_the_binding():
    from hcflow_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    for name in ("hcf_aux_bn_act_workspace", "hcf_aux_bn_act", "hcf_aux_bn_act_backward"):
        assert name + "(" in hdr and name in _lib.SYMBOLS
    assert "discriminator_vgg_arch.py:12-33,42-55,171-183" in hdr
    lib = _lib.load()
    assert lib.hcf_aux_bn_act_workspace(64, 16, 158, 158) > 0
    assert lib.hcf_aux_bn_act_workspace(0, 16, 158, 158) == 0
    # argument checks run before anything touches a device: a window beyond the input is refused
    rc = lib.hcf_aux_bn_act(16, 4, 3, 1, 4, 4, 2, 2, 3, 3, None, None, None, None, 0, 0.1, 1e-5, 0, 16, 4, None, None, None, 0,
                            None)
    assert rc == -1


@pytest.mark.parametrize("make", [lambda: gan.Discriminator_VGG_128(3, 64), lambda: gan.PatchGANDiscriminator(3, 64, 3)])
def test_no_cpu_fallback(make):
    """A module and input on the CPU raise, with or without a GPU in the machine: there is no eager-PyTorch path."""
    with pytest.raises(HcfError, match="no CPU fallback"):
        make()(torch.rand(2, 3, 128, 128))
