"""CPU checks of the native perceptual loss (hcflow_amd/gan.py: PerceptualLoss over the kernels of hcf_vgg.hip): its C entries are
declared, listed and exported (tests/test_cabi_cpu.py then holds the .so to the whole header), they reject bad arguments before
they touch a device, and the Python class fails loudly for what it does not support. No compute calls."""
import os
import re

import pytest
import torch

from hcflow_amd import _lib, gan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["hcf_aux_input_norm", "hcf_aux_input_norm_backward", "hcf_aux_maxpool2", "hcf_aux_maxpool2_act_backward",
           "hcf_aux_act_backward", "hcf_aux_feature_loss_workspace", "hcf_aux_feature_loss"]


def test_entries_are_declared_listed_and_exported():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared, "%s is not declared in include/hcflow.h" % name
        assert name in _lib.SYMBOLS, "%s is not listed in _lib.SYMBOLS" % name
        assert hasattr(lib, name), "libhcflow_hip.so does not export %s" % name
        assert getattr(lib, name).argtypes is not None, "%s has no argument types" % name
    assert lib.hcf_aux_feature_loss_workspace.restype is _lib.C.c_size_t


def test_entries_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    n = None
    assert lib.hcf_aux_input_norm(n, n, n, 1, 4, 4, n, n) == -1
    assert lib.hcf_aux_input_norm_backward(n, n, 1, 4, 4, n, n) == -1
    assert lib.hcf_aux_maxpool2(n, 4, 4, 1, 4, 4, n, 4, n) == -1
    assert lib.hcf_aux_maxpool2_act_backward(n, 4, n, 4, 4, 1, 4, 4, 1, n, 4, n) == -1
    assert lib.hcf_aux_act_backward(n, n, 1, 16, n, n) == -1
    assert lib.hcf_aux_feature_loss(n, n, 16, 0, n, n, n, 0, n) == -1
    # shape / flag errors come before any launch too (16-byte aligned dummy addresses, never dereferenced on the host)
    p = 4096
    assert lib.hcf_aux_maxpool2(p, 6, 4, 1, 4, 4, p, 4, n) == -1                       # cs % 4 != 0
    assert lib.hcf_aux_maxpool2(p, 4, 4, 1, 1, 4, p, 4, n) == -1                       # H < 2: no window
    assert lib.hcf_aux_maxpool2_act_backward(p, 4, p, 4, 4, 1, 4, 4, 2, p + 16, 4, n) == -1    # act is 0 or 1 here
    assert lib.hcf_aux_act_backward(p, p, 3, 16, p, n) == -1                           # act in 0..2
    assert lib.hcf_aux_act_backward(p, p, 1, 18, p, n) == -1                           # n % 4 != 0
    assert lib.hcf_aux_feature_loss(p, p, 16, 2, p, n, p, 4096, n) == -1               # kind is 0 (L1) or 1 (MSE)
    assert lib.hcf_aux_feature_loss(p, p, 0, 0, p, n, p, 4096, n) == -1                # n >= 1
    assert lib.hcf_aux_feature_loss(p, p, 1 << 20, 0, p, n, p, 8, n) == -7             # workspace too small: HCF_ERR_NOMEM
    assert lib.hcf_aux_feature_loss_workspace(0) == 0
    assert lib.hcf_aux_feature_loss_workspace(7) >= 8 and lib.hcf_aux_feature_loss_workspace(1 << 30) <= 1 << 14


def test_perceptual_loss_raises_off_gpu():
    cri = gan.PerceptualLoss(gan.VGGFeatureExtractor(feature_layer=34, use_bn=False), criterion="l1")
    with pytest.raises(_lib.HcfError, match="no CPU fallback"):
        cri(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16))


def test_perceptual_loss_rejects_batchnorm_vgg():
    with pytest.raises(ValueError, match="use_bn=True"):
        gan.PerceptualLoss(gan.VGGFeatureExtractor(feature_layer=34, use_bn=True))


def test_perceptual_loss_rejects_a_real_image_that_requires_grad():
    cri = gan.PerceptualLoss(gan.VGGFeatureExtractor(feature_layer=34, use_bn=False))
    with pytest.raises(ValueError, match="real_H requires grad"):
        cri(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16, requires_grad=True))


def test_perceptual_loss_names_what_else_it_does_not_take():
    netF = gan.VGGFeatureExtractor(feature_layer=34, use_bn=False)
    with pytest.raises(ValueError, match="criterion"):
        gan.PerceptualLoss(netF, criterion="huber")
    with pytest.raises(ValueError, match="MaxPool2d"):
        gan.PerceptualLoss(gan.VGGFeatureExtractor(feature_layer=4, use_bn=False))        # features.4 is the first max-pool
    with pytest.raises(TypeError):
        gan.PerceptualLoss(torch.nn.Identity())
    assert gan.PerceptualLoss(torch.nn.DataParallel(netF), criterion="l2").netF is netF   # unwrapped, MSE
