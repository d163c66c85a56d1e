"""CPU checks around the rescaling test loop (hcflow_amd/loader.py on an HCFlowNet_Rescaling, metrics.quantize / from_image): what
can be known before any GPU run -- the fixtures' own margins, the C ABI of the two new entries, and the meaning of "nll"."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd import metrics as M
from tests.util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ["net_rescale_tiny", "net_rescale_tiny_lu"]
BOUNDARY = 1e-3          # |frac(x_ref * 255) - 0.5| below this: the engine's last bits may round the pixel the other way
BOUNDARY_CAP = 0.01      # at most this share of the elements may be left out of the exact comparison


def near_rounding_boundary(x_ref: np.ndarray) -> np.ndarray:
    """Elements of the reference's pre-quantisation LR^ that sit on a rounding boundary of ``Quantization`` (shared with
    tests/test_gpu_rescale_eval.py)."""
    v = x_ref.astype(np.float64) * 255.0
    return np.abs((v - np.floor(v)) - 0.5) < BOUNDARY


@pytest.mark.parametrize("name", NETS)
def test_reference_lr_stays_within_the_rounding_boundary_cap(name):
    """The comparison of ``downscale(hr)`` with the reference's quantised LR^ leaves out the elements within 1e-3 of a rounding
    boundary; for values spread over the 8-bit steps that is ~0.2 % of them. The recorded tensors themselves must stay under
    the 1 % cap, and the recorded pair must be the reference's Quantization of one another."""
    g = load_golden(name)
    x = g["fwd_lr"]
    share = float(near_rounding_boundary(x).mean())
    print("%s: %d elements, %.4f %% within %g of a rounding boundary" % (name, x.size, 100 * share, BOUNDARY))
    assert share <= BOUNDARY_CAP
    want = np.round(np.clip(x, 0, 1) * np.float32(255.0)) / np.float32(255.0)          # np.round: half to even, as torch.round
    assert want.dtype == np.float32 and np.array_equal(want.view(np.int32), g["rt_lrq"].view(np.int32))
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_header_library_and_python_agree_on_the_image_entries():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    lib = _lib.load()
    want = {
        "hcf_metric_quantize": "const float* x, int32_t B, int32_t H, int32_t W, float* q, uint8_t* image_out, hcf_stream_t stream",
        "hcf_metric_from_image": "const uint8_t* image, int32_t B, int32_t H, int32_t W, float* out, hcf_stream_t stream",
    }
    ctype = {"const float*": C.c_void_p, "float*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p,
             "int32_t": C.c_int32, "hcf_stream_t": C.c_void_p}
    for name, args in want.items():
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m, "include/hcflow.h does not declare %s" % name
        assert " ".join(m.group(1).split()) == args
        assert name in _lib.SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [ctype[a.rsplit(" ", 1)[0]] for a in args.split(", ")], name
    # each declaration cites the reference lines it replaces
    doc = hdr[hdr.index("hcf_metric_quantize    x"):hdr.index("int hcf_metric_quantize(")]
    for cite in ("Basic.py:186-202", "HCFlow_Rescaling_model.py:306-324", "utils/util.py:790-816", "data/util.py:72-79"):
        assert cite in doc, cite


def test_image_entries_refuse_bad_arguments_before_the_device():
    """Both entries check their arguments before any HIP call: no device is needed to be refused."""
    lib = _lib.load()
    buf = (C.c_float * 16)()                                           # never dereferenced: every call below is refused first
    p = C.cast(buf, C.c_void_p).value
    n = None
    assert lib.hcf_metric_quantize(n, 1, 2, 2, p, n, n) == -1          # no input
    assert lib.hcf_metric_quantize(p, 1, 2, 2, n, n, n) == -1          # neither output
    for B, H, W in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2), (65536, 2, 2), (1, 1 << 20, 1 << 20)):
        assert lib.hcf_metric_quantize(p, B, H, W, p, p, n) == -1, (B, H, W)
        assert lib.hcf_metric_from_image(p, B, H, W, p, n) == -1, (B, H, W)
    assert lib.hcf_metric_from_image(n, 1, 2, 2, p, n) == -1
    assert lib.hcf_metric_from_image(p, 1, 2, 2, n, n) == -1


def test_quantize_and_from_image_fail_loudly_without_a_gpu():
    with pytest.raises(_lib.HcfError, match="GPU"):
        M.quantize(torch.rand(1, 3, 4, 4))
    with pytest.raises(_lib.HcfError, match="GPU"):
        M.from_image(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(_lib.HcfError, match="GPU"):
        M.quantize(np.zeros((1, 3, 4, 4), np.float32))


def test_rescaling_surface_and_loader_refusals():
    """downscale / upscale exist on the rescaling drop-in only; a rescaling net without a GT in the batch is a ValueError before
    anything runs."""
    from hcflow_amd.arch import HCFlowNet_SR, HCFlowNet_Rescaling
    from hcflow_amd.config import preset
    from hcflow_amd import loader
    net = HCFlowNet_Rescaling(opt=preset("Rescaling_4X_tiny").to_opt(), step=0).eval()
    assert callable(net.downscale) and callable(net.upscale) and not hasattr(HCFlowNet_SR, "downscale")
    lq = torch.rand(1, 3, 4, 4)
    for fn in (lambda: loader.evaluate_batch(net, {"LQ": lq}, [0.0], 1, 4), lambda: loader.evaluate_sweep(net, {"LQ": lq}, [0.0], 1, 4)):
        with pytest.raises(ValueError, match="GT"):
            fn()
    with pytest.raises(ValueError, match="noise"):
        loader.evaluate_batch(net, {"GT": torch.rand(1, 3, 16, 16)}, [0.0], 1, 4, noise=torch.rand(1, 3, 16, 16))
    hr = torch.rand(1, 3, 16, 16, requires_grad=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        net.downscale(hr)                                              # parameters (and hr) want a gradient, grad mode is on


@pytest.mark.parametrize("name", NETS)
def test_nll_column_is_the_mean_of_the_first_split_latent(name):
    """The rescaling "nll" column is HCFLowRescalingModel.test()'s return value fake_z1.mean() (HCFlow_Rescaling_model.py:324) of a
    batch-of-one call. Restated on the recorded reference z1 of the batched call: image b's mean over (c, y, x) is the recorded
    batch-of-one value within 1 ulp of float32 (the reference's own batch-of-one z1 differs from its batched z1 in the last
    bits, which the mean of 2880 values keeps under one unit)."""
    g, e = load_golden(name), load_golden("rescale_eval_tiny")
    z1 = torch.from_numpy(g["fwd_z1"])
    rec = e[name + "_z1_mean_b1"]
    assert rec.dtype == np.float32 and rec.shape == (z1.shape[0],)
    for b in range(z1.shape[0]):
        got = np.float32(z1[b:b + 1].mean().item())
        ulp = np.spacing(np.abs(rec[b]))
        print("%s image %d: mean(z1) %.9g recorded %.9g (%.2f ulp)" % (name, b, got, rec[b], abs(float(got) - float(rec[b])) / float(ulp)))
        assert abs(float(got) - float(rec[b])) <= float(ulp)
        # the recorded value is the float32 mean of the recorded batch-of-one tensor
        own = np.float32(torch.from_numpy(e[name + "_z1_b1"][b:b + 1]).mean().item())
        assert abs(float(own) - float(rec[b])) <= float(ulp)
