"""The references of tests/test_gpu_train_glue.py, checked without a GPU (tests/train_glue_ref.py): for every case of the GPU file
the closed form documented in hcf_common.h equals float64 autograd of the forward formula to 1e-12 relative, and the same closed
form evaluated in float32 stays within HALF of the gate the GPU test applies to the kernel. A case that misses the second check
has ill-conditioned inputs: change the inputs, never the gate."""
import pytest
import torch

from tests import train_glue_ref as R


def _check_both(kin, ref, closed, what):
    c64 = closed(kin, torch.float64)
    for name, entry in ref.items():
        got, want = c64[name].double(), entry[1]
        scale = entry[2] if entry[0] == "s" else max(1.0, float(want.abs().max()))
        err = (got.reshape(want.shape) - want).abs()
        assert bool((err <= 1e-12 * scale).all()), (what, name, float(err.max()))
    R.check(closed(kin, torch.float32), ref, what + " float32", frac=0.5)


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_step_forward_backward_closed_form(case):
    kin, ref = R.step_forward_case(*case)
    _check_both(kin, ref, R.step_forward_closed, "step_forward_backward %s" % (case,))


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_step_inverse_backward_closed_form(case):
    kin, ref = R.step_inverse_case(*case)
    _check_both(kin, ref, R.step_inverse_closed, "step_inverse_backward %s" % (case,))


@pytest.mark.parametrize("kind,rescale,with_gz", R.PRIOR_CASES)
@pytest.mark.parametrize("shape", R.GAUSS_CASES)
def test_prior_backward_closed_form(shape, kind, rescale, with_gz):
    kin, ref = R.prior_case(shape, kind, rescale, with_gz)
    _check_both(kin, ref, R.prior_closed, "prior_backward %s %s rescale=%d gz=%s" % (kind, shape, rescale, with_gz))


@pytest.mark.parametrize("case", R.QUANT_CASES)
def test_quant_logp_backward_closed_form(case):
    kin, ref = R.quant_case(*case)
    _check_both(kin, ref, R.quant_closed, "quant_logp_backward %s" % (case,))


def test_output_mask_is_clamp_backward():
    """The pass mask of the output-gradient kernels is torch.clamp's backward: inclusive at 0 and 1, zero for NaN."""
    z, grad, _, keep = R.mask_case()
    zr = z.clone().requires_grad_(True)
    g, = torch.autograd.grad(torch.clamp(zr, 0, 1), [zr], grad)
    assert torch.equal(g, torch.where(keep, grad, torch.zeros_like(grad)))
    assert int(keep.sum()) not in (0, keep.numel())


@pytest.mark.parametrize("lay,act,res", R.EPI_CASES)
def test_conv_epilogue_backward_closed_form(lay, act, res):
    kin, ref = R.epi_case(lay, act, res)
    _check_both(kin, ref, R.epi_closed, "conv_epilogue_backward %s %s %s" % (lay, act, res))


def test_epilogue_cases_cover_both_multipliers():
    seen = {(R.epi_zy_mult(lay, act), act) for lay, act, res in R.EPI_CASES if res == "none" and act != "lrelu"}
    assert seen == {(1.0, "none"), (3.0, "none"), (1.0, "relu"), (3.0, "relu")}


@pytest.mark.parametrize("C", R.LU_CASES)
def test_lu_chain_closed_form(C):
    kin, ref = R.lu_case(C)
    _check_both(kin, ref, R.lu_closed, "lu_chain C=%d" % C)
