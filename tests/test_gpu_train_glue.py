"""-m gpu: the backward kernels of the training path (hcflow_amd/csrc/hcf_train.hip), one kernel at a time, against float64
torch.autograd of the forward formula (tests/train_glue_ref.py; tests/test_train_glue_ref_cpu.py checks those references without
a GPU). The whole-network gradient checks reach these kernels at 256 or 64 pixels per sample and gate on 1e-4 .. 5e-3 of a gradient
norm; here a sample spans several blocks with a ragged last one whose waves 1..3 own no pixel, every register bucket of the step
kernels and both epilogue kernels run, the per-channel sums take the engine's route (per-block partial rows, launch_sum_jobs), and
the gates sit near fp32 rounding.

Gates (tests/test_gpu_flow_glue.py): elementwise 2e-6 * max(1, |ref|max); per-channel sums 1e-5 * sum |terms| of the channel; the
mask kernels and the epilogue's running maxima bit-exact. Every test prints measured error and gate."""
import pytest
import torch

from tests import train_glue_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_step_forward_backward(dev, case):
    """step_couple_bwd_kernel + step_head_bwd_kernel<8|12|24|48> + sum_jobs_kernel."""
    from hcflow_amd import ops
    k, ref = R.step_forward_case(*case)
    gzin, gh, gb, gl = ops.step_forward_backward(k["gzout"].to(dev), k["zout"].to(dev), k["h"].to(dev), k["za"].to(dev), k["mode"],
                                                 k["ns"], k["W"], k["logs"], k["gobj"], k["gb0"].to(dev), k["gl0"].to(dev))
    R.check({"gzin": gzin, "gh": gh, "g_bias": gb, "g_logs": gl}, ref, "step_forward_backward %s" % (case,))


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_step_inverse_backward(dev, case):
    """step_inv_bwd_kernel<8|12|24|48> + sum_jobs_kernel."""
    from hcflow_amd import ops
    k, ref = R.step_inverse_case(*case)
    gz, gh, gzc, y, gb, gl = ops.step_inverse_backward(k["gx"].to(dev), k["x"].to(dev), k["zc"].to(dev), k["h"].to(dev), k["mode"],
                                                       k["ns"], k["W"], k["bias"], k["logs"], k["gb0"].to(dev), k["gl0"].to(dev))
    R.check({"gz": gz, "gh": gh, "gzc": gzc, "y": y, "g_bias": gb, "g_logs": gl}, ref, "step_inverse_backward %s" % (case,))


@pytest.mark.parametrize("kind,rescale,with_gz", R.PRIOR_CASES)
@pytest.mark.parametrize("shape", R.GAUSS_CASES)
def test_prior_backward(dev, shape, kind, rescale, with_gz):
    """gauss_logp_bwd_kernel (SR logs), gauss_sample_bwd_kernel and gauss_encode_bwd_kernel with and without the rescaling
    net's soft clamp; encode also without a gradient of z."""
    from hcflow_amd import ops
    k, ref = R.prior_case(shape, kind, rescale, with_gz)
    ga, gh = ops.prior_backward(kind, k["a"].to(dev), k["h"].to(dev), None if k["ga"] is None else k["ga"].to(dev),
                                None if k["gz"] is None else k["gz"].to(dev), bool(rescale), k["gobj"])
    R.check({"ga": ga, "gh": gh}, ref, "prior_backward %s %s rescale=%d gz=%s" % (kind, shape, rescale, with_gz))


@pytest.mark.parametrize("case", R.QUANT_CASES)
def test_quant_logp_backward(dev, case):
    from hcflow_amd import ops
    k, ref = R.quant_case(*case)
    gz = ops.quant_logp_backward(k["z"].to(dev), k["lr"].to(dev), k["gobj"], k["gz0"].to(dev))
    R.check({"gz": gz}, ref, "quant_logp_backward %s" % (case,))


def test_output_gradient_masks_bit_exact(dev):
    """add_nchw_grad_kernel (with and without clamp01), mask_unit_range_kernel, mask_flat_kernel: gradients pass at exactly 0 and 1
    and are zero next to them on the outside and for NaN."""
    from hcflow_amd import ops
    z, g, gz0, keep = R.mask_case()
    zero = torch.zeros_like(g)
    zd, gd, g0d = z.to(dev), g.to(dev), gz0.to(dev)
    assert torch.equal(ops.output_grad_backward("add", gd, zd, g0d).cpu(), gz0 + g)
    assert torch.equal(ops.output_grad_backward("add_clamp01", gd, zd, g0d).cpu(), gz0 + torch.where(keep, g, zero))
    assert torch.equal(ops.output_grad_backward("mask_unit_range", None, zd, g0d).cpu(), torch.where(keep, gz0, zero))
    assert torch.equal(ops.output_grad_backward("mask_flat", gd, zd, g0d).cpu(), torch.where(keep, g, zero))
    print("output-gradient masks: bit-exact on %d elements, %d pass" % (keep.numel(), int(keep.sum())))


@pytest.mark.parametrize("lay,act,res", R.EPI_CASES)
def test_conv_epilogue_backward(dev, lay, act, res):
    """conv_epilogue_bwd_vec_kernel / conv_epilogue_bwd_kernel + sum_jobs_kernel; the running maxima bit-exact against the
    returned gpre, once with a carried value above it."""
    from hcflow_amd import ops
    k, ref = R.epi_case(lay, act, res)
    need_y = act != "none" or k["want_zy"]
    carry = 1.0e4 if R.EPI_RES.index(res) == 1 else None            # far above any |gpre| here
    out = ops.conv_epilogue_backward(
        k["gy"].to(dev), k["y"].to(dev) if need_y else None, k["scale"], act,
        rs1=R.RS1 if res != "none" else None, g1=k["g10"].to(dev) if res != "none" else None,
        rs2=R.RS2 if res == "both" else None, g2=k["g20"].to(dev) if res == "both" else None,
        want_zy=k["want_zy"], zy_mult=k["m"], sum_pre=k["sp0"].to(dev), sum_zy=k["sz0"].to(dev), want_max=2, carry2=carry,
        cs=k["cs"], c0=k["c0"])
    R.check(out, ref, "conv_epilogue_backward %s %s %s" % (lay, act, res))
    mx = out["gpre"].abs().max().reshape(1)
    assert float(mx) > 0 and torch.equal(out["absmax"], mx)
    want2 = mx if carry is None else torch.full_like(mx, carry)
    assert carry is None or carry > float(mx)
    assert torch.equal(out["absmax2"], want2), (out["absmax2"], want2)


@pytest.mark.parametrize("C", R.LU_CASES)
def test_lu_chain(dev, C):
    from hcflow_amd import ops
    k, ref = R.lu_case(C)
    dl, du, ds = ops.lu_chain(k["dW"].to(dev), k["P"].to(dev), k["L"].to(dev), k["U"].to(dev), k["dl0"].to(dev), k["du0"].to(dev),
                              k["ds0"].to(dev))
    R.check({"dl": dl, "du": du, "dlog_s": ds}, ref, "lu_chain C=%d" % C)
