"""The case table of tests/test_gpu_fused_convs.py, checked without a GPU: every case selects the launch the table claims
(hcf_debug_conv_plan on the geometry the per-op entries build), the cases together cover every fused row of kVariants and both
fcn12 instantiations, and the gate's cap separates a dropped lo term of the f16 split from an fp32-class evaluation: a float64
evaluation with one conv operand rounded to float16 is more than 3 x the cap away from float64 in every case."""
import ctypes as C

import pytest
import torch

from hcflow_amd import _lib
from tests import fused_conv_cases as FC

SWITCHES = ("HCF_NO_TH4",)


def plan(c, monkeypatch):
    lib = _lib.load()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    vin = (C.c_int32 * 40)(*FC.plan_input(c))
    out = (C.c_int64 * 18)()
    assert lib.hcf_debug_set_ablation(c["ablation"]) == 0
    try:
        assert lib.hcf_debug_conv_plan(vin, 40, out, 18) == 0
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
    return list(out)


@pytest.mark.parametrize("c", FC.CASES, ids=FC.case_id)
def test_case_selects_the_row_the_table_claims(c, monkeypatch):
    if FC.takes_fcn12(c):
        assert c["row"] == ("fcn12", int(c["pre"]))
        return
    assert not (c["kind"] == "fcn" and c["pre"]), "the direct form refuses a pre-activation term"
    got = plan(c, monkeypatch)
    assert got[0] == 0 and tuple(got[1:10]) == c["row"], (got, c["row"])
    assert got[11] == 256


def test_cases_cover_every_fused_row():
    assert {c["row"] for c in FC.CASES} == FC.ALL_ROWS


def test_refusals_are_what_the_plan_returns(monkeypatch):
    """The direct form with a pre-activation term: HCF_ERR_ARG; a 48-channel step: HCF_ERR_UNSUPPORTED."""
    c = dict(FC.FCN_CASES[1], form=1)
    v = FC.plan_input(c)
    v[25:28] = [1, 64, 0]
    out = (C.c_int64 * 18)()
    lib = _lib.load()
    assert lib.hcf_debug_conv_plan((C.c_int32 * 40)(*v), 40, out, 18) == 0 and out[0] == -1
    t = dict(FC.TAIL_CASES[0], C=48, ns=36, f_out=24)
    assert lib.hcf_debug_conv_plan((C.c_int32 * 40)(*FC.plan_input(t)), 40, out, 18) == 0 and out[0] == -6


def test_entries_check_their_arguments_before_the_device():
    lib = _lib.load()
    n = None
    info = (C.c_int32 * 16)()
    assert lib.hcf_op_fcn12(n, n, n, 1, 1, 4, 4, n, n, n, n, n, n, n, n, 0, info, n) == -1
    assert lib.hcf_op_conv2d_step_inverse(n, 64, n, n, n, 6, n, 6, 0, 3, n, n, n, n, n, 0, 1, 4, 4, info, n) == -1


@pytest.mark.parametrize("c", FC.CASES, ids=FC.case_id)
def test_cap_separates_a_dropped_lo_term(c):
    d = FC.make_inputs(c)
    if c["kind"] == "fcn":
        ref = FC.fcn_eval(c, d)
        errs = {k: FC.err(FC.fcn_eval(c, d, drop=k), ref) for k in FC.FCN_DROPS}
        e32 = FC.err(FC.fcn_eval(c, d, dtype=torch.float32), ref)
    else:
        ref = FC.tail_eval(c, d)[0]
        errs = {k: FC.err(FC.tail_eval(c, d, drop=k)[0], ref) for k in FC.TAIL_DROPS}
        e32 = FC.err(FC.tail_eval(c, d, dtype=torch.float32)[0], ref)
    print("%s: dropped-lo errors %s, float32 evaluation %.3g" % (FC.case_id(c), {k: "%.3g" % v for k, v in errs.items()}, e32))
    assert all(v > 3 * FC.CAP for v in errs.values()), errs
    assert 4 * max(e32, FC.FLOOR) <= FC.CAP, e32          # the float32 evaluation alone leaves the gate inside its cap
