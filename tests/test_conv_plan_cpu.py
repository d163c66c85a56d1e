"""The conv launchers' selection, pinned without a GPU: hcf_debug_conv_plan (plan_conv_f16x3 / plan_conv_wgrad, the pure functions the
launchers dispatch from) against tests/golden/conv_plan_cases.json -- what the launchers selected before the plans existed, recorded
from host builds of the two launcher files whose launch macro and HIP calls were recorders. Status, kernel template arguments, grid,
block, dynamic LDS bytes and the argument fields the launcher patches must match exactly, with every per-launch switch set and unset."""
import ctypes as C
import json
import os

import pytest

from hcflow_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan_cases.json")
CASES = json.load(open(GOLDEN))["cases"]
SWITCHES = ("HCF_NO_TH4", "HCF_NO_DG_TH4", "HCF_NO_DG_STRIP", "HCF_NO_WG_STRIP", "HCF_WG_SINGLE_BUF", "HCF_WG_DB_BLOCK", "HCF_NO_K1")
N_IN, N_OUT = 40, 18


def plan(case, monkeypatch):
    lib = _lib.load()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        assert k in SWITCHES
        monkeypatch.setenv(k, v)
    vin = (C.c_int32 * N_IN)(*case["in"])
    out = (C.c_int64 * N_OUT)()
    assert lib.hcf_debug_set_ablation(case["ablation"]) == 0
    try:
        assert lib.hcf_debug_conv_plan(vin, N_IN, out, N_OUT) == 0
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
    return list(out)


def test_case_list_covers_every_kernel_variant_status_and_switch():
    conv = {tuple(c["expect"][1:10]) for c in CASES if c["in"][0] == 0 and c["expect"][0] == 0}
    wgrad = {tuple(c["expect"][1:5]) for c in CASES if c["in"][0] == 1 and c["expect"][0] == 0}
    assert len(conv) == 39 and len(wgrad) == 16      # every row of the launchers' tables
    assert {c["expect"][0] for c in CASES} == {0, -1, -6}
    used = set().union(*(c["env"].keys() for c in CASES))
    assert used == set(SWITCHES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_the_recorded_launch(case, monkeypatch):
    got = plan(case, monkeypatch)
    want = case["expect"]
    if case["in"][0] == 1 and want[0] != 0:
        # a refused weight-gradient call launched nothing: its status and the scratch size are all that was recorded
        got, want = [got[0], got[14]], [want[0], want[14]]
    assert got == want, "%s: in %s" % (case["name"], case["in"])
    if case["in"][0] == 0 and want[0] == 0 and want[7] and want[13]:
        # a scaled launch with the vector epilogue: its grid IS the number of partial-sum rows the engine plans for, within the bound
        assert got[16] == got[10]
    assert case["in"][0] == 1 or got[16] <= got[17]


def test_debug_entry_rejects_bad_calls():
    lib = _lib.load()
    vin, out = (C.c_int32 * N_IN)(), (C.c_int64 * N_OUT)()
    assert lib.hcf_debug_conv_plan(None, N_IN, out, N_OUT) == -1
    assert lib.hcf_debug_conv_plan(vin, N_IN - 1, out, N_OUT) == -1
    vin[0] = 2
    assert lib.hcf_debug_conv_plan(vin, N_IN, out, N_OUT) == -1
