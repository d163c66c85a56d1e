"""The case table of tests/test_gpu_fused_dgrad.py, checked without a GPU: hcf_op_conv2d_dgrad_fused_views is exported, declared and
refuses malformed calls before it touches a device; every direct-kernel case selects the fused SCALED row, the strip width and the
rows of partial sums the table claims (hcf_debug_conv_plan with fb_y and fb_part set); the Winograd unit counts are the table's; the
gate of every case stays inside its cap from the float32-against-float64 reference alone; the planted zeros of ``y`` sit where the
reference gradient is not tiny."""
import ctypes as C
import os
import re

import pytest
import torch

from hcflow_amd import _lib, ops
from tests import fused_dgrad_cases as FC
from tests import view_conv_cases as VC

IDS = [c["name"] for c in FC.CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_declared():
    lib = _lib.load()
    name = "hcf_op_conv2d_dgrad_fused_views"
    assert name in _lib.SYMBOLS and hasattr(lib, name)
    assert len(getattr(lib, name).argtypes) == 19
    with open(os.path.join(ROOT, "include", "hcflow.h")) as f:
        decl = re.search(r"int %s\(([^;]*)\);" % name, f.read())
    assert decl and len(decl.group(1).split(",")) == 19
    assert len(ops.DGRAD_FUSED_FIELDS) == 18 and ops.DGRAD_FUSED_FIELDS[16:] == ("rows", "units")


def test_entry_refuses_malformed_calls_before_any_launch():
    """(style of tests/test_cabi_cpu.py) no pointer below is ever dereferenced: every call is refused first"""
    lib = _lib.load()
    n = None
    info = (C.c_int32 * 18)()
    w = torch.zeros(32 * 64 * 9)
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p).value

    def V(cs, c0, nn, up=0, ptr=p):
        return (_lib.hcf_view * 1)(_lib.hcf_view(ptr, cs, c0, nn, up))
    good_s, good_o, good_y = V(64, 0, 64), V(32, 0, 32), V(64, 16, 32)
    wp, dp = C.c_void_p(w.data_ptr()), C.c_void_p(p)

    def call(src=good_s, n_src=1, B=1, H=4, W=4, wt=wp, k=3, y=good_y, act=2, zy=0, out=good_o, sp=dp, sz=n, mx=dp, mx2=dp, inf=info):
        return lib.hcf_op_conv2d_dgrad_fused_views(src, n_src, B, H, W, wt, k, y, act, n, zy, 1.0, out, sp, sz, mx, mx2, inf, n)
    assert lib.hcf_op_set_precision(1) == 0
    try:
        assert call(src=n) == -1 and call(wt=n) == -1 and call(y=n) == -1 and call(out=n) == -1 and call(inf=n) == -1
        assert call(sp=n) == -1 and call(mx=n) == -1
        assert call(n_src=0) == -1 and call(n_src=4) == -1 and call(k=2) == -1 and call(act=3) == -1 and call(act=-1) == -1
        assert call(B=0) == -1 and call(H=0) == -1 and call(W=0) == -1
        assert call(src=V(64, 0, 64, ptr=None)) == -1 and call(src=V(64, 1, 64)) == -1 and call(src=V(64, 0, 0)) == -1
        assert call(src=V(64, 0, 64, up=1)) == -1                      # a gradient is never read through an upsample
        assert call(y=V(64, 16, 28)) == -1 and call(y=V(64, 40, 32)) == -1 and call(y=V(64, 16, 32, up=1)) == -1
        assert call(out=V(128, 0, 96)) == -1 and call(out=V(32, 0, 32, up=1)) == -1 and call(out=V(32, 0, 32, ptr=None)) == -1
        assert call(zy=1) == -1                                         # the sum of dz * y needs its destination
    finally:
        assert lib.hcf_op_set_precision(0) == 0
    # exact op precision: the fused form does not exist there -- refused, again before any launch
    for i in range(18):
        info[i] = 7
    assert call() == -6 and not any(info)


def plan(c, monkeypatch):
    lib = _lib.load()
    for k in FC.SWITCHES + VC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        assert k in FC.SWITCHES
        monkeypatch.setenv(k, v)
    out = (C.c_int64 * 18)()
    assert lib.hcf_debug_set_ablation(c["abl"]) == 0
    try:
        assert lib.hcf_debug_conv_plan((C.c_int32 * 40)(*FC.plan_input(c)), 40, out, 18) == 0
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
    return list(out)


@pytest.mark.parametrize("c", FC.CASES, ids=IDS)
def test_case_selects_the_launch_the_table_claims(c, monkeypatch):
    strip_w, th, rows, units = FC.TABLE[c["name"]]
    assert (c["strip_w"], c["rows"], c["units"]) == (strip_w, rows, units)
    assert units == (FC.wino_units(c["B"], c["H"], c["W"]) if c["kernel"] == "wino" else 0)
    got = plan(c, monkeypatch)          # (a Winograd case: the fused scaled row the same call would take where Winograd refuses)
    assert got[0] == 0, got
    if c["kernel"] == "wino":
        assert got[7] == 1 and c["out"][2] == 32 and not c["scale"] and not c["zy"] and rows == min(units, FC.NCU)
        assert c["k"] == 3 and all(w[2] % 16 == 0 and VC.aligned(c, w) for w in c["srcs"]) and VC.aligned(c, c["out"]) and VC.aligned(c, c["y"])
        return
    assert c["row"][5] == th
    assert ("f16x3",) + tuple(got[1:10]) + (got[13], got[14]) == FC.expected(c), (got, FC.expected(c))
    assert got[10] == got[16] == rows and got[16] <= got[17] and got[11] == 256
    assert got[15] == ((1 << 32) // strip_w + 1 if strip_w else 0)
    # without fb_part, or with a y that is not 16-byte addressable, the plan refuses: the entry then answers HCF_ERR_UNSUPPORTED
    for j, v in ((38, 0), (35, 2)):
        bad = FC.plan_input(c)
        bad[j] = v
        out = (C.c_int64 * 18)()
        assert _lib.load().hcf_debug_conv_plan((C.c_int32 * 40)(*bad), 40, out, 18) == 0 and out[0] == -6


def test_the_table_is_what_the_issue_of_each_path_needs():
    by = FC.BY_NAME
    assert {n: by[n]["strip_w"] for n in ("direct_n32_th4", "direct_strip", "direct_nostrip")} == {"direct_n32_th4": 34, "direct_strip": 21,
                                                                                                  "direct_nostrip": 0}
    assert by["direct_n32_th4"]["row"][5] == 4 and by["direct_n32_th8"]["row"][5] == 8 and by["direct_n64"]["row"][0] == 2
    assert by["direct_n64"]["abl"] == 0 and all(c["abl"] == FC.ABL_NO_WINO for c in FC.CASES if c["kernel"] == "f16x3" and c["name"] != "direct_n64")
    assert by["direct_scale_zy_k1"]["row"][7] == 1 and by["direct_scale_zy_k1"]["k"] == 1
    n24 = by["direct_n24"]
    assert n24["out"][2] == 24 and n24["out"][1] + 24 < n24["bufs"][n24["out"][0]][0]          # live channels behind the window
    m = by["wino_multi_unit"]
    units = FC.wino_units(m["B"], m["H"], m["W"])
    rounds = (units + FC.NCU - 1) // FC.NCU
    assert units == 384 > FC.NCU and rounds == 2 and units * 100 >= rounds * FC.NCU * 75       # conv_wino_rounds_ok at 256 CUs
    assert by["wino_ragged"]["units"] == 4 and by["wino_ragged_17x65"]["units"] == 12
    for c in FC.CASES:
        for w in FC.windows(c)[0] + FC.windows(c)[1]:
            assert 0 <= w[1] and w[1] + w[2] <= c["bufs"][w[0]][0] and w[3] == 0, (c["name"], w)
        assert c["env"].keys() <= set(FC.SWITCHES), c["name"]
    rows = {(FC.expected(c), c["rows"], c["units"]) for c in FC.CASES}
    assert FC.coverage(rows) == []
    assert FC.coverage({r for r in rows if r[2] <= r[1]}) == [("wino", "several units per block")]
    assert [a["env"] for a in FC.ALTERNATING] == [{}, {}]


@pytest.mark.parametrize("c", FC.CASES, ids=IDS)
def test_gate_stays_inside_its_cap(c):
    ref, e32, gate = FC.reference(c)
    print("%s: e32 %s" % (c["name"], {k: "%.3g" % v for k, v in e32.items()}))
    assert set(ref) == {"out", "sum_pre"} | ({"sum_zy"} if c["zy"] else set())
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert all(g <= FC.CAP for g in gate.values()), gate


@pytest.mark.parametrize("c", FC.CASES, ids=IDS)
def test_plants_sit_where_the_gradient_is_not_tiny(c):
    d = FC.make_inputs(c)
    if c["act"] == "none" or c["zero_src"]:
        assert d["plants"] is None
        return
    y = d["win"][c["y"]].flatten()
    idx = d["plants"]
    assert idx.numel() == 2 * FC.NPLANT == idx.unique().numel()
    bits = y[idx].view(torch.int32)
    assert bool((bits[:FC.NPLANT] == 0).all()) and bool((bits[FC.NPLANT:] == -2 ** 31).all())       # +0.0, then -0.0
    dd = FC.conv_d(c, d).abs().flatten()
    assert float(dd[idx].min()) >= 1e-3 * float(dd.max())
    # ... and the two readings of the split differ there by more than any gate: lrelu 0.8 |d|, relu |d|
    assert float(dd[idx].min()) * 0.8 / max(1.0, float(dd.max())) > 100 * FC.CAP


def test_every_relu_and_lrelu_case_has_plants_and_both_presets_bracket_the_data():
    for c in FC.CASES:
        d = FC.make_inputs(c)
        assert (d["plants"] is not None) == (c["act"] != "none" and not c["zero_src"])
        top = max([float(FC.reference(c)[0]["out"].abs().max())] + [float(d["win"][w].abs().max()) for w in c["srcs"]])
        assert FC.PRESETS["small"] == 0.0 and FC.PRESETS["big"] > 2 * top
