"""The case table of tests/test_gpu_view_convs.py, checked without a GPU: every run selects the launch the table claims
(hcf_debug_conv_plan on the case's own layout: windows, strides, alignment), the cases together reach every variant that only
windows reach, the arena builder round-trips and counts its outside-window floats as the geometry predicts, the gate of every
case stays inside its cap. (The view entries' refusals of malformed descriptors: tests/test_cabi_cpu.py.)"""
import ctypes as C

import pytest
import torch

from hcflow_amd import _lib
from tests import view_conv_cases as VC

RUNS = [(c, m) for c in VC.CASES for m in VC.modes(c)]
RUN_IDS = ["%s-%s" % (VC.case_id(c), m) for c, m in RUNS]


def plan(c, mode, monkeypatch):
    lib = _lib.load()
    for k in VC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in c["env"].items():
        assert k in VC.SWITCHES
        monkeypatch.setenv(k, v)
    out = (C.c_int64 * 18)()
    assert lib.hcf_debug_set_ablation(VC.ablation(mode)) == 0
    try:
        assert lib.hcf_debug_conv_plan((C.c_int32 * 40)(*VC.plan_input(c, mode)), 40, out, 18) == 0
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
    return list(out)


@pytest.mark.parametrize("c,mode", RUNS, ids=RUN_IDS)
def test_run_selects_the_row_the_table_claims(c, mode, monkeypatch):
    want = VC.expected(c, mode)
    if VC.plan_input(c, mode) is None:
        assert want[0] in ("exact", "wino", "epi")
        if c["kind"] == "conv" and c["k1_exact"] and mode != "exact":
            # the f16x3 plan must refuse this 1x1 conv: the run is the exact kernel's
            got = plan(dict(c, k1_exact=False, row=VC.f16_row(2, 0, 1, 8, k1=1)), "f16x3_nowino", monkeypatch)
            assert got[0] == -6 and not any(got[1:16]), got
        return
    got = plan(c, mode, monkeypatch)
    assert got[0] == 0, got
    if c["kind"] == "wgrad":
        assert ("wgrad",) + tuple(got[1:5]) + (got[12],) == want, (got, want)
        assert got[8] == (512 if want[1] else 256) and got[13] == ((1 << 32) // got[12] + 1 if got[12] else 0)
        return
    assert ("f16x3",) + tuple(got[1:10]) + (got[13], got[14]) == want, (got, want)
    assert got[11] == 256 and got[12] == int(any(w[3] for w in c["srcs"]))
    if c["strip_w"]:
        assert got[14] == c["W"] + 1 and got[15] == (1 << 32) // got[14] + 1


def test_winograd_cases_are_what_the_f16x3_kernel_would_take_too(monkeypatch):
    """a case the f16x3 run hands to Winograd has a direct-kernel row for the ablated run, and only 3x3 cases on 16-byte
    addressable windows of 16 k channels claim Winograd"""
    for c in VC.CONV_CASES:
        ok = (c["k"] == 3 and c["out"][2] in (32, 64) and sum(w[2] for w in c["srcs"]) >= 64 and
              all(w[2] % 16 == 0 and w[3] == 0 and VC.aligned(c, w) for w in c["srcs"]) and
              all(VC.aligned(c, w) for w in (c["out"], c["res1"], c["res2"]) if w is not None) and (c["res2"] is None or c["res1"] is not None))
        assert (c["wino"] == c["out"][2]) if ok else (c["wino"] == 0), VC.case_id(c)
        assert "f16x3_nowino" in VC.modes(c) or not c["wino"]


def test_cases_cover_every_variant_only_windows_reach():
    rows = {VC.expected(c, m) for c, m in RUNS}
    assert VC.coverage(rows) == []
    # ... and the check can fail: without the scaled cases twelve minus four K1 rows are missing
    rows = {VC.expected(c, m) for c, m in RUNS if not c.get("scaled")}
    assert len(VC.coverage(rows)) == 8


def test_geometry_of_the_named_cases():
    by = {VC.case_id(c): c for c in VC.CASES}
    g = by["conv-growth"]
    assert g["out"][0] == g["srcs"][1][0] == "grow" and g["bufs"]["grow"][0] == 128          # source and out share a buffer
    s = by["conv-shift3"]["srcs"][0]
    assert s[1] & 3 and s[1] + s[2] == by["conv-shift3"]["bufs"]["z"][0] and s[2] % 4 == 1    # the last unit reads 3 floats past the record
    st = by["conv-scaled_strip"]
    strips, tiles = (st["B"] * (st["W"] + 1) + 31) // 32, st["B"] * ((st["W"] + 31) // 32)
    assert (strips * 2, tiles * 2) == (4, 6) and strips * 10 <= tiles * 9                     # 8-row tiles: 4 against 6
    for c in VC.CASES:
        assert (c["B"], c["H"], c["W"]) in ((2, 9, 33), (2, 10, 34), (3, 9, 20)), VC.case_id(c)
        for w in VC.windows(c)[0] + VC.windows(c)[1]:
            assert 0 <= w[1] and w[1] + w[2] <= c["bufs"][w[0]][0] and w[3] == c["bufs"][w[0]][2], (VC.case_id(c), w)


@pytest.mark.parametrize("c", VC.CASES, ids=VC.case_id)
def test_arena_round_trips_and_counts(c):
    d = VC.make_inputs(c)
    off, total = VC.layout(c)
    rd, wr = VC.windows(c)
    for name, o in off.items():                                       # 16-byte aligned base, or off by exactly 4 bytes
        assert o % 4 == c["bufs"][name][1]
    for fill in ("nan", "loud"):
        a = VC.build_arena(c, d, fill)
        assert a.numel() == total and a.dtype == torch.float32
        for w, t in d["win"].items():
            assert torch.equal(VC.get(c, a, w), t)
        m = VC.outside_mask(c, list(d["win"]))
        assert int(m.sum()) == VC.outside_count(c, list(d["win"]))
        out = a[m]
        if fill == "nan":
            assert bool(torch.isnan(out).all())
        else:
            assert out.unique().numel() == out.numel() and float(out.abs().min()) >= 1e3 and float(out.abs().max()) <= 6e4
    assert int(VC.outside_mask(c, wr).sum()) == VC.outside_count(c, wr)
    # the guards: 64 floats before the pad and after the data of every buffer lie outside every window
    m = VC.outside_mask(c, rd + wr)
    for name, o in off.items():
        B, H, W, cs = VC.buf_shape(c, name)
        lo, hi = o - c["bufs"][name][1] - VC.GUARD, o + B * H * W * cs
        assert bool(m[lo:o].all()) and bool(m[hi: hi + VC.GUARD].all())
    # the dense twin holds the same windows at channel 0 of buffers of their own
    t, wm = VC.dense_twin(c)
    a = VC.build_arena(t, VC.twin_inputs(d, wm), "zero")
    for w, x in d["win"].items():
        assert wm[w][1] == 0 and torch.equal(VC.get(t, a, wm[w]), x)
    assert int((a != 0).sum()) <= sum(x.numel() for x in d["win"].values())


@pytest.mark.parametrize("c", VC.CASES, ids=VC.case_id)
def test_gate_stays_inside_its_cap(c):
    ref, e32, gate = VC.reference(c)
    print("%s: e32 %s" % (VC.case_id(c), {k: "%.3g" % v for k, v in e32.items()}))
    assert all(torch.isfinite(v).all() for v in ref.values())
    assert all(g <= VC.CAP for g in gate.values()), gate
