"""-m gpu: the fused epilogue-backward data-gradient convs, ONE launch per run on channel windows of shared buffers, against float64.

When a data-gradient conv's output is the complete dL/dy of the conv before it, training applies that producer's epilogue backward
in the data-gradient conv's own epilogue (ConvArgs::fb_y): the SCALED rows of conv_f16x3_kernel and conv_wino2_kernel<0, true>.
hcf_op_conv2d_dgrad_fused_views fills ConvArgs as launch_dgrad (hcf_engine_train.inc) does and makes that launch on the caller's
windows; the cases (tests/fused_dgrad_cases.py) cut their buffers out of one arena, [guard][pad][buffer][guard] each, pre-filled
with NaN or with loud finite values. Every run -- one launch per (case, fill, fb_max2 preset) -- must satisfy:
  1 row         ``info`` is the launch the table claims (pinned without a GPU by tests/test_fused_dgrad_cpu.py); the rows SEEN cover
                the fused f16x3 kernel with NTB 1 / 2, TH 4 / 8, K1, with and without strips, and the fused Winograd kernel with
                one unit per block and with several (``units > grid``: a device with another CU count fails loudly).
  2 values      out, sum_pre, sum_zy: err = max |got - ref64| / max(1, max |ref64|) <= gate = 4 max(e32, 1e-6).
  3 reduction   sum_pre against the float64 sum of the launch's own stored float32 out window, per channel, within
                1e-5 sum |terms|; without want_zy, sum_zy is exactly 0 (the kernel's zeros in the NaN-filled second row).
  4 maxima      bit for bit: fb_max = max |out window| over the stored float32 values; fb_max2 = max(preset, fb_max, max |source
                windows|); all-zero sources touch neither (both preset to negative sentinels there, which any atomicMax would raise).
  5 composed    out is bit-identical to conv2d_views(scaled) followed by conv_epilogue_backward_views in place wherever that conv
                reports the same kernel, and so is fb_max; the sums agree within gate 2.
  6 no stray    every float outside the out window -- the rest of its buffer, the guards, every source buffer, the y buffer -- is
    store       bit-identical to the int32 snapshot taken before the launch.
  7 no stray    the NaN-filled arena returns HCF_OK with the range flag clear and gives the loud arena's outputs bit for bit.
    read
  8 rerun       a second identical launch is bit-identical in all outputs (Winograd: under HCF_WINO_REV=0); under the default
                alternation two consecutive Winograd launches agree bit for bit in out and both maxima, in the sums within gate 3.
A HIP error ends the module: no later case starts (DEAD).

Measured on an MI355X, loud fill, fb_max2 preset 0 (the NaN fill and the large preset: the same bits in every output but fb_max2).
"kernel reported": f16x3 (the nine template arguments, vec_epi, strip_w) or wino (channels):
  case                  kernel reported                    output        err      e32   gate  rows units
  direct_n32_th4        f16x3 (1,1,0,0,0,4,1,0,0,1,34)     out      6.07e-07 2.27e-07  4e-06     9
                                                           sum_pre  4.28e-07 1.28e-07  4e-06
  direct_n32_th8        f16x3 (1,1,0,0,0,8,1,0,0,1,34)     out      7.78e-07 3.38e-07  4e-06     6
                                                           sum_pre  6.04e-07 2.84e-07  4e-06
  direct_n64            f16x3 (2,1,0,0,0,4,1,0,0,1,34)     out      7.53e-07 3.12e-07  4e-06     9
                                                           sum_pre  6.95e-07 2.47e-07  4e-06
  direct_scale_zy       f16x3 (1,1,0,0,0,4,1,0,0,1,34)     out      6.76e-07  2.5e-07  4e-06     9
                                                           sum_pre  4.71e-07 1.69e-07  4e-06
                                                           sum_zy    2.7e-07 1.81e-07  4e-06
  direct_scale_zy_relu  f16x3 (1,1,0,0,0,4,1,0,0,1,34)     out      6.44e-07 2.79e-07  4e-06     9
                                                           sum_pre   3.1e-07  1.7e-07  4e-06
                                                           sum_zy   6.06e-07 2.98e-07  4e-06
  direct_scale_zy_k1    f16x3 (1,1,0,0,0,4,1,1,0,1,34)     out      1.82e-07  2.1e-07  4e-06     9
                                                           sum_pre  2.57e-07 1.59e-07  4e-06
                                                           sum_zy   1.38e-07 9.33e-08  4e-06
  direct_n24            f16x3 (1,1,0,0,0,4,1,0,0,1,34)     out      7.75e-07 2.64e-07  4e-06     9
                                                           sum_pre  3.05e-07  1.6e-07  4e-06
  direct_strip          f16x3 (1,1,0,0,0,4,1,0,0,1,21)     out      7.34e-07 2.41e-07  4e-06     6
                                                           sum_pre  8.37e-07 3.77e-07  4e-06
  direct_nostrip        f16x3 (1,1,0,0,0,4,1,0,0,1,0)      out      5.19e-07 2.07e-07  4e-06     6
                                                           sum_pre  4.34e-07 1.99e-07  4e-06
  direct_zero_src       f16x3 (1,1,0,0,0,4,1,0,0,1,34)     out             0        0  4e-06     9
  wino_ragged           wino (32,)                         out      3.89e-07 4.05e-07  4e-06     4     4
                                                           sum_pre  2.08e-07 2.47e-07  4e-06
  wino_ragged_17x65     wino (32,)                         out      3.24e-07 3.03e-07  4e-06    12    12
                                                           sum_pre  4.26e-07 4.73e-07  4e-06
  wino_ragged_relu      wino (32,)                         out      3.27e-07 2.31e-07  4e-06     4     4
                                                           sum_pre  2.91e-07 2.55e-07  4e-06
  wino_zero_src         wino (32,)                         out             0        0  4e-06     4     4
  wino_multi_unit       wino (32,)                         out      2.31e-07 6.24e-07  4e-06   256   384
                                                           sum_pre  6.66e-07 1.81e-07  4e-06
  worst err : gate 0.21 (direct_strip sum_pre); every gate sits on its 1e-6 floor (4e-6). Check 3: the worst channel is 2.4e-8 of
  sum |terms| (direct_nostrip) against the bound 1e-5. Check 5: every case but wino_multi_unit (whose composed conv, 16 input
  channels, runs on the direct kernel) reports the composed conv's row and is bit-identical to it in out and fb_max; the sums
  differ from the composed path's in the last bits of 21 .. 45 channels, by at most 4.1e-7 of max(1, max |sum|) (other blocks).
Walk direction: under the default alternation the sums of two consecutive Winograd launches were bit-identical in all 32 channels
of both wino_ragged_17x65 (one unit per block) and wino_multi_unit (largest difference 0 at largest |sum| 596): no dependence of a
step's bias gradients on launch parity was seen. It is not guaranteed -- a block's slot adds its units in walk order, in float32 --
which is why the test holds the two launches' sums to check 3 only and prints what it saw.

A defect found: with relu, both fused kernels stored ``v * 0.f`` where the producer was off, i.e. -0.0 for every negative dL/dy
(and NaN for a non-finite one) where conv_epilogue_bwd_kernel stores +0.0. Check 5 caught it on direct_n64, direct_scale_zy_relu
and direct_scale_zy_k1 (4771 .. 9462 values of out differing from the composed path in the sign bit, gap 0); the kernels now select
+0.0, and wino_ragged_relu holds the Winograd kernel's relu branch, which no engine launch reaches, to the same.

That the checks can fail -- scratch builds on a copy, one defect each, never committed; 123 tests each:
  i   ``*slot = *slot + fbs`` -> ``*slot = fbs`` in conv_wino2_kernel: 6 failures, all of wino_multi_unit and no other case -- check 2
      on sum_pre in all four runs (err 0.915 against the gate 4e-6; out stays at 2.3e-7), check 3 (5.7e-3 of sum |terms| against
      1e-5), the composed comparison and the alternating pair. Every other Winograd case has one unit per block and passes.
  ii  ``yv >= 0.f`` -> ``yv > 0.f`` for lrelu in the f16x3 fused branch: 25 failures -- check 2 on out in all 20 runs of the five
      lrelu cases on that kernel (err 0.39 .. 0.57: a planted zero that takes 0.2 d instead of d), and check 5 on the same five
      cases. Without the plants nothing sees it: no float32 y of these cases is otherwise exactly zero under lrelu.
  iii ``m2 = max(m, in_max_bits)`` -> ``m2 = m``: 10 failures, check 4 on fb_max2 under the small preset wherever max |source
      windows| exceeds max |out| (e.g. 4.27 stored, 4.45 wanted); the large preset hides it, as it must.
  iv  ``c4 < n4`` -> ``c4 <= n4`` in the f16x3 vector epilogue: 5 failures, all of direct_n24 -- check 6 in its four runs (2376 =
      2 * 9 * 33 * 4 floats behind the out window changed) and the composed comparison (the same count in its launch).
"""
import contextlib

import pytest
import torch

from tests import fused_dgrad_cases as FC
from tests import view_conv_cases as VC

pytestmark = pytest.mark.gpu

RUNS = [(c, p) for c in FC.CASES for p in FC.PRESETS]
RUN_IDS = ["%s-%s" % (c["name"], p) for c, p in RUNS]
IDS = [c["name"] for c in FC.CASES]
RESULTS = {}         # (case name, fill, preset) -> the run
SEEN = {}            # case name -> (row reported, rows reduced, units)
ARENAS = {}          # (case name, fill) -> the host arena (never modified)
DEAD = []            # the run after which nothing more may start: a HIP error, not a verdict on numbers
SENTINELS = (-1.0, -2.0)      # fb_max / fb_max2 before a launch on all-zero sources ("small" preset)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def _settings(c, mp):
    """the case's switches, f16x3 op precision and the ablation bits of the run, all put back afterwards"""
    from hcflow_amd import _lib, ops
    lib = _lib.load()
    for k in FC.SWITCHES + VC.SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in c["env"].items():
        mp.setenv(k, v)
    ops.set_precision("f16x3")
    assert lib.hcf_debug_set_ablation(c["abl"]) == 0
    try:
        yield
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
        ops.set_precision("exact")
        for k in c["env"]:
            mp.delenv(k, raising=False)


def _arena(c, fill):
    key = (FC.base_name(c), fill)
    if key not in ARENAS:
        ARENAS[key] = VC.build_arena(c, FC.make_inputs(c), fill)
    return ARENAS[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _presets(c, preset):
    """(fb_max, fb_max2) before the launch"""
    if c["zero_src"] and preset == "small":
        return SENTINELS
    return 0.0, FC.PRESETS[preset]


def _run(c, fill, preset, dev, mp, composed=False):
    """ONE fused launch of the case on an arena filled with ``fill`` (composed: the unfused pair of launches instead). Returns the
    outputs (CPU), the row reported, the launch record and how many floats outside the out window changed."""
    from hcflow_amd import _lib, ops
    assert not DEAD, "not started: the launch of %s ended in a HIP error" % DEAD[0]
    d = FC.make_inputs(c)
    host = _arena(c, fill)
    before = host.view(torch.int32)
    arena = host.to(dev)
    off = VC.layout(c)[0]
    B, H, W, n = c["B"], c["H"], c["W"], c["out"][2]

    def V(w):
        return ops.View(arena, off[w[0]], c["bufs"][w[0]][0], w[1], w[2], w[3])
    m0, m20 = _presets(c, preset)
    sp, sz = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    mx, mx2 = torch.full((1,), m0, device=dev), torch.full((1,), m20, device=dev)
    try:
        # (composed: a direct-kernel case keeps Winograd ablated for the plain conv too, so that the same kernel answers)
        with _settings(dict(c, abl=FC.ABL_NO_WINO) if composed and c["kernel"] == "f16x3" else c, mp):
            if composed:
                info = ops.conv2d_views([V(w) for w in c["srcs"]], B, H, W, d["w"], None, None, None, V(c["out"]), scaled=True)
                ops.conv_epilogue_backward_views(V(c["out"]), B, H, W, y=V(c["y"]), scale=d["scale"], act=c["act"], sum_pre=sp,
                                                 sum_zy=sz if c["zy"] else None, zy_mult=c["zy_mult"], absmax=mx)
            else:
                info = ops.conv2d_dgrad_fused_views([V(w) for w in c["srcs"]], B, H, W, d["w"], V(c["y"]), V(c["out"]), sp, mx, mx2,
                                                    fb_act=c["act"], fb_scale=d["scale"], sum_zy=sz, want_zy=c["zy"], zy_mult=c["zy_mult"])
            torch.cuda.synchronize(dev)
            after = arena.cpu()
    except _lib.HcfError as e:
        if getattr(e, "status", None) == -2:
            DEAD.append("%s-%s-%s" % (c["name"], fill, preset))
        raise
    except Exception:
        DEAD.append("%s-%s-%s" % (c["name"], fill, preset))
        raise
    outs = {"out": VC.get(c, after, c["out"]), "sum_pre": sp.cpu(), "sum_zy": sz.cpu(), "fb_max": mx.cpu(), "fb_max2": mx2.cpu()}
    keep = VC.outside_mask(c, [c["out"]])
    changed = int((before[keep] != after.view(torch.int32)[keep]).sum())
    return dict(outs=outs, row=FC.reported(info), info=info, changed=changed)


def _result(c, fill, preset, dev, mp):
    key = (c["name"], fill, preset)
    if key not in RESULTS:
        RESULTS[key] = _run(c, fill, preset, dev, mp)
    return RESULTS[key]


def _diff(a, b, keys):
    return {k: int((_bits(a["outs"][k]) != _bits(b["outs"][k])).sum()) for k in keys}


ALL = ("out", "sum_pre", "sum_zy", "fb_max", "fb_max2")


def _errs(c, outs):
    ref, e32, gate = FC.reference(c)
    return {k: VC.err(outs[k], ref[k]) for k in ref}, e32, gate


def _sum_check(outs):
    """check 3: (worst |sum_pre - float64 sum of the stored out| / sum |terms| over the channels, that bound's 1e-5)"""
    o = outs["out"].double()
    terms = o.abs().sum((0, 2, 3))
    dev_ = (outs["sum_pre"].double() - o.sum((0, 2, 3))).abs()
    return float((dev_ / terms.clamp_min(1e-30)).max()) if float(terms.max()) > 0 else float(dev_.max()), 1e-5


@pytest.mark.parametrize("fill", ["loud", "nan"])
@pytest.mark.parametrize("c,preset", RUNS, ids=RUN_IDS)
def test_fused_run(dev, c, preset, fill, monkeypatch):
    """1 the row, 2 values against float64, 3 the reduction alone, 4 the maxima bit for bit, 6 nothing outside the out window
    changes, 7 (nan) HCF_OK with the range flag clear"""
    r = _run(c, fill, preset, dev, monkeypatch)
    RESULTS[(c["name"], fill, preset)] = r
    SEEN[c["name"]] = (r["row"], r["info"]["rows"], r["info"]["units"])
    o = r["outs"]
    errs, e32, gate = _errs(c, o)
    for k in errs:
        print("%-22s %-5s %-4s %-7s err %.3g  e32 %.3g  gate %.3g  ratio %.2f  %s rows %d units %d" % (
            c["name"], preset, fill, k, errs[k], e32[k], gate[k], errs[k] / gate[k], r["row"], r["info"]["rows"], r["info"]["units"]))
    # 1
    assert r["row"] == FC.expected(c), (r["row"], r["info"])
    assert r["info"]["status"] == 0 and r["info"]["range_flag"] == 0, r["info"]
    assert r["info"]["rows"] == r["info"]["grid"] == c["rows"] and r["info"]["units"] == c["units"], r["info"]
    if c["name"] == "wino_multi_unit":
        assert r["info"]["units"] > r["info"]["grid"], "no block walks a second unit on this device: %s" % (r["info"],)
    # 6
    assert r["changed"] == 0, "%d floats outside the out window changed" % r["changed"]
    # 2
    for k in errs:
        assert torch.isfinite(o[k]).all(), k
        assert gate[k] <= FC.CAP
        assert errs[k] <= gate[k], (k, errs[k], gate[k])
    # 3
    worst, bound = _sum_check(o)
    print("%-22s %-5s %-4s sum_pre against the stored out: %.3g of sum |terms| (bound %.0e)" % (c["name"], preset, fill, worst, bound))
    assert worst <= bound
    if not c["zy"]:
        assert int((_bits(o["sum_zy"]) != 0).sum()) == 0, o["sum_zy"]
    # 4
    m0, m20 = _presets(c, preset)
    d = FC.make_inputs(c)
    src_max = max(float(d["win"][w].abs().max()) for w in c["srcs"])
    if c["zero_src"]:
        assert int((_bits(o["out"]) << 1 != 0).sum()) == 0                     # +-0.0 everywhere
        want_m, want_m2 = torch.tensor([m0]), torch.tensor([m20])
    else:
        want_m = o["out"].abs().max().view(1)
        want_m2 = torch.maximum(torch.maximum(want_m, torch.tensor([m20])), torch.tensor([src_max]))
    assert torch.equal(_bits(o["fb_max"]), _bits(want_m)), (o["fb_max"], want_m)
    assert torch.equal(_bits(o["fb_max2"]), _bits(want_m2)), (o["fb_max2"], want_m2, preset)
    if preset == "small" and not c["zero_src"]:
        assert float(o["fb_max2"]) == max(float(want_m), src_max) > 0.0
    if preset == "big":
        assert float(o["fb_max2"]) == FC.PRESETS["big"]


@pytest.mark.parametrize("c,preset", RUNS, ids=RUN_IDS)
def test_nothing_outside_the_windows_reaches_the_result(dev, c, preset, monkeypatch):
    """7: the NaN-filled arena gives the loud arena's outputs bit for bit"""
    a, b = _result(c, "loud", preset, dev, monkeypatch), _result(c, "nan", preset, dev, monkeypatch)
    assert a["row"] == b["row"]
    assert not any(_diff(a, b, ALL).values()), _diff(a, b, ALL)


@pytest.mark.parametrize("c", FC.CASES, ids=IDS)
def test_fused_equals_the_conv_followed_by_the_epilogue_backward(dev, c, monkeypatch):
    """5: conv2d_views(scaled, no activation) then conv_epilogue_backward_views in place"""
    a = _result(c, "loud", "small", dev, monkeypatch)
    b = _run(c, "loud", "small", dev, monkeypatch, composed=True)
    same = a["row"] == b["row"]
    dif = _diff(a, b, ("out", "fb_max", "sum_pre", "sum_zy"))
    ref, _, gate = FC.reference(c)
    gap = {k: float((a["outs"][k].double() - b["outs"][k].double()).abs().max()) / max(1.0, float(ref[k].abs().max())) for k in ref}
    print("%-22s composed ran %s: %s; values differing %s; gap %s" % (c["name"], b["row"], "same row" if same else "ANOTHER row", dif,
                                                                     {k: "%.3g" % v for k, v in gap.items()}))
    assert b["changed"] == 0
    errs, _, _ = _errs(c, b["outs"])
    assert all(errs[k] <= gate[k] for k in errs), errs
    assert all(gap[k] <= gate[k] for k in gap), gap
    # the composed conv takes the Winograd kernel from 64 input channels on only: wino_multi_unit's 16 run on the direct kernel there
    assert same == (c["name"] != "wino_multi_unit"), (a["row"], b["row"])
    if same:
        assert dif["out"] == 0 and (c["zero_src"] or dif["fb_max"] == 0), dif


@pytest.mark.parametrize("c", FC.CASES, ids=IDS)
def test_a_second_run_is_bit_identical(dev, c, monkeypatch):
    """8: the per-block partial rows, their fixed-order reduction, the strips; Winograd under HCF_WINO_REV=0"""
    a = _result(c, "loud", "small", dev, monkeypatch)
    b = _run(c, "loud", "small", dev, monkeypatch)
    assert a["row"] == b["row"] and not any(_diff(a, b, ALL).values()), _diff(a, b, ALL)


@pytest.mark.parametrize("c", FC.ALTERNATING, ids=[c["name"] for c in FC.ALTERNATING])
def test_consecutive_winograd_launches_agree_in_both_walk_directions(dev, c, monkeypatch):
    """8, default alternation: two consecutive launches walk their units in opposite directions. out and both maxima agree bit for
    bit with each other and with the HCF_WINO_REV=0 run; the sums stay within check 3 (a block's slot adds its units in walk order)."""
    base = _result(FC.BY_NAME[FC.base_name(c)], "loud", "small", dev, monkeypatch)
    a = _run(c, "loud", "small", dev, monkeypatch)
    b = _run(c, "loud", "small", dev, monkeypatch)
    for r in (a, b):
        assert r["row"] == ("wino", 32) and r["changed"] == 0
        assert not any(_diff(base, r, ("out", "fb_max", "fb_max2")).values())
        worst, bound = _sum_check(r["outs"])
        assert worst <= bound
        errs, _, gate = _errs(c, r["outs"])
        assert all(errs[k] <= gate[k] for k in errs), errs
    n = _diff(a, b, ("sum_pre",))["sum_pre"]
    gap = float((a["outs"]["sum_pre"].double() - b["outs"]["sum_pre"].double()).abs().max())
    print("%-22s sum_pre between the two walk directions: %d of %d values differ, largest difference %.3g (largest |sum| %.3g)" % (
        c["name"], n, a["outs"]["sum_pre"].numel(), gap, float(a["outs"]["sum_pre"].abs().max())))
    assert not any(_diff(a, b, ("out", "fb_max", "fb_max2", "sum_zy")).values())


def test_rows_seen_cover_both_fused_kernels(dev, monkeypatch):
    """1, over the module (a run that has not happened in this session is launched here)"""
    for c in FC.CASES:
        if c["name"] not in SEEN:
            r = _result(c, "loud", "small", dev, monkeypatch)
            SEEN[c["name"]] = (r["row"], r["info"]["rows"], r["info"]["units"])
    assert FC.coverage(set(SEEN.values())) == []
