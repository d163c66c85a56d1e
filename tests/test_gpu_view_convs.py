"""-m gpu: the conv, weight-gradient and epilogue-backward kernels on channel WINDOWS of shared buffers, against float64.

Every activation of the engine is a View: channels [c0, c0 + n) of a wider NHWC buffer whose other channels are somebody else's
live data. The older per-op entries stage each tensor into a fresh, aligned, zero-filled buffer with the window at channel 0, so a
missing channel-tail mask, a store outside the out window and every variant that only an unaligned or offset window selects
(conv_mfma_kernel<.., false>, the (N, false, true) rows of kVariants, the scalar epilogues, the VEC = false weight-gradient
kernels) ran only inside whole nets, and the SCALED / K1 rows only inside whole-net gradient tests. hcf_op_conv2d_views,
hcf_op_conv2d_wgrad_views and hcf_op_conv_epilogue_backward_views make ONE launch on the caller's windows as they are; the cases
(tests/view_conv_cases.py) cut their buffers out of one arena, [guard][pad][buffer][guard] each, pre-filled with NaN or with
loud finite values, and every run -- one launch per (case, op precision, fill) -- must satisfy:
  1 row        ``info`` is the launch the table claims (pinned without a GPU by tests/test_view_convs_cpu.py); the rows SEEN over
               the module cover the list below.
  2 accuracy   err = max |got - ref64| / max(1, max |ref64|) <= gate = 4 max(e32, 1e-6), e32 = the error of the float32 CPU
               evaluation of the reference; every gate <= 1e-5.
  3 no stray   every float outside the written windows -- the rest of the out buffer, its guards, every source and residual
    store      buffer in full (all but the out window where a case aliases them) -- is bit-identical to the int32 snapshot taken
               before the launch.
  4 no stray   the NaN run returns HCF_OK with the range flag clear and gives the loud run's result bit for bit.
    read
  5 layout     the same case on dense zero-padded views at channel 0 is bit-identical where it reports the same row, and inside
               the gate where alignment selects another kernel (ROW_DIFFERS, last column below).
  6 rerun      a second identical launch is bit-identical (fixed reduction order of the weight gradient, strips, partial sums).
A HIP error ends the module: no later case starts (DEAD).

Rows covered (VC.coverage): all 12 SCALED and K1 rows of kVariants -- (N,1,0,0,0,TH,1,0,0), (N,1,0,0,0,TH,S,1,0), N 1 / 2, TH 4 /
8, S 0 / 1 --, the four UP rows of TH 8 (N,V,1,0,0,8,0,0,0), V 0 / 1; conv_wgrad_kernel and conv_wgrad_f16x3_kernel with taps 9 / 1
and VEC 0 / 1 (all 8); both epilogue-backward kernels; both Winograd kernels, plain and scaled; conv_mfma_kernel with VEC 0 / 1 and
with the vector and the scalar epilogue. "kernel reported": exact (VEC, vec_epi, NT); f16x3 (the nine template arguments,
vec_epi, strip_w); wgrad (f16x3 kernel, TAPS, VEC, DB, strip_w); epi (vector kernel); wino (channels).

Measured on an MI355X, loud fill (the NaN fill: the same bits); epi: the worst of its six outputs:
  run (case-mode)                   kernel reported                           err      e32   gate  dense twin
  conv-growth-exact                 exact (1,1,1)                        1.14e-06 3.13e-07  4e-06  bit-identical
  conv-growth-f16x3                 wino (32,)                           2.73e-07 3.13e-07  4e-06  bit-identical
  conv-growth-f16x3_nowino          f16x3 (1,1,0,0,0,4,0,0,0,1,0)        6.55e-07 3.13e-07  4e-06  bit-identical
  conv-rdb_last-exact               exact (1,1,2)                        5.24e-08  4.4e-08  4e-06  bit-identical
  conv-rdb_last-f16x3               wino (64,)                            4.4e-08  4.4e-08  4e-06  bit-identical
  conv-rdb_last-f16x3_nowino        f16x3 (2,1,0,0,0,4,0,0,0,1,0)         4.4e-08  4.4e-08  4e-06  bit-identical
  conv-z1_tail-exact                exact (1,1,2)                        7.31e-07 2.53e-07  4e-06  bit-identical
  conv-z1_tail-f16x3                f16x3 (2,1,0,0,0,4,0,0,0,1,0)        5.92e-07 2.53e-07  4e-06  bit-identical
  conv-shift3-exact                 exact (0,1,2)                        9.05e-07 2.92e-07  4e-06  bit-identical, twin ran (exact,1,1,2)
  conv-shift3-f16x3                 f16x3 (2,0,1,0,0,8,0,0,0,1,0)        5.92e-07 2.92e-07  4e-06  bit-identical, twin ran (f16x3,2,1,0,0,0,4,0,0,0,1,0)
  conv-shift3_n32-exact             exact (0,1,1)                        8.87e-07 3.07e-07  4e-06  bit-identical, twin ran (exact,1,1,1)
  conv-shift3_n32-f16x3             f16x3 (1,0,1,0,0,8,0,0,0,1,0)        4.38e-07 3.07e-07  4e-06  bit-identical, twin ran (f16x3,1,1,0,0,0,4,0,0,0,1,0)
  conv-misaligned_src-exact         exact (0,1,1)                        6.16e-07 2.81e-07  4e-06  bit-identical, twin ran (exact,1,1,1)
  conv-misaligned_src-f16x3         f16x3 (1,0,1,0,0,8,0,0,0,1,0)        5.01e-07 2.81e-07  4e-06  inside the gate, twin ran (wino,32)
  conv-misaligned_out-exact         exact (1,0,2)                        6.74e-07  2.3e-07  4e-06  bit-identical, twin ran (exact,1,1,2)
  conv-misaligned_out-f16x3         f16x3 (2,1,0,0,0,8,0,0,0,0,0)         4.1e-07  2.3e-07  4e-06  inside the gate, twin ran (wino,64)
  conv-out_c0_2-exact               exact (1,0,1)                        7.61e-07 3.01e-07  4e-06  bit-identical, twin ran (exact,1,1,1)
  conv-out_c0_2-f16x3               f16x3 (1,1,0,0,0,8,0,0,0,0,0)        6.47e-07 3.01e-07  4e-06  inside the gate, twin ran (wino,32)
  conv-out_n24-exact                exact (1,1,1)                        7.24e-07 2.74e-07  4e-06  bit-identical
  conv-out_n24-f16x3                f16x3 (1,1,0,0,0,4,0,0,0,1,0)         5.7e-07 2.74e-07  4e-06  bit-identical
  conv-head_tails-exact             exact (1,0,1)                        5.29e-07  3.6e-07  4e-06  bit-identical
  conv-head_tails-f16x3             f16x3 (1,1,0,0,0,8,0,0,0,0,0)        3.45e-07  3.6e-07  4e-06  bit-identical
  conv-up_window-exact              exact (1,1,2)                        7.72e-07 2.84e-07  4e-06  bit-identical
  conv-up_window-f16x3              f16x3 (2,1,1,0,0,8,0,0,0,1,0)           4e-07 2.84e-07  4e-06  bit-identical
  conv-up_window_n32-exact          exact (1,1,1)                        8.18e-07 2.66e-07  4e-06  bit-identical
  conv-up_window_n32-f16x3          f16x3 (1,1,1,0,0,8,0,0,0,1,0)        8.29e-07 2.66e-07  4e-06  bit-identical
  conv-k1_n64_th4-exact             exact (1,1,2)                        2.86e-07 3.18e-07  4e-06  bit-identical
  conv-k1_n64_th4-f16x3             f16x3 (2,1,0,0,0,4,0,1,0,1,0)        1.88e-07 3.18e-07  4e-06  bit-identical
  conv-k1_n64_th8-exact             exact (1,1,2)                        2.65e-07 2.65e-07  4e-06  bit-identical
  conv-k1_n64_th8-f16x3             f16x3 (2,1,0,0,0,8,0,1,0,1,0)        1.75e-07 2.65e-07  4e-06  bit-identical
  conv-k1_n32_th4-exact             exact (1,1,1)                        2.44e-07 2.44e-07  4e-06  bit-identical
  conv-k1_n32_th4-f16x3             f16x3 (1,1,0,0,0,4,0,1,0,1,0)        1.75e-07 2.44e-07  4e-06  bit-identical
  conv-k1_n32_th8-exact             exact (1,1,1)                        2.59e-07 2.54e-07  4e-06  bit-identical
  conv-k1_n32_th8-f16x3             f16x3 (1,1,0,0,0,8,0,1,0,1,0)        1.71e-07 2.54e-07  4e-06  bit-identical
  conv-k1_unaligned-exact           exact (0,1,2)                        2.43e-07  2.9e-07  4e-06  bit-identical, twin ran (exact,1,1,2)
  conv-k1_unaligned-f16x3           exact (0,1,2)                        2.43e-07  2.9e-07  4e-06  inside the gate, twin ran (f16x3,2,1,0,0,0,4,0,1,0,1,0)
  conv-scaled_n32_th4-exact         exact (1,1,1)                        2.16e-07  8.3e-08  4e-06  bit-identical
  conv-scaled_n32_th4-f16x3         wino (32,)                           7.95e-08  8.3e-08  4e-06  bit-identical
  conv-scaled_n32_th4-f16x3_nowino  f16x3 (1,1,0,0,0,4,1,0,0,1,34)       2.01e-07  8.3e-08  4e-06  bit-identical
  conv-scaled_k1_n32_th4-exact      exact (1,1,1)                        3.49e-07 3.16e-07  4e-06  bit-identical
  conv-scaled_k1_n32_th4-f16x3      f16x3 (1,1,0,0,0,4,1,1,0,1,34)          2e-07 3.16e-07  4e-06  bit-identical
  conv-scaled_n32_th8-exact         exact (1,1,1)                        1.31e-06 2.53e-07  4e-06  bit-identical
  conv-scaled_n32_th8-f16x3         wino (32,)                           2.68e-07 2.53e-07  4e-06  bit-identical
  conv-scaled_n32_th8-f16x3_nowino  f16x3 (1,1,0,0,0,8,1,0,0,1,34)       5.29e-07 2.53e-07  4e-06  bit-identical
  conv-scaled_k1_n32_th8-exact      exact (1,1,1)                        2.88e-07 2.82e-07  4e-06  bit-identical
  conv-scaled_k1_n32_th8-f16x3      f16x3 (1,1,0,0,0,8,1,1,0,1,34)       1.97e-07 2.82e-07  4e-06  bit-identical
  conv-scaled_n64_th4-exact         exact (1,1,2)                        3.29e-07 9.62e-08  4e-06  bit-identical
  conv-scaled_n64_th4-f16x3         wino (64,)                           8.74e-08 9.62e-08  4e-06  bit-identical
  conv-scaled_n64_th4-f16x3_nowino  f16x3 (2,1,0,0,0,4,1,0,0,1,34)       1.95e-07 9.62e-08  4e-06  bit-identical
  conv-scaled_k1_n64_th4-exact      exact (1,1,2)                        3.44e-07 4.29e-07  4e-06  bit-identical
  conv-scaled_k1_n64_th4-f16x3      f16x3 (2,1,0,0,0,4,1,1,0,1,34)       2.38e-07 4.29e-07  4e-06  bit-identical
  conv-scaled_n64_th8-exact         exact (1,1,2)                        1.12e-06 2.93e-07  4e-06  bit-identical
  conv-scaled_n64_th8-f16x3         wino (64,)                           2.53e-07 2.93e-07  4e-06  bit-identical
  conv-scaled_n64_th8-f16x3_nowino  f16x3 (2,1,0,0,0,8,1,0,0,1,34)       6.35e-07 2.93e-07  4e-06  bit-identical
  conv-scaled_k1_n64_th8-exact      exact (1,1,2)                        3.36e-07 2.57e-07  4e-06  bit-identical
  conv-scaled_k1_n64_th8-f16x3      f16x3 (2,1,0,0,0,8,1,1,0,1,34)       2.18e-07 2.57e-07  4e-06  bit-identical
  conv-scaled_strip-exact           exact (1,1,1)                        2.54e-07 6.35e-08  4e-06  bit-identical
  conv-scaled_strip-f16x3           wino (32,)                           7.04e-08 6.35e-08  4e-06  bit-identical
  conv-scaled_strip-f16x3_nowino    f16x3 (1,1,0,0,0,4,1,0,0,1,21)       1.47e-07 6.35e-08  4e-06  bit-identical
  wgrad-growth-exact                wgrad (0,9,1,0,0)                    4.32e-07 7.85e-07  4e-06  bit-identical
  wgrad-growth-f16x3                wgrad (1,9,1,2,34)                   1.68e-07 7.85e-07  4e-06  bit-identical
  wgrad-shift3-exact                wgrad (0,9,0,0,0)                    4.13e-07 4.37e-07  4e-06  bit-identical, twin ran (wgrad,0,9,1,0,0)
  wgrad-shift3-f16x3                wgrad (1,9,0,2,34)                   1.29e-07 4.37e-07  4e-06  bit-identical, twin ran (wgrad,1,9,1,2,34)
  wgrad-head_tails-exact            wgrad (0,9,1,0,0)                    4.42e-07  5.1e-07  4e-06  bit-identical
  wgrad-head_tails-f16x3            wgrad (1,9,1,2,34)                   1.33e-07  5.1e-07  4e-06  bit-identical
  wgrad-misaligned-exact            wgrad (0,9,0,0,0)                    4.55e-07 4.84e-07  4e-06  bit-identical, twin ran (wgrad,0,9,1,0,0)
  wgrad-misaligned-f16x3            wgrad (1,9,0,2,34)                   1.32e-07 4.84e-07  4e-06  bit-identical, twin ran (wgrad,1,9,1,2,34)
  wgrad-up_window-exact             wgrad (0,9,1,0,0)                    5.39e-07 7.97e-07  4e-06  bit-identical
  wgrad-up_window-f16x3             wgrad (1,9,1,2,35)                   1.52e-07 7.97e-07  4e-06  bit-identical
  wgrad-taps1-exact                 wgrad (0,1,1,0,0)                    3.72e-07 4.75e-07  4e-06  bit-identical
  wgrad-taps1-f16x3                 wgrad (1,1,1,2,34)                   1.19e-07 4.75e-07  4e-06  bit-identical
  wgrad-taps1_unaligned-exact       wgrad (0,1,0,0,0)                     4.2e-07 5.46e-07  4e-06  bit-identical, twin ran (wgrad,0,1,1,0,0)
  wgrad-taps1_unaligned-f16x3       wgrad (1,1,0,2,34)                   1.28e-07 5.46e-07  4e-06  bit-identical, twin ran (wgrad,1,1,1,2,34)
  wgrad-strip-exact                 wgrad (0,9,1,0,0)                    3.61e-07 7.29e-07  4e-06  bit-identical
  wgrad-strip-f16x3                 wgrad (1,9,1,2,21)                   1.29e-07 7.29e-07  4e-06  bit-identical
  epi-vec_none-exact                epi (1,) worst: sum_zy               1.28e-07 5.94e-08  4e-06  bit-identical
  epi-scalar_none-exact             epi (0,) worst: sum_zy               1.33e-07 1.69e-07  4e-06  bit-identical
  epi-vec_relu-exact                epi (1,) worst: sum_pre              8.68e-08 7.63e-08  4e-06  bit-identical
  epi-scalar_relu-exact             epi (0,) worst: sum_pre              1.11e-07 1.11e-07  4e-06  bit-identical
  epi-vec_lrelu-exact               epi (1,) worst: sum_pre               1.8e-07 1.12e-07  4e-06  bit-identical
  epi-scalar_lrelu-exact            epi (0,) worst: sum_pre              1.12e-07 5.63e-08  4e-06  bit-identical
  worst err : gate 0.33 (conv-scaled_n32_th8-exact); every gate sits on its 1e-6 floor (4e-6)
No case failed on the real kernels. Layout: every run whose dense twin reports the same row is bit-identical to it, and so is
every pair that differs only in VEC or in the epilogue form (exact and f16x3 kernels, both weight-gradient kernels). The pairs held
to the gate only are those whose twin takes ANOTHER algorithm: conv-misaligned_src / misaligned_out / out_c0_2 in f16x3 (the aligned
twin is Winograd-eligible) and conv-k1_unaligned in f16x3 (the twin takes a K1 row, the window runs exactly on the fp32 kernel: bit
for bit the exact-precision run, test_k1_unaligned_runs_exactly_on_the_fp32_kernel).

That the checks can fail -- scratch builds, one defect each, never committed:
  a HCF_SPLIT_SLOT without its channel-tail mask (stg_valid < 4): 8 failures, all under the NaN fill -- check 4: the launches of
    conv-z1_tail, shift3, shift3_n32 and head_tails in f16x3 raise the range flag (HCF_ERR_UNSUPPORTED instead of HCF_OK). The
    loud fill cannot see this defect: the pack holds zeros for the channels behind a window, finite garbage times zero is zero.
  b ``c4 < n4`` -> ``c4 <= n4`` in conv_mfma_kernel's vector epilogue: check 3, 2376 = 2 * 9 * 33 * 4 floats behind the window of
    conv-out_n24 changed under both fills; its dense twin (check 5) reads err 0.80. Only a window of whole quads that is no whole
    32-channel tile sees it (at n = 32 / 64, c4 never reaches n4): the case out_n24 exists for this.
  c conv_wgrad_kernel's G mask without ``vg``: NOT caught, and not a defect of the result -- an output channel's column of G feeds
    only that channel's rows of dW, and the reduce step never stores rows >= n: with or without the mask the stored dW is the same,
    NaN neighbours included (all 407 tests pass). The pixel half of the same mask is live: without ``ok`` (mskg) every 3x3 fp32
    weight-gradient case fails check 2 with err 0.33 .. 0.41.
  d a_lo * b_hi dropped from the first K chunk of the SCALED rows: check 2 on all nine scaled f16x3 runs, err 1.8e-5 .. 1.9e-4
    against the gate 4e-6 (err : gate 4.5 .. 47), under both fills, and check 5 on the same runs.
"""
import contextlib

import pytest
import torch

from tests import view_conv_cases as VC

pytestmark = pytest.mark.gpu

RUNS = [(c, m) for c in VC.CASES for m in VC.modes(c)]
RUN_IDS = ["%s-%s" % (VC.case_id(c), m) for c, m in RUNS]
RESULTS = {}         # (case id, mode, fill) -> the run: outputs on the CPU, the row reported
SEEN = {}            # (case id, mode) -> the row its launch reported
DEAD = []            # the run after which nothing more may start: a HIP error, not a verdict on numbers


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def _settings(c, mode, mp):
    """the case's switches, the op precision and the ablation bits of the run, all put back afterwards"""
    from hcflow_amd import _lib, ops
    lib = _lib.load()
    for k in VC.SWITCHES:
        mp.delenv(k, raising=False)
    for k, v in c["env"].items():
        mp.setenv(k, v)
    ops.set_precision(VC.precision(mode))
    assert lib.hcf_debug_set_ablation(VC.ablation(mode)) == 0
    try:
        yield
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
        ops.set_precision("exact")
        for k in c["env"]:
            mp.delenv(k, raising=False)


def _run(c, mode, fill, dev, mp, d=None):
    """ONE launch of the case on an arena filled with ``fill``. Returns the outputs (CPU), the row reported, the launch record
    and how many floats outside the written windows changed (int32 comparison with the snapshot taken before the launch)."""
    from hcflow_amd import _lib, ops
    assert not DEAD, "not started: the launch of %s ended in a HIP error" % DEAD[0]
    d = VC.make_inputs(c) if d is None else d
    host = VC.build_arena(c, d, fill)
    before = host.view(torch.int32).clone()
    arena = host.to(dev)
    off = VC.layout(c)[0]
    B, H, W = c["B"], c["H"], c["W"]

    def V(w):
        return None if w is None else ops.View(arena, off[w[0]], c["bufs"][w[0]][0], w[1], w[2], w[3])
    extra = {}
    try:
        with _settings(c, mode, mp):
            if c["kind"] == "conv":
                info = ops.conv2d_views([V(w) for w in c["srcs"]], B, H, W, d["w"], d["bias"], d["scale"], c["act"], V(c["out"]),
                                        res1=V(c["res1"]), rs1=c["rs1"], res2=V(c["res2"]), rs2=c["rs2"], scaled=c["scaled"])
            elif c["kind"] == "wgrad":
                extra["dw"], info = ops.conv2d_wgrad_views([V(w) for w in c["srcs"]], B, H, W, V(c["g"]), c["k"])
            else:
                sp, sz, mx = d["sp0"].to(dev), d["sz0"].to(dev), torch.zeros(1, device=dev)
                info = ops.conv_epilogue_backward_views(V(c["gy"]), B, H, W, y=V(c["y"]), scale=d["scale"], act=c["act"], rs1=c["rs1"],
                                                        g1=V(c["g1"]), rs2=c["rs2"], g2=V(c["g2"]), sum_pre=sp, sum_zy=sz,
                                                        zy_mult=c["zy_mult"], absmax=mx)
                extra = {"sum_pre": sp.cpu(), "sum_zy": sz.cpu(), "absmax": mx.cpu()}
            torch.cuda.synchronize(dev)
            after = arena.cpu()
    except _lib.HcfError as e:
        if getattr(e, "status", None) == -2:
            DEAD.append("%s-%s-%s" % (VC.case_id(c), mode, fill))
        raise
    except Exception:
        DEAD.append("%s-%s-%s" % (VC.case_id(c), mode, fill))
        raise
    if c["kind"] == "conv":
        outs = {"out": VC.get(c, after, c["out"])}
    elif c["kind"] == "wgrad":
        outs = dict(extra)
    else:
        outs = dict(extra, gpre=VC.get(c, after, c["gy"]), g1=VC.get(c, after, c["g1"]), g2=VC.get(c, after, c["g2"]))
    keep = VC.outside_mask(c, VC.windows(c)[1])
    changed = int((before[keep] != after.view(torch.int32)[keep]).sum())
    return dict(outs=outs, row=VC.reported(c, info), info=info, changed=changed)


def _result(c, mode, fill, dev, mp):
    key = (VC.case_id(c), mode, fill)
    if key not in RESULTS:
        RESULTS[key] = _run(c, mode, fill, dev, mp)
    return RESULTS[key]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _errs(c, outs):
    ref, e32, gate = VC.reference(c)
    return {k: VC.err(outs[k], ref[k]) for k in ref}, e32, gate


@pytest.mark.parametrize("fill", ["loud", "nan"])
@pytest.mark.parametrize("c,mode", RUNS, ids=RUN_IDS)
def test_window_run(dev, c, mode, fill, monkeypatch):
    """1 the row, 2 accuracy against float64, 3 nothing outside the written windows changes, 4 (nan) HCF_OK, range flag clear"""
    r = _run(c, mode, fill, dev, monkeypatch)
    RESULTS[(VC.case_id(c), mode, fill)] = r
    SEEN[(VC.case_id(c), mode)] = r["row"]
    errs, e32, gate = _errs(c, r["outs"])
    for k in errs:
        print("%-34s %-6s %-5s %-8s err %.3g  e32 %.3g  gate %.3g  ratio %.2f  %s" % (
            "%s-%s" % (VC.case_id(c), mode), fill, r["row"][0], k, errs[k], e32[k], gate[k], errs[k] / gate[k], r["row"][1:]))
    assert r["row"] == VC.expected(c, mode), (r["row"], r["info"])
    if c["kind"] == "conv":
        assert r["info"]["status"] == 0 and r["info"]["range_flag"] == 0, r["info"]
    assert r["changed"] == 0, "%d floats outside the written windows changed" % r["changed"]
    for k in errs:
        assert torch.isfinite(r["outs"][k]).all(), k
        assert gate[k] <= VC.CAP
        assert errs[k] <= gate[k], (k, errs[k], gate[k])


@pytest.mark.parametrize("c,mode", RUNS, ids=RUN_IDS)
def test_nothing_outside_the_source_windows_reaches_the_result(dev, c, mode, monkeypatch):
    """the NaN-filled arena gives the loud arena's result bit for bit"""
    a, b = _result(c, mode, "loud", dev, monkeypatch), _result(c, mode, "nan", dev, monkeypatch)
    assert a["row"] == b["row"]
    for k in a["outs"]:
        n = int((_bits(a["outs"][k]) != _bits(b["outs"][k])).sum())
        assert n == 0, "%s: %d values differ between the fills" % (k, n)


# (case, op precision) whose dense twin runs ANOTHER variant: alignment, or a window start that is no multiple of 4, selected it
ROW_DIFFERS = ({("conv-" + n, p) for n in ("shift3", "shift3_n32", "misaligned_src", "misaligned_out", "out_c0_2") for p in ("exact", "f16x3")} |
               {("conv-k1_unaligned", "exact"), ("conv-k1_unaligned", "f16x3")} |
               {("wgrad-" + n, p) for n in ("shift3", "misaligned", "taps1_unaligned") for p in ("exact", "f16x3")})


@pytest.mark.parametrize("c,mode", RUNS, ids=RUN_IDS)
def test_the_window_changes_no_arithmetic(dev, c, mode, monkeypatch):
    """the same case on dense zero-padded views at channel 0: bit-identical where the same kernel variant runs, inside the gate
    where alignment selects another"""
    a = _result(c, mode, "loud", dev, monkeypatch)
    t, wm = VC.dense_twin(c)
    b = _run(t, mode, "zero", dev, monkeypatch, d=VC.twin_inputs(VC.make_inputs(c), wm))
    same = a["row"] == b["row"]
    print("%-34s dense twin: %s%s" % ("%s-%s" % (VC.case_id(c), mode), "same row" if same else "row %s" % (b["row"],),
                                     ", bit-identical" if _same_bits(a["outs"], b["outs"]) else ""))
    assert b["changed"] == 0
    errs, _, gate = _errs(c, b["outs"])
    assert all(errs[k] <= gate[k] for k in errs), errs
    assert same == ((VC.case_id(c), VC.precision(mode)) not in ROW_DIFFERS), (a["row"], b["row"])
    if same:
        assert _same_bits(a["outs"], b["outs"])


@pytest.mark.parametrize("c,mode", RUNS, ids=RUN_IDS)
def test_a_second_run_is_bit_identical(dev, c, mode, monkeypatch):
    """reproducibility: the weight gradient's fixed reduction order, the strips, the per-block partial sums"""
    a = _result(c, mode, "loud", dev, monkeypatch)
    b = _run(c, mode, "loud", dev, monkeypatch)
    assert a["row"] == b["row"] and _same_bits(a["outs"], b["outs"])


def test_k1_unaligned_runs_exactly_on_the_fp32_kernel(dev, monkeypatch):
    """the 1x1 conv the f16x3 plan refuses: the f16x3 run IS the exact run"""
    c = next(x for x in VC.CONV_CASES if x["name"] == "k1_unaligned")
    a, b = _result(c, "exact", "loud", dev, monkeypatch), _result(c, "f16x3", "loud", dev, monkeypatch)
    assert a["row"][0] == b["row"][0] == "exact" and _same_bits(a["outs"], b["outs"])


def test_rows_seen_cover_every_variant_only_windows_reach(dev, monkeypatch):
    """Over all runs the launches reported every SCALED and K1 row of kVariants, the four UP rows of TH 8, both VEC values of every
    weight-gradient kernel, both epilogue-backward kernels, both Winograd kernels and the exact kernel with and without VEC / the
    vector epilogue (a run that has not happened in this session is launched here)."""
    for c, mode in RUNS:
        if (VC.case_id(c), mode) not in SEEN:
            SEEN[(VC.case_id(c), mode)] = _result(c, mode, "loud", dev, monkeypatch)["row"]
    assert VC.coverage(set(SEEN.values())) == []
