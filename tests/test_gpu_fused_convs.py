"""-m gpu: the fused f16x3 conv launches of the default inference path, ONE launch per case, against float64.

Three forms run only inside whole networks otherwise: FCN layers 1 + 2 as the direct FUSE2 rows of kVariants
(hcf_conv_f16x3.hip), the same two layers as the persistent fcn12_kernel<pre> (hcf_conv_fcn.hip), and the Conv2dZeros that
finishes the inverse flow step in its epilogue (the TAILC rows). hcf_op_fcn12 / hcf_op_conv2d_step_inverse launch exactly one of
them and report which (``info``); every case asserts the row it ran, and the rows seen over all cases must be all 13 fused rows
plus both fcn12 instantiations (cases, inputs and references: tests/fused_conv_cases.py).

Error: max |got - ref64| / max(1, max |ref64|) per output tensor. Gate, measured per case: 4 * max(e32, ec, 1e-6), where e32 is
the error of a float32 CPU evaluation of the same composition and ec that of the composed path on kernels pinned elsewhere (FCN:
the f16x3 conv3x3 without Winograd, then the 1x1 conv; tail: the conv, then hcf_op_step_inverse) -- three fp32-class evaluations
that differ in summation order. The gate itself must stay <= 1e-5: a dropped lo term of the f16 split measures 4.9e-5 .. 3.5e-4 on
these inputs (tests/test_fused_convs_cpu.py asserts > 3e-5 for every case and operand).

Measured on an MI355X (err / e32 / ec / gate, worst err : gate ratio of the form):
  case                          err      e32       ec   gate  bit-equal to composed
  fcn-one_tile               1.94e-07 1.89e-07 3.12e-07  4e-06  no
  fcn-ragged_pre             2.59e-07 2.71e-07 3.02e-07  4e-06  no
  fcn-small                  2.23e-07 1.69e-07 1.61e-07  4e-06  no
  fcn-persistent_pre         3.08e-07 3.85e-07 3.29e-07  4e-06  no
  fcn-one_tile_direct        1.64e-07 1.49e-07 1.77e-07  4e-06  no
  fcn-ragged_direct          2.52e-07 2.66e-07 2.68e-07  4e-06  no
  fcn-small_direct            2.4e-07 1.52e-07 2.12e-07  4e-06  no
  fcn-th8_direct             3.03e-07 3.59e-07 2.63e-07  4e-06  no
  fcn-two_sources            5.32e-07  2.8e-07 5.58e-07  4e-06  no
  fcn-upsampled              5.91e-07 3.04e-07 4.94e-07  4e-06  no
  tail-c6_ns3_m0_th4         1.74e-07 1.52e-07 1.53e-07  4e-06  no
  tail-c12_ns6_m0_th4         1.4e-07 1.44e-07  1.4e-07  4e-06  no
  tail-c12_ns3_m0_th4        1.43e-07 1.48e-07 1.43e-07  4e-06  yes
  tail-c24_ns12_m0_th4       1.76e-07 2.12e-07 1.76e-07  4e-06  yes
  tail-c21_ns10_m0_th4       2.14e-07 2.14e-07 2.14e-07  4e-06  yes
  tail-c12_ns3_m1_th4        1.89e-07 1.15e-07 1.89e-07  4e-06  no
  tail-c6_ns3_no_n16_th4     1.58e-07 1.33e-07 1.58e-07  4e-06  yes
  tail-c12_ns6_no_n16_th4     1.7e-07 1.72e-07  1.7e-07  4e-06  yes
  tail-c6_ns3_m0_th8         2.15e-07 1.22e-07 2.15e-07  4e-06  no
  tail-c12_ns6_m0_th8        2.01e-07 1.94e-07 2.01e-07  4e-06  no
  tail-c12_ns3_m0_th8        2.84e-07 2.23e-07 2.84e-07  4e-06  yes
  tail-c24_ns12_m0_th8       2.32e-07 2.32e-07 2.32e-07  4e-06  yes
  tail-c21_ns10_m0_th8       1.58e-07 1.67e-07 1.58e-07  4e-06  yes
  tail-c12_ns3_m1_th8        2.31e-07 9.08e-08 2.57e-07  4e-06  no
  tail-c6_ns3_no_n16_th8     1.61e-07 1.41e-07 1.61e-07  4e-06  yes
  tail-c12_ns6_no_n16_th8    1.33e-07 1.28e-07 1.33e-07  4e-06  yes
  tail-c12_ns6_th8_by_grid   2.09e-07 1.94e-07 2.09e-07  4e-06  no
  tail-c12_ns6_one_tile      1.92e-07 1.53e-07 1.92e-07  4e-06  no
  tail-c6_ns3_small          1.55e-07 9.01e-08 1.55e-07  4e-06  no
  worst err : gate -- persistent fcn12 0.08, direct FUSE2 0.15, fused tail 0.07 (every gate sits on its 1e-6 floor: 4e-6)
A scratch build with deliberately wrong kernels failed every case: one of four K chunks' a_lo b_hi (fcn12) / a_hi b_lo (FUSE2) term
dropped from layer 2 measured err : gate 25 .. 55; in the tail's epilogue one h channel scaled by 1.0001 (16-wide rows) 1.25 .. 3,
the bias dropped from the image's last column (32-wide rows) several thousand.
"""
import contextlib
import math

import pytest
import torch

from tests import fused_conv_cases as FC

pytestmark = pytest.mark.gpu

SEEN = {}            # case id -> the row its launch reported


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _row(info):
    if info["launcher"] == 0:
        return ("fcn12", info["pre"])
    return tuple(info[k] for k in ("ntb", "vec", "up", "fuse2", "tailc", "th", "scaled", "k1", "n16"))


@contextlib.contextmanager
def _ablation(bits):
    from hcflow_amd import _lib
    lib = _lib.load()
    assert lib.hcf_debug_set_ablation(bits) == 0
    try:
        yield
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0


@contextlib.contextmanager
def _f16x3_ops():
    from hcflow_amd import ops
    ops.set_precision("f16x3")
    try:
        with _ablation(FC.ABL_NO_WINO):
            yield
    finally:
        ops.set_precision("exact")


def _sized(c, dev):
    """The persistent-loop case needs more tiles than the launch has blocks (two per CU): raise B on a larger device."""
    if c["name"] != "persistent_pre":
        return c
    per_sample = ((c["H"] + 3) // 4) * ((c["W"] + 31) // 32)
    blocks = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    return dict(c, B=max(c["B"], blocks // per_sample + 1))


def _launch(c, d, dev, mp):
    """The case's one fused launch: (outputs on the CPU, info)."""
    from hcflow_amd import ops
    for k, v in c["env"].items():
        mp.setenv(k, v)
    try:
        with _ablation(c["ablation"]):
            if c["kind"] == "fcn":
                out, info = ops.fcn12([s.to(dev) for s in d["srcs"]], d["w1"], d["bias1"], d["scale1"], d["w2"], d["bias2"], d["scale2"],
                                      pre=None if d["pre"] is None else d["pre"].to(dev), ups=c["ups"], form=c["form"])
                return (out.cpu(),), info
            out, zpad, info = ops.conv2d_step_inverse(d["h2"].to(dev), d["w3"], d["bias3"], d["scale3"], d["z"].to(dev), c["mode"], c["ns"],
                                                      d["mat"], d["an_bias"], d["an_logs"], zpad_n=c["ns"] if c["zpad"] else None)
            return (out.cpu(), None if zpad is None else zpad.cpu()), info
    finally:
        for k in c["env"]:
            mp.delenv(k, raising=False)


def _composed(c, d, dev):
    """The same composition on kernels that have their own fp64 tests."""
    from hcflow_amd import ops
    with _f16x3_ops():
        if c["kind"] == "fcn":
            srcs = [s.to(dev) for s in d["srcs"]]
            if d["pre"] is None:
                h1 = ops.conv2d(srcs, d["w1"], d["bias1"], d["scale1"], "relu", c["ups"])
            else:
                raw = ops.conv2d(srcs, d["w1"], None, None, None, c["ups"])
                h1 = torch.relu(((raw + d["pre"].to(dev)) + d["bias1"].to(dev).view(1, -1, 1, 1)) * d["scale1"].to(dev).view(1, -1, 1, 1))
            return ops.conv2d([h1], d["w2"], d["bias2"], d["scale2"], "relu").cpu()
        h = ops.conv2d([d["h2"].to(dev)], d["w3"], d["bias3"], d["scale3"])
        return ops.step_inverse(d["z"].to(dev), h, c["mode"], c["ns"], d["mat"], d["an_bias"], d["an_logs"]).cpu()


def _check(c, dev, mp):
    c = _sized(c, dev)
    d = FC.make_inputs(c)
    ev = FC.fcn_eval if c["kind"] == "fcn" else (lambda *a, **k: FC.tail_eval(*a, **k)[0])
    ref = ev(c, d)
    e32 = FC.err(ev(c, d, dtype=torch.float32), ref)
    outs, info = _launch(c, d, dev, mp)
    SEEN[FC.case_id(c)] = _row(info)
    assert info["status"] == 0 and info["range_flag"] == 0 and info["block"] == 256
    assert _row(info) == c["row"], info
    comp = _composed(c, d, dev)
    ec, err = FC.err(comp, ref), FC.err(outs[0], ref)
    gate = 4 * max(e32, ec, FC.FLOOR)
    print("%-28s err %.3g  e32 %.3g  ec %.3g  gate %.3g  ratio %.2f  bit-equal to the composed path: %s  grid %d tiles %d"
          % (FC.case_id(c), err, e32, ec, gate, err / gate, bool(torch.equal(outs[0], comp)), info["grid"], info["tiles"]))
    assert torch.isfinite(outs[0]).all()
    assert gate <= FC.CAP, (gate, e32, ec)
    assert err <= gate, (err, gate)
    return c, ref, outs, info, gate


@pytest.mark.parametrize("c", FC.FCN_CASES, ids=FC.case_id)
def test_fcn12_matches_fp64(dev, c, monkeypatch):
    c, _, _, info, _ = _check(c, dev, monkeypatch)
    if c["row"][0] == "fcn12":
        tiles = c["B"] * ((c["H"] + 3) // 4) * ((c["W"] + 31) // 32)
        assert info["tiles"] == tiles and info["grid"] == min(tiles, 2 * torch.cuda.get_device_properties(dev).multi_processor_count)
    if c["name"] == "one_tile":
        assert info["tiles"] == 1
    if c["name"] == "persistent_pre":
        assert info["tiles"] > info["grid"] and info["tiles"] >= 594       # the persistent loop: some block walks two tiles


@pytest.mark.parametrize("c", FC.TAIL_CASES, ids=FC.case_id)
def test_conv2d_step_inverse_matches_fp64(dev, c, monkeypatch):
    c, ref, outs, info, gate = _check(c, dev, monkeypatch)
    th = c["row"][5]
    assert info["grid"] == c["B"] * ((c["H"] + th - 1) // th) * ((c["W"] + 31) // 32)
    if c["zpad"]:
        n = c["ns"]
        want = FC.zpad_of(ref, n)
        e = FC.err(outs[1], want)
        print("%-28s zpad err %.3g" % (FC.case_id(c), e))
        assert e <= gate
        assert torch.equal(outs[1][:, :n], outs[0][:, :n]) and not outs[1][:, n:].any()      # the stored z1, then zeros


def test_direct_form_refuses_a_pre_activation_term(dev):
    """form 1 with ``pre``: plan_conv_f16x3's HCF_ERR_ARG comes back, nothing is substituted, ``out`` is untouched."""
    from hcflow_amd import _lib, ops
    c = dict(FC.FCN_CASES[1], form=1)
    d = FC.make_inputs(c)
    out = torch.full((c["B"], 64, c["H"], c["W"]), 7.0, device=dev)
    with pytest.raises(_lib.HcfError, match="HCF_ERR_ARG") as e:
        ops.fcn12([s.to(dev) for s in d["srcs"]], d["w1"], d["bias1"], d["scale1"], d["w2"], d["bias2"], d["scale2"], pre=d["pre"].to(dev),
                  form=1, out=out)
    assert e.value.status == -1 and e.value.info["launcher"] == 1 and e.value.info["status"] == -1 and e.value.info["grid"] == 0
    assert bool((out == 7.0).all())


def test_a_48_channel_step_is_refused(dev):
    from hcflow_amd import _lib, ops
    c = dict(FC.TAIL_CASES[0], C=48, ns=36, f_out=24, name="c48")
    d = FC.make_inputs(c)
    with pytest.raises(_lib.HcfError, match="HCF_ERR_UNSUPPORTED") as e:
        ops.conv2d_step_inverse(d["h2"].to(dev), d["w3"], d["bias3"], d["scale3"], d["z"].to(dev), c["mode"], c["ns"], d["mat"],
                                d["an_bias"], d["an_logs"])
    assert e.value.status == -6 and e.value.info["launcher"] == 1 and e.value.info["status"] == -6 and e.value.info["range_flag"] == 0


def test_an_input_beyond_the_f16_range_is_reported(dev):
    """One value above 65504 per entry: the launch is made (plan status 0), the range flag comes back, no numbers do."""
    from hcflow_amd import _lib, ops
    c = FC.FCN_CASES[1]
    d = FC.make_inputs(c)
    d["srcs"][0][1, 2, 5, 17] = 1.0e5
    for form, pre in ((0, d["pre"].to(dev)), (1, None)):
        out = torch.full((c["B"], 64, c["H"], c["W"]), 7.0, device=dev)
        with pytest.raises(_lib.HcfError, match="HCF_ERR_UNSUPPORTED") as e:
            ops.fcn12([s.to(dev) for s in d["srcs"]], d["w1"], d["bias1"], d["scale1"], d["w2"], d["bias2"], d["scale2"], pre=pre, form=form,
                      out=out)
        assert e.value.info["launcher"] == form and e.value.info["status"] == 0 and e.value.info["range_flag"] & 1
        assert e.value.info["range_flag"] & (2 << 1), "sample 1 saw it"
        assert bool((out == 7.0).all())
    c = FC.TAIL_CASES[1]
    d = FC.make_inputs(c)
    d["h2"][0, 40, 8, 32] = 1.0e5
    with pytest.raises(_lib.HcfError, match="HCF_ERR_UNSUPPORTED") as e:
        ops.conv2d_step_inverse(d["h2"].to(dev), d["w3"], d["bias3"], d["scale3"], d["z"].to(dev), c["mode"], c["ns"], d["mat"],
                                d["an_bias"], d["an_logs"])
    assert e.value.info["status"] == 0 and e.value.info["range_flag"] & 1 and e.value.info["range_flag"] & (2 << 0)


def test_rows_seen_cover_every_fused_variant(dev, monkeypatch):
    """Over all cases the launches reported all 13 fused rows of kVariants and both fcn12 instantiations (a case that has not run
    in this session is launched here)."""
    for c in FC.CASES:
        if FC.case_id(c) not in SEEN:
            c = _sized(c, dev)
            SEEN[FC.case_id(c)] = _row(_launch(c, FC.make_inputs(c), dev, monkeypatch)[1])
    assert set(SEEN.values()) == FC.ALL_ROWS
    assert len(FC.ALL_ROWS) == 15


def test_fcn_affine3shift_network_matches_oracle(dev):
    """Rescaling_4X_tiny with FCN coupling nets under Affine3shift, f16x3: the shift halves run the shift-3 fused tail without a
    permutation inside a network, and their conv1 reads z[3:], a window the fused FCN forms cannot take (two launches instead).
    Gates of test_random_rescaling_configurations_f16x3_match_oracle."""
    import dataclasses
    from hcflow_amd import HCFlowNet_Rescaling, preset, make_params, eps_shapes
    from hcflow_amd.config import param_spec
    from oracle import hcflow_oracle as O
    cfg = dataclasses.replace(preset("Rescaling_4X_tiny"), nn_module="FCN", hidden=64)
    cfg.validate()
    p = make_params(cfg, 2100)
    net = HCFlowNet_Rescaling(opt=cfg.to_opt(), step=0)
    net.load_state_dict(p, strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).eval().set_precision("f16x3")
    g = torch.Generator().manual_seed(21)
    B, h, w = 2, 10, 18
    hr = torch.rand(B, 3, h * 4, w * 4, generator=g)
    lr = torch.rand(B, 3, h, w, generator=g)
    eps = [torch.randn(s, generator=g) for s in eps_shapes(cfg, B, h, w)]
    lo, z1o, z2o = O.rescale_forward(hr, p, cfg)
    inv_o = O.rescale_inverse(lr, p, cfg, 1.0, eps=eps, clamp=False)
    with torch.no_grad():
        lg, z1g, z2g = net(hr=hr.to(dev), reverse=False)
        eng = net.engine()
        eng.profile_convs(True)
        try:
            inv_g = net.reverse_flow_diracLR(lr.to(dev), None, None, eps_std=1.0, eps=[e.to(dev) for e in eps], clamp=False)
            n_tail = eng.conv_time(9, 0, kind=2)[1]
            n_fcn12 = eng.conv_time(9, 0, kind=5, reset=True)[1]
        finally:
            eng.profile_convs(False)
    assert net.engine().fallback_count() == 0
    # every main step of the 12-channel level (affine and shift halves alternate: f_out 18 / 3) ends in a fused tail, and the
    # affine halves, whose conv1 reads z[:3], still take the persistent two-layer launch
    n_small = sum(1 for k, shp, _ in param_spec(cfg) if k.startswith("flow.layers.") and k.endswith(".actnorm.bias")
                  and ".affine." not in k and shp[1] <= 12)
    assert n_small >= 2 and n_tail >= n_small and n_fcn12 >= 1, (n_small, n_tail, n_fcn12)
    assert float(((lg.cpu() - lo).abs() > 0.5 / 255).float().mean()) <= 1e-3
    assert float((z1g.cpu() - z1o).abs().max()) <= 1e-4 * max(1.0, float(z1o.abs().max()))
    assert float((z2g.cpu() - z2o).abs().max()) <= 1e-4 * max(1.0, float(z2o.abs().max()))
    assert float((inv_g.cpu() - inv_o).abs().max()) <= 1e-4 * max(1.0, float(inv_o.abs().max()))
    assert math.isfinite(float(inv_g.abs().max()))
