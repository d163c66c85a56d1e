"""-m gpu: the unit boundary of the 64-output-channel Winograd kernel (hcf_conv_wino.h: wino64_epilogue, conv_wino4_kernel) --
the exchange rounds, the residual requests ahead of the entry barrier, the stores issued among the second round's exchange
writes, the per-unit pixel addressing -- on the smallest shapes that reach every path of it, through the per-op conv entry of
tests/test_gpu_wino.py against an fp64 evaluation at that file's tolerances (3e-6 of the reference's maximum; 4e-6 against the
direct f16x3 kernel), plus the two forms only the engine launches (the split second tile of a fat dense-block pair, the fused
1x1 layer of a conditional coupling net) at that file's whole-net tolerance (2e-5 against the exact kernels).

Shapes: one exact unit (8 x 32); ragged in both directions (24 x 40: a column remainder of 8, 40 x 72: rows 8 x 5, a column
remainder of 8 after two full units); more units than any device has CUs (6 x 128 x 128 = 384 units), so that a block walks
several units and the next unit's first chunk is requested across the boundary; 64 / 128 / 192 input channels over one to
three sources; 0, 1 and 2 residuals."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_ops import _rel, _gen

pytestmark = pytest.mark.gpu

# B, H, W, source channels, act, residuals (64 output channels: the v4 kernel)
CASES = [
    (1, 8, 32, [64], None, 0),                  # one exact unit, 4 chunks
    (1, 8, 32, [64, 64, 64], "lrelu", 1),       # ... three sources, 12 chunks, one residual
    (2, 24, 40, [64, 64], "lrelu", 0),          # ragged columns, 8 chunks over two sources
    (2, 24, 40, [64, 128], None, 2),            # ... conv5 with both residuals
    (2, 40, 72, [64], "relu", 1),               # ragged both ways
    (2, 40, 72, [64, 64, 64], None, 2),         # ... three sources, both residuals
    (6, 128, 128, [64], "lrelu", 0),            # 384 units: several per block, the shortest K (boundary share at its largest)
    (6, 128, 128, [64, 64], None, 1),           # ... with a residual
    (6, 128, 128, [64, 128], None, 2),          # ... conv5, both residuals
]


def _ablate(bits):
    from hcflow_amd import _lib
    assert _lib.load().hcf_debug_set_ablation(bits) == 0


@pytest.fixture()
def f16x3_ops():
    from hcflow_amd import ops
    ops.set_precision("f16x3")
    yield ops
    ops.set_precision("exact")
    _ablate(0)


@pytest.mark.parametrize("case", CASES)
def test_wino64_boundary_matches_fp64_and_direct(f16x3_ops, case):
    ops = f16x3_ops
    B, H, W, cs, act, nres = case
    g = _gen(7 * sum(cs) + H + W + nres)
    dev = [torch.randn(B, c, H, W, generator=g).cuda() for c in cs]
    cin = sum(cs)
    w = torch.randn(64, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(64, generator=g) * 0.1
    scale = torch.exp(torch.randn(64, generator=g) * 0.1)
    res = [torch.randn(B, 64, H, W, generator=g).cuda() for _ in range(nres)]
    ref = (F.conv2d(torch.cat(dev, 1).double(), w.double().cuda(), None, 1, 1) + bias.double().cuda().view(1, -1, 1, 1)) \
        * scale.double().cuda().view(1, -1, 1, 1)
    ref = F.relu(ref) if act == "relu" else F.leaky_relu(ref, 0.2) if act == "lrelu" else ref
    kw = {}
    if nres >= 1:
        ref = ref * 0.2 + res[0].double()
        kw.update(res1=res[0], rs1=0.2)
    if nres == 2:
        ref = ref * 0.2 + res[1].double()
        kw.update(res2=res[1], rs2=0.2)
    ref = ref.float()
    _ablate(0)
    out = ops.conv2d(dev, w, bias, scale, act, **kw)
    out2 = ops.conv2d(dev, w, bias, scale, act, **kw)
    _ablate(256)                                           # the direct f16x3 kernel on the same call
    direct = ops.conv2d(dev, w, bias, scale, act, **kw)
    _ablate(0)
    print(case, "rel err vs fp64:", _rel(out, ref), "direct:", _rel(direct, ref), "wino vs direct:", _rel(out, direct))
    assert torch.equal(out, out2)
    assert _rel(out, ref) <= 3e-6, (case, _rel(out, ref))
    assert not torch.equal(out, direct)                    # (different summation: proves the other kernel ran)
    assert _rel(out, direct) <= 4e-6


@pytest.mark.parametrize("sample", [0, 4])
def test_wino64_out_of_range_input_is_reported_from_any_unit(f16x3_ops, sample):
    """An input beyond the f16 range in ONE sample of a launch whose blocks walk several units: the range flag (bit 0 + the
    sample's slot, set in the epilogue from the accumulators) reaches the entry whichever block and round saw it."""
    from hcflow_amd import _lib
    x = torch.ones(5, 64, 64, 128)                          # 5 x 8 x 4 = 160 units
    w = torch.randn(64, 64, 3, 3, generator=_gen(1)) * 0.05
    f16x3_ops.conv2d([x.cuda()], w)                         # in range: no report
    x[sample, 37, 61, 99] = 1.0e5                           # the transformed value overflows the hi part
    with pytest.raises(_lib.HcfError):
        f16x3_ops.conv2d([x.cuda()], w)


def test_range_overflow_behind_the_winograd_convs_reruns_its_sample_only():
    """Whole net (fat pairs with the split second tile, conv5 with residuals, the fused 1x1 form): the per-sample slot of the
    range flag still names the sample -- exactly that one is redone on the exact kernels, the others keep their f16x3 bits."""
    from hcflow_amd.config import eps_shapes
    from tests.test_gpu_engine import _net
    cfg, net = _net("SR_4X_tiny", 11, "f16x3")
    g = torch.Generator().manual_seed(16)
    clean = torch.rand(3, 3, 24, 40, generator=g)
    bad = clean.clone()
    bad[2, 1, 17, 33] = 9.0e4
    eps = [torch.randn(s, generator=g) * 0.5 for s in eps_shapes(cfg, 3, 24, 40)]
    with torch.no_grad():
        ref_clean = net(lr=clean.cuda(), eps_std=0.5, reverse=True, eps=eps)
        n0 = net.engine().fallback_count()
        out = net(lr=bad.cuda(), eps_std=0.5, reverse=True, eps=eps)
        assert net.engine().fallback_count() == n0 + 1
        assert torch.equal(out[0], ref_clean[0]) and torch.equal(out[1], ref_clean[1])
        assert not torch.equal(out[2], ref_clean[2])


def test_engine_forms_split_tile_and_fused_1x1_with_several_units_per_block():
    """The two forms of the boundary that only the engine launches, at a size where blocks walk several units (B = 4 at
    LR 40 x 72: 4 x 20 x 9 = 720 units at the first level, ragged columns): fat dense-block launches whose second tile goes to
    its own tensor (kind 7 completions follow them) and conditional coupling nets' conv1 + 1x1 conv2 in one launch (kind 6),
    144 -> 64. Within the f16x3 tolerance of the exact kernels, bit-reproducible, and no range fallback."""
    from hcflow_amd.config import preset, eps_shapes
    from tests.util import cached_params, maxdiff
    from tests.test_gpu_nets import build_net
    cfg = preset("SR_4X_tiny")
    net = build_net(cfg, cached_params("SR_4X_tiny", 11)).set_precision("exact")
    net.invalidate()
    g = torch.Generator().manual_seed(26)
    B, h, w = 4, 40, 72
    lr = torch.rand(B, 3, h, w, generator=g).cuda()
    eps = [torch.randn(s, generator=g).cuda() * 0.8 for s in eps_shapes(cfg, B, h, w)]
    with torch.no_grad():
        ex = net.reverse_flow_diracLR(lr, None, None, eps_std=0.8, eps=eps, clamp=False)
        net.set_precision("f16x3")
        try:
            eng = net.engine()
            a = net.reverse_flow_diracLR(lr, None, None, eps_std=0.8, eps=eps, clamp=False)
            eng.profile_convs(True)
            b = net.reverse_flow_diracLR(lr, None, None, eps_std=0.8, eps=eps, clamp=False)
            n_fat = sum(e.conv_time(9, 0, kind=7)[1] for e in net.engines())
            n_fcn = sum(e.conv_time(9, 0, kind=6, reset=True)[1] for e in net.engines())
            eng.profile_convs(False)
            assert sum(e.fallback_count() for e in net.engines()) == 0
        finally:
            net.set_precision("exact")
    assert n_fat > 0 and n_fcn > 0, (n_fat, n_fcn)
    assert torch.equal(a, b)
    print("max|f16x3 - exact| =", maxdiff(a, ex), "|exact|max =", float(ex.abs().max()))
    assert maxdiff(a, ex) <= 2e-5 * max(1.0, float(ex.abs().max()))
