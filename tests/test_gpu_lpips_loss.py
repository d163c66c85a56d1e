"""-m gpu: hcflow_amd.lpips.LPIPSLoss (forward: the metric's own hcf_lpips_alex call; backward: hcf_lpips_alex_backward).

Values are pinned bit for bit to ``LPIPS.forward``. Gradients are held to float64 CPU autograd over
``tests.lpips_oracle.alex_features`` plus the LPIPS head written out below (``lpips_oracle.lpips_alex`` detaches its inputs).
The gate is measured, not fixed: per case ``e32`` is the relative-norm deviation of FLOAT32 CPU autograd of the same
restatement from the float64 oracle (over the gradients of both inputs together), and every sample of every input must meet
``||g - g64|| / ||g64|| <= 8 * max(e32, 1e-6)``: both are fp32 evaluations that differ in summation order only (dot products
of up to 3 456 terms), the head's cancellation amplifies both alike, and the floor guards against a lucky ``e32``. The upstream
gradient is per sample and non-uniform (``w = linspace(0.5, 1.5, B)``), so a mis-indexed ``gout`` shows.

The kernel DEFINES the gradient through the norm of an all-zero feature vector as 0 where autograd gives NaN; every case
asserts that the oracle has no such pixel, so the two agree on what is compared.
"""
import pytest
import torch
import torch.nn.functional as F

from hcflow_amd import _lib
from hcflow_amd.lpips import LPIPS, LPIPSLoss
from tests import lpips_oracle as O

pytestmark = pytest.mark.gpu

GATE_FACTOR, E32_FLOOR = 8.0, 1e-6
# the smallest shapes at which each kernel can still go wrong: AlexNet's minimum (pool2 output 1x1, Hs = 8 against H1 = 7);
# two spare s2d rows, one spare column, neither side a multiple of 4; H1 = 24 even (the last conv1 row is in no pool window)
SHAPES = [(1, 3, 31, 31), (2, 3, 33, 47), (3, 3, 100, 132)]
KINDS = ["random", "sr", "near"]


@pytest.fixture(scope="module")
def metric():
    return LPIPS(seed=0).cuda()


@pytest.fixture(scope="module")
def sd():
    return LPIPS(seed=0).state_dict()


def _pair(shape, kind, seed, unit=False):
    """x0, x1 in [-1, 1] (unit: in [0, 1]); sr: x1 = clamp(x0 + 0.05 randn); near: 1e-3, the cancellation regime of the head"""
    g = torch.Generator().manual_seed(seed)
    lo = 0.0 if unit else -1.0
    x0 = torch.rand(shape, generator=g) * (1 - lo) + lo
    if kind == "random":
        x1 = torch.rand(shape, generator=g) * (1 - lo) + lo
    else:
        x1 = (x0 + {"sr": 0.05, "near": 1e-3}[kind] * torch.randn(shape, generator=g)).clamp(lo, 1)
    return x0, x1


def _features(x, sd, dtype):
    """tests.lpips_oracle.alex_features in `dtype` (that one casts the parameters to float64 itself)"""
    if dtype == torch.float64:
        return O.alex_features(x, sd)
    g = lambda k: sd[k].detach().to("cpu", dtype)
    w = [(g(k + ".weight"), g(k + ".bias")) for k in O.CONV_KEYS]
    h1 = F.relu(F.conv2d(x, *w[0], stride=4, padding=2))
    h2 = F.relu(F.conv2d(F.max_pool2d(h1, 3, 2), *w[1], padding=2))
    h3 = F.relu(F.conv2d(F.max_pool2d(h2, 3, 2), *w[2], padding=1))
    h4 = F.relu(F.conv2d(h3, *w[3], padding=1))
    h5 = F.relu(F.conv2d(h4, *w[4], padding=1))
    return [h1, h2, h3, h4, h5]


def _cpu_grads(x0, x1, sd, normalize, dtype):
    """(dL/dx0, dL/dx1, zero-norm pixels) of L = sum_b w_b d(x0, x1)_b by CPU autograd in `dtype`"""
    a, b = x0.detach().to("cpu", dtype).requires_grad_(True), x1.detach().to("cpu", dtype).requires_grad_(True)
    shift, scale = sd["scaling_layer.shift"].to("cpu", dtype), sd["scaling_layer.scale"].to("cpu", dtype)
    pre = (lambda t: 2 * t - 1) if normalize else (lambda t: t)
    f0, f1 = _features((pre(a) - shift) / scale, sd, dtype), _features((pre(b) - shift) / scale, sd, dtype)
    d, zero = 0, 0
    for l in range(5):
        s0, s1 = f0[l].pow(2).sum(1, keepdim=True), f1[l].pow(2).sum(1, keepdim=True)
        zero += int((s0 == 0).sum()) + int((s1 == 0).sum())
        n0, n1 = f0[l] / (s0.sqrt() + 1e-10), f1[l] / (s1.sqrt() + 1e-10)
        d = d + F.conv2d((n0 - n1) ** 2, sd["lin%d.model.1.weight" % l].to("cpu", dtype)).mean(dim=(1, 2, 3))
    w = torch.linspace(0.5, 1.5, x0.shape[0], dtype=dtype)
    (w * d).sum().backward()
    return a.grad, b.grad, zero


def _gpu_grads(metric, x0, x1, normalize, need=(True, True), reduction="none"):
    a = x0.cuda().requires_grad_(need[0])
    b = x1.cuda().requires_grad_(need[1])
    d = LPIPSLoss(metric, reduction=reduction)(a, b, normalize=normalize)
    w = torch.linspace(0.5, 1.5, x0.shape[0], device="cuda")
    (w * d.reshape(-1)).sum().backward() if reduction == "none" else d.backward()
    return a.grad, b.grad


def _check_against_oracle(metric, sd, x0, x1, normalize, tag):
    g64 = _cpu_grads(x0, x1, sd, normalize, torch.float64)
    assert g64[2] == 0, "%s: the oracle has %d pixels with an all-zero feature vector" % (tag, g64[2])
    g32 = _cpu_grads(x0, x1, sd, normalize, torch.float32)
    ref = torch.cat([g64[0].reshape(-1), g64[1].reshape(-1)])
    e32 = float((torch.cat([g32[0].reshape(-1), g32[1].reshape(-1)]).double() - ref).norm() / ref.norm())
    gate = GATE_FACTOR * max(e32, E32_FLOOR)
    got = _gpu_grads(metric, x0, x1, normalize)
    worst = 0.0
    for i in range(2):
        assert got[i].dtype == torch.float32 and got[i].shape == x0.shape and bool(torch.isfinite(got[i]).all())
        for b in range(x0.shape[0]):
            r = g64[i][b]
            worst = max(worst, float((got[i][b].double().cpu() - r).norm() / r.norm()))
    print("lpips-loss-vs-oracle %s: e32 %.3e, gate %.3e, worst per-sample rel-norm error %.3e (%.3f of the gate)"
          % (tag, e32, gate, worst, worst / gate))
    assert worst <= gate, (tag, worst, gate)


# ---- 1. values
@pytest.mark.parametrize("normalize", [False, True])
def test_values_are_the_metrics_bit_for_bit(metric, normalize):
    x0, x1 = _pair((3, 3, 50, 61), "random", 1, unit=normalize)
    x0, x1 = x0.cuda(), x1.cuda()
    want = metric(x0, x1, normalize=normalize)
    a, b = x0.clone().requires_grad_(True), x1.clone().requires_grad_(True)
    none = LPIPSLoss(metric, reduction="none")(a, b, normalize=normalize)
    assert none.shape == (3, 1, 1, 1) and none.requires_grad and torch.equal(none.detach(), want)
    assert torch.equal(LPIPSLoss(metric, "mean")(a, b, normalize=normalize).detach(), want.mean())
    assert torch.equal(LPIPSLoss(metric, "sum")(a, b, normalize=normalize).detach(), want.sum())
    assert torch.equal(LPIPSLoss(metric)(a, b, normalize=normalize).detach(), want.mean())       # the default is "mean"


def test_no_grad_and_detached_inputs_keep_no_tape(metric):
    x0, x1 = _pair((2, 3, 64, 64), "random", 2)
    x0, x1 = x0.cuda(), x1.cuda()
    want = metric(x0, x1)
    crit = LPIPSLoss(metric, reduction="none")
    tape_bytes = _lib.load().hcf_lpips_workspace(2, 64, 64)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        d1 = crit(x0.clone().requires_grad_(True), x1)
    d2 = crit(x0, x1)
    for d in (d1, d2):
        assert torch.equal(d, want) and d.grad_fn is None and not d.requires_grad
    assert torch.cuda.memory_allocated() - base < tape_bytes          # only the two [B] results are still alive
    d3 = crit(x0.clone().requires_grad_(True), x1)
    assert d3.grad_fn is not None and torch.cuda.memory_allocated() - base >= tape_bytes


# ---- 2. gradients against the oracle
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gradients_match_the_fp64_oracle(metric, sd, shape, kind):
    x0, x1 = _pair(shape, kind, seed=shape[2] * 7 + shape[3])
    _check_against_oracle(metric, sd, x0, x1, False, "%s %s" % (kind, "x".join(map(str, shape))))


@pytest.mark.parametrize("kind", ["random", "sr"])
def test_gradients_match_the_fp64_oracle_normalize(metric, sd, kind):
    x0, x1 = _pair((2, 3, 33, 47), kind, seed=5, unit=True)       # inputs in [0, 1]: the factor 2 of 2x - 1 matters
    _check_against_oracle(metric, sd, x0, x1, True, "%s normalize 2x3x33x47" % kind)


def test_float16_inputs_get_float16_gradients(metric):
    x0, x1 = _pair((2, 3, 33, 47), "sr", seed=6, unit=True)
    h0, h1 = x0.half(), x1.half()
    want = _gpu_grads(metric, h0.float(), h1.float(), True)
    got = _gpu_grads(metric, h0, h1, True)
    for g, w in zip(got, want):                                   # the fp32 gradient of the same values, rounded once
        assert g.dtype == torch.float16 and torch.equal(g, w.half())


# ---- 3. which input gets a gradient
def test_either_input_or_both(metric):
    x0, x1 = _pair((2, 3, 33, 47), "sr", seed=7)
    both = _gpu_grads(metric, x0, x1, False, (True, True))
    only0 = _gpu_grads(metric, x0, x1, False, (True, False))
    only1 = _gpu_grads(metric, x0, x1, False, (False, True))
    assert only0[1] is None and only1[0] is None
    assert torch.equal(only0[0], both[0]) and torch.equal(only1[1], both[1])
    assert float(both[0].abs().max()) > 0 and float(both[1].abs().max()) > 0


# ---- 4. gradient properties
def test_gradient_is_bit_reproducible_and_independent_of_the_batch(metric):
    x0, x1 = _pair((8, 3, 72, 90), "random", seed=11)
    full = _gpu_grads(metric, x0, x1, False, (True, False), reduction="sum")[0]
    again = _gpu_grads(metric, x0, x1, False, (True, False), reduction="sum")[0]
    assert torch.equal(full, again)
    for b in (0, 3, 7):
        one = _gpu_grads(metric, x0[b:b + 1], x1[b:b + 1], False, (True, False), reduction="sum")[0]
        assert torch.equal(one, full[b:b + 1])


# ---- 5. identical inputs
def test_identical_inputs_give_an_exactly_zero_gradient(metric):
    x = _pair((2, 3, 40, 52), "random", seed=3)[0]
    g0, g1 = _gpu_grads(metric, x, x.clone(), False)
    for g in (g0, g1):
        assert bool(torch.isfinite(g).all()) and bool((g == 0).all())


# ---- 6. through the generator
def _tiny_netG():
    from hcflow_amd import HCFlowNet_SR, preset, make_params
    cfg = preset("SR_4X_tiny")
    netG = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    netG.load_state_dict(make_params(cfg, 11), strict=True)
    for m in netG.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    netG = netG.cuda().train()
    netG.set_precision("exact")
    return netG


def test_generator_step(metric):
    netG = _tiny_netG()
    gen = torch.Generator().manual_seed(1)
    lr = torch.rand(2, 3, 8, 8, generator=gen).cuda()
    gt = torch.rand(2, 3, 32, 32, generator=gen).cuda()
    crit = LPIPSLoss(metric)
    seen = []
    fake = netG(lr=lr, z=None, u=None, eps_std=0.8, reverse=True, seed=5)
    assert fake.shape == gt.shape
    fake.register_hook(seen.append)
    crit(fake, gt, normalize=True).backward()
    grads = [p.grad for p in netG.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    leaf = fake.detach().clone().requires_grad_(True)
    crit(leaf, gt, normalize=True).backward()
    assert len(seen) == 1 and torch.equal(seen[0], leaf.grad)


def test_plugs_into_latent_optimise(metric):
    """The caller-supplied loss of hcflow_amd.latent.optimise: the encoding of a seeded image with eps perturbed, 10 Adam steps on
    LPIPS to the image. Every loss is finite and positive, and the loss has fallen."""
    from hcflow_amd import latent
    netG = _tiny_netG()
    gen = torch.Generator().manual_seed(21)
    hr = torch.rand(2, 3, 40, 48, generator=gen).cuda()
    with torch.no_grad():
        z, eps, _ = netG.encode(hr)
    eps_p = [e + 0.3 * torch.randn(e.shape, generator=gen).cuda() for e in eps]
    crit = LPIPSLoss(metric)
    _, _, losses = latent.optimise(netG, z, eps_p, lambda out: crit(out, hr, normalize=True), 10)
    print("lpips losses:", " ".join("%.4e" % v for v in losses))
    assert len(losses) == 10 and all(0 < v < float("inf") for v in losses)
    assert losses[-1] < losses[0], losses


# ---- 7. failure modes
def test_failure_modes(metric):
    crit = LPIPSLoss(metric)
    x = torch.rand(1, 3, 40, 40, requires_grad=True)
    with pytest.raises(_lib.HcfError):
        crit(x, x.detach())                                        # CPU inputs
    y = torch.rand(1, 3, 30, 64, device="cuda", requires_grad=True)
    with pytest.raises(_lib.HcfError):
        crit(y, y.detach())                                        # H = 30
    z = torch.rand(1, 3, 40, 40, device="cuda", requires_grad=True)
    with pytest.raises(_lib.HcfError):
        crit(z, torch.rand(1, 3, 40, 44, device="cuda"))           # mismatched shapes
    with pytest.raises(_lib.HcfError):
        LPIPSLoss(LPIPS())(z, z.detach())                          # parameters still on the CPU
    tuned = LPIPS(seed=0).cuda()
    tuned.lin0.model[1].weight.requires_grad_(True)
    with pytest.raises(ValueError):
        LPIPSLoss(tuned)(z, z.detach())
    with pytest.raises(ValueError):
        LPIPSLoss(metric, reduction="batchmean")
    with pytest.raises(_lib.HcfError):
        metric(z, z.detach())                                      # the metric itself is unchanged: still no backward
