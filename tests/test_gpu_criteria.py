"""-m gpu: the training criteria on the device (hcflow_amd/losses.py, hcf_loss.hip) against the float64 oracle
(tests/criteria_oracle.py, which tests/test_criteria_cpu.py holds to the reference-generated fixture), the reference-generated
fixture itself for the caller's GAN sequences, and whole objectives against the same step in the reference's torch expressions.

Gates. A criterion evaluates every term and every sum in fp64 and rounds once, so a value lies within one fp32 ulp of the
float64 value, 2^-23 |ref| (half an ulp from the rounding; the rest covers the oracle's own summation order). A gradient element
is one fp64 product rounded once: 2^-23 |ref| plus one fp32 denormal. The GAN gradients add 1e-12 max|ref| for the cancellation
between the two relativistic paths; at logits of +-100 a BCE value may be a denormal (log1p(exp(-100)) = 3.7e-44), whose rounding
error is absolute: 1e-30 covers it."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import criteria_oracle as O
from tests.util import load_golden, t

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
DENORM = 2.0 ** -149
CAP_N = 1024 * 4096 + 7          # one row just past the 1024 partial blocks a sample may take (4096 floats each), odd

PAIR_SHAPES = [(1, 1, 1, 1), (3, 3, 5, 7), (2, 3, 16, 16), (5, 1, 33, 31), (2, 3, 64, 64), (1, 3, 160, 160), (2, 3, 250, 333),
               (1, 1, 1, CAP_N)]
GAN_TYPES = ["gan", "ragan", "lsgan", "wgan-gp"]
GAN_SHAPES = [(1, 1), (3, 1), (16, 1), (2, 1, 17, 17), (16, 1, 35, 35)]


def L():
    from hcflow_amd import losses
    return losses


def criteria():
    """name -> (module, oracle, kind); kinds 0 / 1 have an exactly zero gradient at d = 0."""
    ls = L()
    out = {}
    for c, kind in (("l1", 0), ("l2", 1)):
        for r in ("mean", "sum", "none"):
            out["pixel_%s_%s" % (c, r)] = (ls.PixelLoss(c, r), functools.partial(O.pixel, criterion=c, reduction=r), kind)
    for lt, kind in (("l2", 1), ("l1", 2)):
        for r in ("mean", "none"):
            out["rec_%s_%s" % (lt, r)] = (ls.ReconstructionLoss(lt, reduction=r),
                                          functools.partial(O.reconstruction, losstype=lt, reduction=r), kind)
    out["rec_l1_eps"] = (ls.ReconstructionLoss("l1", eps=1e-3), functools.partial(O.reconstruction, losstype="l1", eps=1e-3), 2)
    out["charbonnier"] = (ls.CharbonnierLoss(), O.charbonnier, 2)
    return out


CRITERIA = ["pixel_l1_mean", "pixel_l1_sum", "pixel_l1_none", "pixel_l2_mean", "pixel_l2_sum", "pixel_l2_none", "rec_l2_mean",
            "rec_l2_none", "rec_l1_mean", "rec_l1_none", "rec_l1_eps", "charbonnier"]


@functools.lru_cache(maxsize=None)
def pair_inputs(shape):
    """x, y (never modified by a test) with d = 0 at every third element, and one upstream weight per sample."""
    g = torch.Generator().manual_seed(sum(shape) + 17)
    x = torch.rand(shape, generator=g)
    y = torch.rand(shape, generator=g)
    y.view(-1)[1::3] = x.view(-1)[1::3]
    w = torch.rand(shape[0], generator=g) + 0.5
    return x.cuda(), y.cuda(), w.cuda()


def value_close(have, ref, floor=0.0):
    have, ref = have.detach().double().cpu(), ref.detach().double().cpu()
    if ref.numel() == 1 and have.dim() == 0:                           # a fixture scalar comes back as [1]
        ref = ref.reshape(())
    assert have.shape == ref.shape, (have.shape, ref.shape)
    err = (have - ref).abs()
    assert bool((err <= ULP * ref.abs() + floor).all()), (float(err.max()), float(ref.abs().max()))


def grad_close(have, ref, floor=DENORM):
    have, ref = have.detach().double(), ref.detach().double()
    assert have.shape == ref.shape, (have.shape, ref.shape)
    err = (have - ref).abs()
    bad = err > ULP * ref.abs() + floor
    assert not bool(bad.any()), (int(bad.sum()), float(err.max()), float(ref.abs().max()))


def run(cri, x, y, w=None):
    """(value, gx, gy) of the module; a per-sample result is weighted by the upstream vector w."""
    a, b = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    v = cri(a, b)
    (v if v.dim() == 0 else (v * w).sum()).backward()
    return v.detach(), a.grad, b.grad


def run_oracle(fn, x, y, w=None):
    a, b = x.double().requires_grad_(True), y.double().requires_grad_(True)
    v = fn(a, b)
    ga, gb = O.grads(v if v.dim() == 0 else (v * w.double()).sum(), a, b)
    return v.detach(), ga, gb


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_criteria_match_float64(shape):
    """Every kind and every reduction: the value within one ulp, both gradients per element, exact zeros where d = 0."""
    x, y, w = pair_inputs(shape)
    zero = (x == y)
    assert bool(zero.any()) or x.numel() == 1
    for name, (cri, fn, kind) in criteria().items():
        v, gx, gy = run(cri, x, y, w)
        rv, rgx, rgy = run_oracle(fn, x, y, w)
        assert v.dtype == torch.float32 and v.shape == rv.shape, name
        value_close(v, rv)
        grad_close(gx, rgx)
        grad_close(gy, rgy)
        assert torch.equal(gy, -gx), name
        if kind < 2:
            assert not bool(gx[zero].any()) and not bool(gy[zero].any()), name
    assert sorted(criteria()) == sorted(CRITERIA)


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 3, 250, 333)], ids=lambda s: "x".join(map(str, s)))
def test_pair_criteria_are_reproducible_and_independent_of_batch_and_alignment(shape):
    x, y, w = pair_inputs(shape)
    N = x.numel()
    bx, by = torch.empty(N + 1, device="cuda"), torch.empty(N + 3, device="cuda")
    xo, yo = bx[1:].view(shape), by[3:].view(shape)                    # 4 and 12 bytes past a 16-byte boundary
    xo.copy_(x)
    yo.copy_(y)
    assert xo.is_contiguous() and xo.data_ptr() % 16 == 4 and yo.data_ptr() % 16 == 12
    for name, (cri, fn, kind) in criteria().items():
        first = run(cri, x, y, w)
        for a, b in zip(first, run(cri, x, y, w)):                     # two calls: equal bits
            assert torch.equal(a, b), name
        for a, b in zip(first, run(cri, xo, yo, w)):                   # a view at an odd float offset: the bits of the aligned copy
            assert torch.equal(a, b), name
        if first[0].dim() == 1:                                        # row b of 'none' = the one-row call on that row
            for b in range(shape[0]):
                vb, gxb, gyb = run(cri, x[b:b + 1], y[b:b + 1], w[b:b + 1])
                assert torch.equal(vb[0], first[0][b]) and torch.equal(gxb[0], first[1][b]) and torch.equal(gyb[0], first[2][b]), name
        if kind < 2:                                                   # identical inputs: 0 and exact zeros
            v0, gx0, gy0 = run(cri, x, x, w)
            assert not bool(v0.any()) and not bool(gx0.any()) and not bool(gy0.any()), name


def test_no_graph_without_grad_and_noncontiguous_inputs_keep_their_link():
    ls = L()
    x, y, _ = pair_inputs((2, 3, 16, 16))
    assert ls.PixelLoss()(x, y).grad_fn is None
    a = x.clone().requires_grad_(True)
    with torch.no_grad():
        assert ls.PixelLoss()(a, y).grad_fn is None
    at = x.transpose(2, 3).contiguous().requires_grad_(True)           # the criterion sees a transposed (non-contiguous) view
    assert not at.transpose(2, 3).is_contiguous()
    v = ls.PixelLoss("l2")(at.transpose(2, 3), y)
    v.backward()
    rv, rg, _ = run_oracle(functools.partial(O.pixel, criterion="l2"), x, y)
    value_close(v, rv)
    grad_close(at.grad.transpose(2, 3), rg)
    for bad in (lambda: ls.PixelLoss()(x, y[:, :2]), lambda: ls.PixelLoss()(x, y.double()), lambda: ls.PixelLoss()(x, y.cpu()),
                lambda: ls.PixelLoss("l1", "none")(x.view(-1), y.view(-1)), lambda: ls.latent_l2(x, y.half())):
        with pytest.raises(Exception) as e:
            bad()
        assert type(e.value).__name__ == "HcfError"


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_a_nonfinite_element_is_seen_and_finite_sum_drops_the_term(poison):
    ls = L()
    x, y, _ = pair_inputs((2, 3, 250, 333))
    xp = x.clone()
    xp[1, 2, 249, 332] = poison                                        # the last element: the tail behind the last quad
    for name, (cri, fn, kind) in criteria().items():
        v = cri(xp, y)
        assert not bool(torch.isfinite(v).all()), name
        if v.dim() == 1:
            assert bool(torch.isfinite(v[0])), name
    a, b, c = xp.clone().requires_grad_(True), x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    z = (x * 3).requires_grad_(True)
    bad = 2.0 * ls.PixelLoss("l1")(a, y)
    ok1 = 0.5 * ls.ReconstructionLoss("l1")(b, y)
    ok2 = ls.latent_l2(z)
    total, vals = ls.finite_sum(bad, ok1, ok2)
    assert vals.shape == (3,) and not vals.requires_grad and not bool(torch.isfinite(vals[0])) and bool(torch.isfinite(vals[1:]).all())
    assert torch.equal(total.detach(), vals[1] + vals[2])
    total.backward()
    assert not bool(a.grad.any())                                      # exact zeros, also at the poisoned element
    _, rg, _ = run_oracle(functools.partial(O.reconstruction, losstype="l1"), x, y)
    grad_close(b.grad, 0.5 * rg)
    # the latent term is gated the same way
    zp = (xp * 3).requires_grad_(True)
    total, vals = ls.finite_sum(ls.latent_l2(zp, c), ls.PixelLoss("l2")(c, y))
    assert not bool(torch.isfinite(vals[0])) and torch.equal(total.detach(), vals[1])
    total.backward()
    assert not bool(zp.grad.any())
    grad_close(c.grad, run_oracle(functools.partial(O.pixel, criterion="l2"), x, y)[1])


def test_upstream_scalar_on_the_device():
    """w * loss with w a device tensor: the backward reads its upstream gradient on the device."""
    ls = L()
    x, y, _ = pair_inputs((5, 1, 33, 31))
    w = torch.tensor(0.37, device="cuda")
    for name, (cri, fn, kind) in criteria().items():
        if name.endswith("none"):
            continue
        a = x.clone().requires_grad_(True)
        (w * cri(a, y)).backward()
        _, rg, _ = run_oracle(fn, x, y)
        grad_close(a.grad, w.double() * rg)


@functools.lru_cache(maxsize=None)
def latents():
    from hcflow_amd import preset, eps_shapes
    g = torch.Generator().manual_seed(5)
    zs = [torch.randn(s, generator=g) for s in eps_shapes(preset("Rescaling_4X_tiny"), 2, 8, 8)]     # z of a 32 x 32 HR image
    odd = [torch.randn(7, generator=g), torch.randn(3, 5, 67, generator=g) * 2, torch.randn(1, 40001, generator=g)]
    return [z.cuda() for z in zs], [z.cuda() for z in odd]


@pytest.mark.parametrize("which", ["rescaling", "two", "three"])
def test_latent_l2_matches_float64(which):
    ls = L()
    zs, odd = latents()
    ts = {"rescaling": zs, "two": odd[:2], "three": odd}[which]
    leaves = [z.clone().requires_grad_(True) for z in ts]
    v = ls.latent_l2(*leaves)
    v.backward()
    dl = [z.double().requires_grad_(True) for z in ts]
    rv = O.latent_l2(*dl)
    value_close(v, rv)
    for have, ref in zip(leaves, O.grads(rv, *dl)):
        grad_close(have.grad, ref)
    # reproducible; an odd float offset gives the bits of the aligned copy; only the tensors that ask get a gradient
    off = []
    for z in ts:
        buf = torch.empty(z.numel() + 1, device="cuda")
        o = buf[1:].view(z.shape)
        o.copy_(z)
        off.append(o.requires_grad_(True))
    assert off[0].data_ptr() % 16 == 4
    v2 = ls.latent_l2(*off)
    v2.backward()
    assert torch.equal(v2.detach(), v.detach()) and all(torch.equal(a.grad, b.grad) for a, b in zip(off, leaves))
    half = [z.clone().requires_grad_(i == len(ts) - 1) for i, z in enumerate(ts)]
    v3 = ls.latent_l2(*half)
    (torch.tensor(2.0, device="cuda") * v3).backward()
    assert half[0].grad is None and torch.equal(v3.detach(), v.detach())
    grad_close(half[-1].grad, 2.0 * O.grads(rv, *dl)[-1])
    assert ls.latent_l2(*ts).grad_fn is None


def test_latent_l2_matches_the_reference_fixture():
    ls = L()
    g = load_golden("criteria_ref")
    zs = [t(g[k]).cuda().requires_grad_(True) for k in ("z1", "z2", "z3")]
    v = ls.latent_l2(*zs[:2])
    v.backward()
    value_close(v, t(g["lat2_val"]))
    grad_close(zs[0].grad, t(g["lat2_g1"]).cuda())
    grad_close(zs[1].grad, t(g["lat2_g2"]).cuda())
    zs = [t(g[k]).cuda().requires_grad_(True) for k in ("z1", "z2", "z3")]
    v = ls.latent_l2(*zs)
    v.backward()
    value_close(v, t(g["lat3_val"]))
    for z, k in zip(zs, ("lat3_g1", "lat3_g2", "lat3_g3")):
        grad_close(z.grad, t(g[k]).cuda())


def test_pair_criteria_match_the_reference_fixture():
    ls = L()
    g = load_golden("criteria_ref")
    x, y = t(g["x"]).cuda(), t(g["y"]).cuda()
    cases = {"l1": ls.PixelLoss("l1"), "mse": ls.PixelLoss("l2"), "rec_l2": ls.ReconstructionLoss("l2"),
             "rec_l1": ls.ReconstructionLoss("l1"), "rec_l1_eps": ls.ReconstructionLoss("l1", eps=1e-3), "charb": ls.CharbonnierLoss()}
    for name, cri in cases.items():
        v, gx, gy = run(cri, x, y)
        value_close(v, t(g[name + "_val"]))
        grad_close(gx, t(g[name + "_gx"]).cuda())
        grad_close(gy, t(g[name + "_gy"]).cuda())


# ---- GAN criteria ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def logits(shape, seed, span=30.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return ((torch.rand(shape, generator=g) * 2 - 1) * span).cuda()


def gan_grad_close(have, ref):
    grad_close(have, ref, floor=1e-12 * float(ref.abs().max()))


def check_gan(gan_type, labels, pr, pf, floor=0.0):
    """forward(input, real / fake), generator_loss and discriminator_loss of one GANLoss against the oracle."""
    ls = L()
    cri = ls.GANLoss(gan_type, *labels)
    seen = []
    for real in (True, False):
        a = pr.clone().requires_grad_(True)
        v = cri(a, real)
        v.backward()
        d = pr.double().requires_grad_(True)
        rv = O.gan_term(d, real, gan_type, *labels)
        value_close(v, rv, floor)
        gan_grad_close(a.grad, O.grads(rv, d)[0])
        seen.append(v.detach())
    a, b = pf.clone().requires_grad_(True), pr.clone().requires_grad_(True)
    v = cri.generator_loss(a, b)
    v.backward()
    da, db = pf.double().requires_grad_(True), pr.double().requires_grad_(True)
    rv = O.gan_generator(da, db, gan_type, *labels)
    value_close(v, rv, floor)
    gan_grad_close(a.grad, O.grads(rv, da)[0])
    assert b.grad is None                                              # pred_real is detached in the generator step
    seen.append(v.detach())
    a, b = pr.clone().requires_grad_(True), pf.clone().requires_grad_(True)
    tot, logs = cri.discriminator_loss(a, b)
    assert logs.shape == (5,) and not logs.requires_grad and logs.grad_fn is None and torch.equal(tot.detach(), logs[2])
    (torch.tensor(0.5, device="cuda") * tot).backward()
    da, db = pr.double().requires_grad_(True), pf.double().requires_grad_(True)
    rt, rlogs = O.gan_discriminator(da, db, gan_type, *labels)
    value_close(logs, rlogs, floor)
    rga, rgb = O.grads(0.5 * rt, da, db)
    gan_grad_close(a.grad, rga)
    gan_grad_close(b.grad, rgb)
    tot2, logs2 = cri.discriminator_loss(pr, pf)                       # no graph, the same bits
    assert tot2.grad_fn is None and torch.equal(logs2, logs)
    # one of the two predictions alone may ask for a gradient
    b2 = pf.clone().requires_grad_(True)
    cri.discriminator_loss(pr, b2)[0].backward()
    gan_grad_close(b2.grad, 2.0 * rgb)
    return seen + [logs]


@pytest.mark.parametrize("labels", [(1.0, 0.0), (0.9, 0.1)], ids=["hard", "smooth"])
@pytest.mark.parametrize("gan_type", GAN_TYPES)
def test_gan_criteria_match_float64(gan_type, labels):
    for shape in GAN_SHAPES:
        check_gan(gan_type, labels, logits(shape, 1), logits(shape, 2))
    check_gan(gan_type, labels, logits((2, 1, 17, 17), 3), logits((3, 1, 17, 17), 4))          # na != nb


@pytest.mark.parametrize("gan_type", GAN_TYPES)
def test_gan_criteria_stay_finite_at_large_logits(gan_type):
    for shape in [(3, 1), (2, 1, 17, 17)]:
        pr, pf = logits(shape, 5, 100.0).clone(), logits(shape, 6, 100.0).clone()
        pr.view(-1)[0], pr.view(-1)[1], pf.view(-1)[0], pf.view(-1)[1] = 100.0, -100.0, -100.0, 100.0
        for labels in [(1.0, 0.0), (0.9, 0.1)]:
            for v in check_gan(gan_type, labels, pr, pf, floor=1e-30):
                assert bool(torch.isfinite(v).all())
                if gan_type != "wgan-gp":                              # the Wasserstein critic is signed
                    assert bool((v[:3] >= 0).all()) if v.dim() else bool(v >= 0)
    ls = L()
    sat = torch.full((4, 1), 100.0, device="cuda")
    if gan_type in ("gan", "ragan"):                                   # a saturated, correct discriminator: a denormal, not 0 or inf
        v = ls.GANLoss(gan_type)(sat, True)
        ref = O.gan_term(sat.double(), True, gan_type)
        assert 0 < float(ref) < 1e-40 and abs(float(v) - float(ref)) <= 1e-30


@pytest.mark.parametrize("s", ["v", "p"])
@pytest.mark.parametrize("gan_type", GAN_TYPES)
def test_gan_sequences_match_the_reference_fixture(gan_type, s):
    """The literal generator and discriminator sequences of HCFlow_SR_model.py:242-247 / :271-278, run by the reference."""
    ls = L()
    g = load_golden("criteria_ref")
    key = "%s_%s" % (s, gan_type.replace("-", ""))
    pr, pf = t(g[s + "_pr"]).cuda(), t(g[s + "_pf"]).cuda()
    for tag, labels in (("", (1.0, 0.0)), ("_smooth", (0.9, 0.1))):
        cri = ls.GANLoss(gan_type, *labels)
        for real in (True, False):
            a = pr.clone().requires_grad_(True)
            v = cri(a, real)
            v.backward()
            value_close(v, t(g["%s%s_fwd%d_val" % (key, tag, real)]))
            gan_grad_close(a.grad, t(g["%s%s_fwd%d_g" % (key, tag, real)]).cuda())
    cri = ls.GANLoss(gan_type)
    a = pf.clone().requires_grad_(True)
    v = cri.generator_loss(a, pr)
    v.backward()
    value_close(v, t(g[key + "_g_val"]))
    gan_grad_close(a.grad, t(g[key + "_g_gpf"]).cuda())
    a, b = pr.clone().requires_grad_(True), pf.clone().requires_grad_(True)
    tot, logs = cri.discriminator_loss(a, b)
    tot.backward()
    value_close(logs, t(g[key + "_d_logs"]))
    gan_grad_close(a.grad, t(g[key + "_d_gpr"]).cuda())
    gan_grad_close(b.grad, t(g[key + "_d_gpf"]).cuda())


def test_patchgan_lsgan_discriminator_step_matches_the_composed_torch_expression():
    """netD = PatchGANDiscriminator, one D step with GANLoss('lsgan').discriminator_loss against nn.MSELoss on filled labels
    (loss.py:29,44-46) on the SAME module. Both sides run the module's own fp32 backward from upstream gradients that differ by at
    most one fp32 rounding per element (6e-8 relative), and the backward is linear in them: 1e-5 of a tensor's largest gradient
    leaves two decades for cancellation inside a weight gradient. The torch value is an fp32 mean of 968 squares: 1e-6 relative. The two
    logit means are ours against float64: one rounding."""
    from hcflow_amd import gan
    ls = L()
    torch.manual_seed(7)
    netD = gan.PatchGANDiscriminator(3, 16, 3).cuda().train()
    g = torch.Generator().manual_seed(2)
    real, fake = torch.rand(2, 3, 32, 32, generator=g).cuda(), torch.rand(2, 3, 32, 32, generator=g).cuda()
    cri = ls.GANLoss("lsgan")
    netD.zero_grad()
    pr, pf = netD(real), netD(fake)
    assert pr.shape == (2, 1, 22, 22)
    tot, logs = cri.discriminator_loss(pr, pf)
    tot.backward()
    ours = [p.grad.clone() for p in netD.parameters()]
    netD.zero_grad()
    pr2, pf2 = netD(real), netD(fake)
    assert torch.equal(pr2, pr) and torch.equal(pf2, pf)
    l_real = F.mse_loss(pr2, torch.empty_like(pr2).fill_(1.0))
    l_fake = F.mse_loss(pf2, torch.empty_like(pf2).fill_(0.0))
    (l_real + l_fake).backward()
    want = torch.stack([l_real, l_fake, l_real + l_fake]).detach().double()
    assert bool(((logs[:3].double() - want).abs() <= 1e-6 * want.abs()).all()), (logs, want)
    for have, p_ in ((logs[3], pr2), (logs[4], pf2)):                  # D_real / D_fake: a signed mean, relative to the mean magnitude
        assert abs(float(have) - float(p_.detach().double().mean())) <= ULP * float(p_.detach().double().abs().mean())
    for a, p in zip(ours, netD.parameters()):
        assert float((a - p.grad).abs().max()) <= 1e-5 * float(p.grad.abs().max())


def test_quantization_is_metrics_quantize_forward_and_the_identity_backward():
    from hcflow_amd import metrics
    ls = L()
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(2, 3, 17, 23, generator=g) * 1.4 - 0.2).cuda()
    a = x.clone().requires_grad_(True)
    q = ls.Quantization()(a)
    assert torch.equal(q.detach(), metrics.quantize(x)) and torch.equal(ls.Quantization()(x), metrics.quantize(x))
    up = torch.randn(2, 3, 17, 23, generator=g).cuda()
    q.backward(up)
    assert torch.equal(a.grad, up)


def test_rescaling_objective_matches_the_reference_expressions_on_the_same_net():
    """One generator step of HCFlow_Rescaling_model.optimize_parameters (:214-232) on Rescaling_4X_tiny, B = 2, HR 32 x 32: the
    forward, the LR loss, the latent loss, Quantization, the inverse, the HR loss and the finite gate, through the criteria of this
    package and through the reference's torch expressions on the same net. The total within 1e-6 relative; every parameter
    gradient within the gate tests/test_gpu_backward.py::test_rescaling_step_gradients_match_reference holds this net's step to
    (check_grads_against_fixture with rtol = 5e-3, elem_rtol = 3e-2: norms relative to max(norm, 2e-5 of the largest norm), elements
    relative to max(the tensor's largest, 1e-6 of the net's largest) plus 1e-8 of the net's largest)."""
    from hcflow_amd import HCFlowNet_Rescaling, preset, eps_shapes
    from tests.util import cached_params, spec_grads
    ls = L()
    cfg = preset("Rescaling_4X_tiny")
    net = HCFlowNet_Rescaling(opt=cfg.to_opt(), step=0)
    net.load_state_dict(cached_params("Rescaling_4X_tiny", 13), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to("cuda:0").train()
    g = torch.Generator().manual_seed(31)
    hr = torch.rand(2, 3, 32, 32, generator=g).cuda() * 0.8 + 0.1
    lr = F.avg_pool2d(hr, 4)
    eps = [torch.randn(s, generator=g).cuda() for s in eps_shapes(cfg, 2, 8, 8)]
    w_lr, w_z, w_hr = 5e-2, 1e-5, 1.0

    def step(native):
        net.zero_grad()
        fake_lr, z1, z2 = net(hr=hr, u=None, reverse=False)
        if native:
            l_lr = w_lr * ls.ReconstructionLoss("l2")(fake_lr, lr)
            l_z = w_z * ls.latent_l2(z1, z2)
            q = ls.Quantization()(fake_lr)
        else:
            l_lr = w_lr * torch.mean(torch.sum((fake_lr - lr) ** 2, (1, 2, 3)))
            l_z = w_z * (torch.cat([z1.flatten(), z2.flatten()], 0) ** 2).mean()
            q = (torch.clamp(fake_lr, 0, 1) * 255.).round() / 255.
            q = fake_lr + (q - fake_lr).detach()
        fake_h = net(lr=q, z=None, u=None, eps_std=1.0, reverse=True, eps=eps)
        if native:
            l_hr = w_hr * ls.ReconstructionLoss("l1")(fake_h, hr)
            total, vals = ls.finite_sum(l_lr, l_z, l_hr)
        else:
            diff = fake_h - hr
            l_hr = w_hr * torch.mean(torch.sum(torch.sqrt(diff * diff + 1e-6), (1, 2, 3)))
            total = 0
            for term in (l_lr, l_z, l_hr):
                if torch.isfinite(term):
                    total = total + term
            vals = torch.stack([l_lr, l_z, l_hr]).detach()
        total.backward()
        return total.detach().double(), vals.double(), spec_grads(net, cfg)

    tot_a, vals_a, grads_a = step(True)
    tot_b, vals_b, grads_b = step(False)
    assert bool(torch.isfinite(vals_a).all()) and float(tot_b) > 0
    assert abs(float(tot_a) - float(tot_b)) <= 1e-6 * abs(float(tot_b)), (float(tot_a), float(tot_b))
    rtol, elem_rtol = 5e-3, 3e-2
    norms = [float(np.sqrt((np.asarray(b, np.float64) ** 2).sum())) for b in grads_b]
    gmax = max(norms)
    assert gmax > 0
    for i, (a, b) in enumerate(zip(grads_a, grads_b)):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert np.isfinite(a).all(), i
        assert abs(np.sqrt((a ** 2).sum()) - norms[i]) <= rtol * max(norms[i], 2e-5 * gmax), i
        assert np.abs(a - b).max() <= elem_rtol * max(np.abs(b).max(), 1e-6 * gmax) + 1e-8 * gmax, i
