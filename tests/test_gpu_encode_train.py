"""-m gpu: the trainable encode -- parameter gradients of z, every eps_l and logp (hcf_train_backward_encode_ex with a gradient
buffer, seed_sum_kernel, the device-scalar form of the log-det jobs, encode(param_grad=True) / _SREncodeStep with parameters,
hcflow_amd.latent.nll_per_sample).

Reference: torch.autograd through the fp32 CPU oracle (tests/encode_oracle.py), per parameter tensor
||g - g_ref|| / max(||g_ref||, 1e-6 * gmax) <= 3e-4, the form and gate of
tests/test_gpu_train_full.py::test_full_depth_gradients_match_oracle_autograd. Every test runs B = 2, LR 10 x 12 (the shapes of
tests/input_grad_cases.py), prints measured error and gate, and shares the oracle runs of tests/encode_train_cases.py."""
import ctypes as C

import pytest
import torch

from tests import encode_train_cases as T
from tests import input_grad_cases as K

pytestmark = pytest.mark.gpu

PRECISIONS = ["exact", "f16x3"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from hcflow_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _net(name, dev, precision, train=False, frozen=False):
    from hcflow_amd import HCFlowNet_SR
    net = HCFlowNet_SR(opt=K._cfg(name).to_opt(), step=0)
    net.load_state_dict(K._params(name), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).set_precision(precision)
    net.train() if train else net.eval()
    if frozen:
        for p in net.parameters():
            p.requires_grad_(False)
    return net


def _counts(net, dev):
    """hcf_train_backward_counts of the forward passes' tape slot."""
    from hcflow_amd import _lib
    eng, _ = net._engine_for(dev)
    _lib.check(eng.lib.hcf_train_select_tape(eng.handle, 0), eng.handle, "hcf_train_select_tape")
    out = (C.c_int64 * 4)()
    _lib.check(eng.lib.hcf_train_backward_counts(eng.handle, out), eng.handle, "hcf_train_backward_counts")
    return [int(v) for v in out]


def _grads(net):
    return {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def _encode_step(net, dev, name, which="all", hr_grad=False):
    """one trainable encode on K.inputs(name, 7): ({key: gradient}, d loss / d hr or None, [z, logp, *eps])"""
    net.zero_grad(set_to_none=True)
    hr = K.inputs(name, 7)[0].to(dev).requires_grad_(hr_grad)
    z, eps, logp = net.encode(hr, param_grad=True)
    assert z.grad_fn is not None and logp.grad_fn is not None and all(e.grad_fn is not None for e in eps), "no graph"
    T.loss_of(which, z, eps, logp).backward()
    return _grads(net), hr.grad, [z.detach(), logp.detach()] + [e.detach() for e in eps]


def _hold(what, got, ref, gate=T.GATE):
    err, key, gmax = T.worst(got, ref)
    print("%s: worst tensor %s, relative error %.3e, gate %.1e, gmax %.3e" % (what, key, err, gate, gmax))
    assert err <= gate, (what, err, key)


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def _taped_is_inference(what, taped, infer, precision):
    """The taped encode's outputs against the inference encode's. exact: bit for bit. f16x3: a taped pass runs the convs without
    the fused epilogues and fused step kernels of the inference path (the backward needs the intermediate tensors), so the two are
    two f16x3 evaluations of one function: each sits within 2e-5 * max(1, |ref|max) of the exact kernels
    (tests/test_gpu_encode.py::test_encode_reruns_an_f16_overflow_exactly), the pair within twice that."""
    for i, (p, q) in enumerate(zip(taped, infer)):
        if precision == "exact":
            assert torch.equal(p, q), "%s: output %d of the taped encode differs from the inference encode's" % (what, i)
        else:
            d, bound = float((p - q).abs().max()), 4e-5 * max(1.0, float(q.abs().max()))
            print("%s output %d: taped against inference max |diff| %.3e, bound %.3e" % (what, i, d, bound))
            assert d <= bound, (what, i, d, bound)


# ---------------------------------------------------------------- 1. parameter gradients against the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", T.NETS)
def test_parameter_gradients_match_oracle(dev, name, precision):
    """smooth_loss over z, every eps_l and logp with unequal per-sample weights on logp: every parameter tensor (the LU net: l, u,
    log_s too) against autograd through tests.encode_oracle.encode. The pass counted its parameter-gradient work."""
    ref = T.encode_param_oracle(name, "all")
    net = _net(name, dev, precision)
    got, g_hr, _ = _encode_step(net, dev, name)
    assert g_hr is None and set(ref) <= set(got)
    _hold("%s %s encode d/d parameters" % (name, precision), got, ref)
    counts = _counts(net, dev)
    print("counts", counts)
    assert counts[0] > 0 and counts[2] > 0 and counts[3] > 0          # (the exact kernels batch no dense-block weight gradient)


# ---------------------------------------------------------------- 2. seeds one at a time
@pytest.mark.parametrize("which", ["logp", "z", "eps"])
def test_one_seed_at_a_time(dev, which):
    name = "SR_4X_tiny"
    ref = T.encode_param_oracle(name, which)
    net = _net(name, dev, "f16x3")
    got, _, _ = _encode_step(net, dev, name, which)
    _hold("%s seed on %s alone" % (name, which), got, ref)
    counts = _counts(net, dev)
    print("counts", counts)
    assert counts[0] > 0 and counts[1] > 0 and counts[2] > 0
    assert (counts[3] > 0) == (which == "logp"), "log-det jobs exactly when logp carries a seed"


# ---------------------------------------------------------------- 3. beside the NLL step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_nll_per_sample_agrees_with_the_nll_step(dev, precision):
    """latent.nll_per_sample(...).mean() is net(hr=, lr=)'s nll for the same noise to 1e-6 relative; its parameter gradients are
    within twice the oracle gate of the NLL step's on the same module (each path is within the gate of the oracle)."""
    from hcflow_amd import latent
    name = "SR_4X_tiny"
    net = _net(name, dev, precision, train=True)
    hr, lr, noise = (t.to(dev) for t in K.inputs(name))
    net.zero_grad(set_to_none=True)
    _, nll = net(hr=hr, lr=lr, reverse=False, noise=noise)
    nll.backward()
    ref = {k: g.cpu() for k, g in _grads(net).items()}
    net.zero_grad(set_to_none=True)
    per = latent.nll_per_sample(net, hr, lr, noise=noise)
    assert tuple(per.shape) == (hr.shape[0],) and per.grad_fn is not None
    mean = per.mean()
    mean.backward()
    rel = abs(float(mean.detach()) - float(nll.detach())) / abs(float(nll.detach()))
    print("%s nll %.9f, nll_per_sample mean %.9f: relative difference %.3e, bound 1.0e-06" % (precision, float(nll), float(mean), rel))
    assert rel <= 1e-6
    _hold("%s nll_per_sample d/d parameters against the NLL step" % precision, _grads(net), ref, 2 * T.GATE)
    with torch.no_grad():
        _, frozen = latent.get_encode_z_and_nll(net, lr, hr, noise=noise)
    assert torch.allclose(per.detach(), frozen, rtol=1e-6, atol=0.0)


# ---------------------------------------------------------------- 4. bit properties
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bit_properties(dev, precision):
    name = "SR_4X_tiny"
    net = _net(name, dev, precision, train=True)
    hr, lr, noise = (t.to(dev) for t in K.inputs(name))
    x = K.inputs(name, 7)[0].to(dev)

    def infer():
        with torch.no_grad():
            z, eps, logp = net.encode(x)
        return [z, logp] + list(eps)

    def nll_step():
        net.zero_grad(set_to_none=True)
        net(hr=hr, lr=lr, reverse=False, noise=noise)[1].backward()
        return _grads(net)

    first = infer()
    assert not any(t.requires_grad for t in first)
    nll_before = nll_step()
    a, none_hr, outs = _encode_step(net, dev, name)
    assert none_hr is None
    _taped_is_inference(precision, outs, first, precision)
    b, _, _ = _encode_step(net, dev, name)
    assert _same(a, b), "two identical calls give different flat gradients"
    with_hr, g_hr, _ = _encode_step(net, dev, name, hr_grad=True)
    assert g_hr is not None and _same(a, with_hr), "the parameter gradients change with the hr gradient beside them"
    counts = _counts(net, dev)
    assert counts[0] > 0 and counts[2] > 0 and counts[3] > 0
    assert _same(nll_before, nll_step()), "an NLL step changed after a trainable encode on the same engine"
    assert all(torch.equal(p, q) for p, q in zip(first, infer())), "an inference call changed after a trainable encode"
    for p in net.parameters():
        p.requires_grad_(False)
    none, g_only, _ = _encode_step(net, dev, name, hr_grad=True)
    assert not none and _counts(net, dev) == [0, 0, 0, 0]
    assert torch.equal(g_only, g_hr), "d/d hr of the full pass differs from the input-gradient-only pass"


def test_backward_on_the_other_tape_does_not_disturb_the_pass_state(dev):
    """An inverse pass taped and differentiated on slot 1 between the encode's forward and its backward: the same gradients."""
    name = "SR_4X_tiny"
    net = _net(name, dev, "f16x3")
    ref, _, _ = _encode_step(net, dev, name)
    net.zero_grad(set_to_none=True)
    x = K.inputs(name, 7)[0].to(dev)
    z, eps, logp = net.encode(x, param_grad=True)
    loss = T.loss_of("all", z, eps, logp)
    lq = K.inputs(name)[1].to(dev)
    sr = net(lr=lq, eps_std=0.7, reverse=True, seed=3)
    inv = torch.autograd.grad(sr.square().mean(), [p for p in net.parameters() if p.requires_grad], allow_unused=True)
    assert any(g is not None and float(g.abs().max()) > 0 for g in inv)
    loss.backward()
    assert _same(ref, _grads(net))


def test_a_wrong_gradient_buffer_is_refused_and_the_tape_survives(dev):
    """A gradient buffer of the wrong length is an argument error before anything runs -- the tape then still serves the backward."""
    name = "SR_4X_tiny"
    net = _net(name, dev, "f16x3")
    ref, _, _ = _encode_step(net, dev, name)
    net.zero_grad(set_to_none=True)
    z, eps, logp = net.encode(K.inputs(name, 7)[0].to(dev), param_grad=True)
    eng, _ = net._engine_for(dev)
    total = sum(p.numel() for p in net._params())
    flat = torch.empty(total, device=dev)
    assert eng.lib.hcf_train_backward_encode_ex(eng.handle, None, None, 0, None, flat.data_ptr(), total - 1, None, None) == -1
    assert b"size mismatch" in eng.lib.hcf_last_error(eng.handle)
    T.loss_of("all", z, eps, logp).backward()
    assert _same(ref, _grads(net))


# ---------------------------------------------------------------- 5. the kernels
@pytest.mark.parametrize("B", [1, 2, 5, 64, 21845])
def test_seed_sum_op(dev, B):
    """seed_sum_kernel: the float64 sum rounded to fp32, bit for bit, twice."""
    from hcflow_amd import ops
    g = (torch.randn(B, generator=torch.Generator().manual_seed(900 + B)) * 3.0).to(dev)
    want = g.cpu().double().sum().float()
    got, again = ops.seed_sum(g), ops.seed_sum(g)
    print("B = %d: %.9e, float64 sum %.9e" % (B, float(got), float(want)))
    assert torch.equal(got.cpu().view(()), want) and torch.equal(got, again)


@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("n", [6, 21, 45 * 45])
def test_axpy_job_device_scalar_op(dev, n, with_x):
    """A job whose device scalar holds the float the host form is given writes the host form's bits (alpha = 1); both are
    y + k * (x or 1) of float64 within fp32 rounding; alpha * *k_dev multiplies as two floats do."""
    from hcflow_amd import ops
    gen = torch.Generator().manual_seed(70 + n + with_x)
    y = torch.randn(n, generator=gen).to(dev)
    x = torch.randn(n, generator=gen).to(dev) if with_x else None
    k = torch.randn(1, generator=gen) * 37.0
    host = ops.axpy_job(x, y, float(k))
    scal = ops.axpy_job(x, y, 1.0, k_dev=k.to(dev))
    assert torch.equal(host, scal), "the device-scalar form differs from the host form"
    xs = x.cpu().double() if with_x else torch.ones(n, dtype=torch.float64)
    want = y.cpu().double() + k.double() * xs
    err = float((host.cpu().double() - want).abs().max())
    bound = 2e-7 * float(want.abs().max() + (k.double() * xs).abs().max())
    print("n = %d x %s: max |diff| to float64 %.3e, bound %.3e" % (n, with_x, err, bound))
    assert err <= bound
    hw = 120.0                                            # H * W of a level, times the seed sum on the device
    assert torch.equal(ops.axpy_job(x, y, hw, k_dev=k.to(dev)), ops.axpy_job(x, y, float(torch.tensor(hw) * k[0])))


# ---------------------------------------------------------------- 6. the module
def test_encode_trains_the_net(dev):
    """Trainable weights, a plain hr: outputs with a grad_fn; five hcflow_amd.optim.Adam steps on the latent regulariser
    0.5 mean(z^2) + sum_l 0.5 mean(eps_l^2) give finite, decreasing losses; the next inference call sees the updated weights."""
    from hcflow_amd.optim import Adam
    name = "SR_4X_tiny"
    net = _net(name, dev, "f16x3", train=True)
    hr = K.inputs(name, 7)[0].to(dev)
    with torch.no_grad():
        z0 = net.encode(hr)[0]
    opt = Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        z, eps, logp = net.encode(hr, param_grad=True)
        assert z.grad_fn is not None and logp.grad_fn is not None and all(e.grad_fn is not None for e in eps)
        loss = 0.5 * (z ** 2).mean() + sum(0.5 * (e ** 2).mean() for e in eps)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses:", " ".join("%.6e" % v for v in losses))
    assert all(v == v and abs(v) < float("inf") for v in losses)
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    z_t = net.encode(hr, param_grad=True)[0].detach()
    with torch.no_grad():
        z_i = net.encode(hr)[0]
    _taped_is_inference("after the steps", [z_t], [z_i], "f16x3")
    moved = float((z_i - z0).abs().max())
    print("the inference z moved by %.3e over the steps" % moved)
    assert moved > 1e-3


def test_untrained_actnorms_are_refused_in_train_mode(dev):
    name = "SR_4X_tiny"
    net = _net(name, dev, "f16x3", train=True)
    m = next(m for m in net.modules() if "ActNorm" in type(m).__name__)
    with torch.no_grad():
        m.bias.zero_()
    m.inited = False
    hr = K.inputs(name, 7)[0].to(dev)
    with pytest.raises(NotImplementedError, match="ActNorm"):
        net.encode(hr, param_grad=True)
    with torch.no_grad():
        assert not net.encode(hr)[0].requires_grad                  # the inference path does not fit them and does not mind
    net.eval()
    assert net.encode(hr, param_grad=True)[0].grad_fn is not None
    assert net.encode(hr)[0].grad_fn is None                        # without the keyword: the inference path, as ever
