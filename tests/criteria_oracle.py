"""An independent float64 restatement of the training criteria (hcflow_amd/losses.py), differentiable by torch autograd, on
whatever device its inputs live. tests/test_criteria_cpu.py holds it to the reference-generated fixture
(tests/golden/criteria_ref.npz) at 1e-12 relative; the GPU tests use it at the sizes the fixture does not cover. Written from
the formulas, not from the reference's code: sums over explicit axes, the logistic loss through softplus."""
import torch
import torch.nn.functional as F


def _d(x, y):
    return x.double() - y.double()


def _rows(v, reduction_rows):
    return v.reshape(v.shape[0], -1).sum(1) if reduction_rows else v.sum()


def pixel(x, y, criterion="l1", reduction="mean"):
    d = _d(x, y)
    t = d.abs() if criterion == "l1" else d * d
    if reduction == "none":
        return _rows(t, True) / (t.numel() // t.shape[0])
    return t.sum() / t.numel() if reduction == "mean" else t.sum()


def reconstruction(x, y, losstype="l2", eps=1e-6, reduction="mean"):
    d = _d(x, y)
    t = d * d if losstype == "l2" else (d * d + eps).sqrt()
    rows = _rows(t, True)
    return rows if reduction == "none" else rows.sum() / rows.numel()


def charbonnier(x, y, eps=1e-6):
    d = _d(x, y)
    return (d * d + eps).sqrt().sum()


def latent_l2(*ts):
    return sum((t.double() ** 2).sum() for t in ts) / sum(t.numel() for t in ts)


def gan_term(v, target_is_real, gan_type, real=1.0, fake=0.0):
    """mean over the logits v (float64) of the criterion of `gan_type` against the label of `target_is_real`."""
    if gan_type == "wgan-gp":
        return -v.mean() if target_is_real else v.mean()
    t = real if target_is_real else fake
    if gan_type == "lsgan":
        return ((v - t) ** 2).mean()
    return (t * F.softplus(-v) + (1.0 - t) * F.softplus(v)).mean()      # -t log s(v) - (1 - t) log(1 - s(v))


def gan_generator(pred_fake, pred_real, gan_type, real=1.0, fake=0.0):
    pf = pred_fake.double()
    if gan_type != "ragan":
        return gan_term(pf, True, gan_type, real, fake)
    pr = pred_real.double().detach()
    return 0.5 * (gan_term(pr - pf.mean(), False, gan_type, real, fake) + gan_term(pf - pr.mean(), True, gan_type, real, fake))


def gan_discriminator(pred_real, pred_fake, gan_type, real=1.0, fake=0.0):
    """(total, [l_real, l_fake, total, D_real, D_fake])."""
    pr, pf = pred_real.double(), pred_fake.double()
    if gan_type != "ragan":
        l_r, l_f = gan_term(pr, True, gan_type, real, fake), gan_term(pf, False, gan_type, real, fake)
        tot = l_r + l_f
    else:
        l_r, l_f = gan_term(pr - pf.mean(), True, gan_type, real, fake), gan_term(pf - pr.mean(), False, gan_type, real, fake)
        tot = 0.5 * (l_r + l_f)
    return tot, torch.stack([l_r.detach(), l_f.detach(), tot.detach(), pr.detach().mean(), pf.detach().mean()])


def grads(value, *inputs):
    """d value / d inputs (float64 tensors; None where an input does not reach the value). The graph is kept: a test may ask again."""
    return torch.autograd.grad(value, inputs, allow_unused=True, retain_graph=True)
