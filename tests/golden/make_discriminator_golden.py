#!/usr/bin/env python
"""Fixtures for Discriminator_VGG_128 and PatchGANDiscriminator, generated from the REFERENCE ITSELF (build container only).

    python tests/golden/make_discriminator_golden.py     # writes tests/golden/gan_vgg128.npz, gan_patchgan35.npz, gan_patchgan3.npz

Loads the reference's ``discriminator_vgg_arch.py`` and ``loss.py`` (``torchvision`` stubbed as in make_golden.gen_gan_fixture:
the discriminators do not use it) and runs, on CPU in fp32, one discriminator step of HCFlow_SR_model.optimize_parameters
(:258-285) per net under ``torch.manual_seed`` (the nets' own default initialisation; our classes build the same modules in the
same order, so the GPU box regenerates identical parameters -- ``param_digest`` checks it). Stored: key / shape tables,
predictions, losses, per-parameter gradient digests (and those of the same step in float64), every BatchNorm's running statistics after the step; for the 35-layer
PatchGAN also one generator-side pass (netD frozen but in train(), HCFlow_SR_model.py:237-246): prediction, loss, the digest of
the input gradient and the running statistics after it. Data only; nothing of the reference's code is stored.
"""
import importlib.util as ilu
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, grad_digest, np_  # noqa: E402


def load_reference():
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tv.models)
    mods = []
    for name in ("discriminator_vgg_arch", "loss"):
        spec = ilu.spec_from_file_location("ref_" + name, os.path.join(REF, "models", "modules", name + ".py"))
        m = ilu.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods


def table(net, seed):
    sd = net.state_dict()
    return {"keys": np.array(list(sd.keys())), "shapes": np.array([",".join(str(v) for v in t.shape) for t in sd.values()]),
            "seed": seed,
            "param_digest": np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])}


def running_stats(net, prefix):
    # copies: the numpy view of a CPU buffer would follow the next train() forward
    return {prefix + k: np_(v).copy() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k}


def d_step(net, cri, real, fake):
    """HCFlow_SR_model.py:270-283 without the optimiser: l_d_real + l_d_fake, backward."""
    pred_real, pred_fake = net(real), net(fake)
    l_real, l_fake = cri(pred_real, True), cri(pred_fake, False)
    (l_real + l_fake).backward()
    out = {"pred_real": np_(pred_real), "pred_fake": np_(pred_fake), "l_real": np.float64(float(l_real.detach())),
           "l_fake": np.float64(float(l_fake.detach())),
           "grad_keys": np.array([k for k, _ in net.named_parameters()]),
           "grad_digest": np.array([grad_digest(np_(p.grad), i) for i, (_, p) in enumerate(net.named_parameters())])}
    out.update(running_stats(net, "after_"))
    return out


def f64_digests(make, D, L, seed, gan_type, real, fake, x=None):
    """The same step in float64. The GPU tests hold stock ops in float64 against these digests (the restatement is the
    reference's step) and our gradients against that float64 evaluation with our LeakyReLU sign pattern."""
    torch.manual_seed(seed)
    net = make(D).train().double()
    cri = L.GANLoss(gan_type, 1.0, 0.0)
    (cri(net(real.double()), True) + cri(net(fake.double()), False)).backward()
    out = {"grad_digest_f64": np.array([grad_digest(np_(p.grad), i) for i, (_, p) in enumerate(net.named_parameters())])}
    if x is not None:
        for p in net.parameters():
            p.requires_grad = False
        xd = x.detach().double().requires_grad_(True)
        cri(net(xd), True).backward()
        out["dx_digest_f64"] = np.array(grad_digest(np_(xd.grad), 0))
    return out


def gen(name, make, seed, gan_type, shape, input_seed, g_side=False):
    D, L = load_reference()
    torch.manual_seed(seed)
    net = make(D).train()
    out = table(net, seed)
    g = torch.Generator().manual_seed(input_seed)
    real, fake = torch.rand(*shape, generator=g), torch.rand(*shape, generator=g)
    out.update(d_step(net, L.GANLoss(gan_type, 1.0, 0.0), real, fake), input_seed=input_seed, gan_type=gan_type,
               input_shape=np.array(shape))
    x = None
    if g_side:
        # generator side: netD's parameters frozen, netD still in train() (its running statistics move), gradient to the input
        for p in net.parameters():
            p.requires_grad = False
        x = torch.rand(*shape, generator=g).requires_grad_(True)
        pred = net(x)
        l_g = L.GANLoss(gan_type, 1.0, 0.0)(pred, True)
        l_g.backward()
        out.update(pred_g=np_(pred), l_g=np.float64(float(l_g.detach())), dx_digest=np.array(grad_digest(np_(x.grad), 0)))
        out.update(running_stats(net, "after_g_"))
    out.update(f64_digests(make, D, L, seed, gan_type, real, fake, x))
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024), "l_real %.6f l_fake %.6f" % (out["l_real"], out["l_fake"]))


def main():
    torch.set_num_threads(8)
    gen("gan_vgg128", lambda D: D.Discriminator_VGG_128(3, 64), 123, "gan", (2, 3, 128, 128), 7)
    gen("gan_patchgan35", lambda D: D.PatchGANDiscriminator(3, 64, 35), 321, "lsgan", (2, 3, 96, 96), 8, g_side=True)
    gen("gan_patchgan3", lambda D: D.PatchGANDiscriminator(3, 64, 3), 77, "lsgan", (2, 3, 40, 40), 9)


if __name__ == "__main__":
    main()
