#!/usr/bin/env python
"""Generate tests/golden/criteria_ref.npz from the REFERENCE ITSELF (runs only in the build container, on the CPU).

Imports the reference's ``models/modules/loss.py`` (read-only, never copied) and runs its classes, and the literal expressions
its two callers build around them (HCFlow_SR_model.py:242-247 / :271-278, HCFlow_Rescaling_model.py:215-220), in float64 on
small fp32-representable inputs. The file holds data only: inputs, values, and the gradient to every input.

    python tests/golden/make_criteria_golden.py
"""
import importlib.util as ilu
import os

import numpy as np
import torch
import torch.nn as nn

REF = "/root/reference/codes"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "criteria_ref.npz")
GAN_TYPES = ["gan", "ragan", "lsgan", "wgan-gp"]


def reference_loss_module():
    spec = ilu.spec_from_file_location("ref_loss", os.path.join(REF, "models", "modules", "loss.py"))
    mod = ilu.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def leaf(a):
    return torch.from_numpy(a).double().requires_grad_(True)


def g_step(cri, gan_type, pred_g_fake, pred_d_real):
    """HCFlow_SR_model.py:242-247 (l_gan_w = 1)."""
    if gan_type in ["gan", "lsgan", "wgan-gp"]:
        return cri(pred_g_fake, True)
    pred_d_real = pred_d_real.detach()
    return (cri(pred_d_real - torch.mean(pred_g_fake), False) + cri(pred_g_fake - torch.mean(pred_d_real), True)) / 2


def d_step(cri, gan_type, pred_d_real, pred_d_fake):
    """HCFlow_SR_model.py:271-278."""
    if gan_type in ["gan", "lsgan", "wgan-gp"]:
        l_d_real = cri(pred_d_real, True)
        l_d_fake = cri(pred_d_fake, False)
        l_d_total = l_d_real + l_d_fake
    else:
        l_d_real = cri(pred_d_real - torch.mean(pred_d_fake), True)
        l_d_fake = cri(pred_d_fake - torch.mean(pred_d_real), False)
        l_d_total = (l_d_real + l_d_fake) / 2
    return l_d_real, l_d_fake, l_d_total


def main():
    L = reference_loss_module()
    rng = np.random.RandomState(20240)
    out = {}

    # ---- pair criteria on a [3, 3, 5, 7] pair (n = 105: odd), d = 0 at every third element
    x = rng.rand(3, 3, 5, 7).astype(np.float32)
    y = rng.rand(3, 3, 5, 7).astype(np.float32)
    y.reshape(-1)[1::3] = x.reshape(-1)[1::3]
    out["x"], out["y"] = x, y
    crits = {"l1": nn.L1Loss(), "mse": nn.MSELoss(), "rec_l2": L.ReconstructionLoss("l2"), "rec_l1": L.ReconstructionLoss("l1"),
             "rec_l1_eps": L.ReconstructionLoss("l1", eps=1e-3), "charb": L.CharbonnierLoss()}
    for name, cri in crits.items():
        a, b = leaf(x), leaf(y)
        v = cri(a, b)
        v.backward()
        out[name + "_val"], out[name + "_gx"], out[name + "_gy"] = v.detach().numpy(), a.grad.numpy(), b.grad.numpy()

    # ---- latent term, HCFlow_Rescaling_model.py:216 (l_w_z = 1)
    z1 = rng.randn(2, 9, 4, 4).astype(np.float32)
    z2 = rng.randn(2, 36, 2, 2).astype(np.float32) * 3
    z3 = rng.randn(7).astype(np.float32)
    out["z1"], out["z2"], out["z3"] = z1, z2, z3
    a, b = leaf(z1), leaf(z2)
    v = (torch.cat([a.flatten(), b.flatten()], 0) ** 2).mean()
    v.backward()
    out["lat2_val"], out["lat2_g1"], out["lat2_g2"] = v.detach().numpy(), a.grad.numpy(), b.grad.numpy()
    a, b, c = leaf(z1), leaf(z2), leaf(z3)
    v = (torch.cat([a.flatten(), b.flatten(), c.flatten()], 0) ** 2).mean()
    v.backward()
    out["lat3_val"], out["lat3_g1"], out["lat3_g2"], out["lat3_g3"] = v.detach().numpy(), a.grad.numpy(), b.grad.numpy(), c.grad.numpy()

    # ---- GAN criteria: [3, 1] (VGG discriminators) and [2, 1, 5, 5] (PatchGAN) logits, na != nb in the second set
    sets = {"v": (rng.randn(3, 1).astype(np.float32) * 4, rng.randn(3, 1).astype(np.float32) * 4),
            "p": (rng.randn(2, 1, 5, 5).astype(np.float32) * 4, rng.randn(3, 1, 5, 5).astype(np.float32) * 4)}
    for s, (pr, pf) in sets.items():
        out["%s_pr" % s], out["%s_pf" % s] = pr, pf
        for gt in GAN_TYPES:
            key = "%s_%s" % (s, gt.replace("-", ""))
            for tag, (rl, fl) in (("", (1.0, 0.0)), ("_smooth", (0.9, 0.1))):
                cri = L.GANLoss(gt, rl, fl)
                for real in (True, False):                              # forward(input, target_is_real)
                    a = leaf(pr)
                    v = cri(a, real)
                    v.backward()
                    out["%s%s_fwd%d_val" % (key, tag, real)], out["%s%s_fwd%d_g" % (key, tag, real)] = v.detach().numpy(), a.grad.numpy()
            cri = L.GANLoss(gt, 1.0, 0.0)
            a, b = leaf(pf), leaf(pr)
            v = g_step(cri, gt, a, b)
            v.backward()
            out[key + "_g_val"], out[key + "_g_gpf"] = v.detach().numpy(), a.grad.numpy()
            a, b = leaf(pr), leaf(pf)
            lr_, lf_, lt_ = d_step(cri, gt, a, b)
            lt_.backward()
            out[key + "_d_logs"] = np.array([float(v_.detach()) for v_ in (lr_, lf_, lt_, a.mean(), b.mean())])
            out[key + "_d_gpr"], out[key + "_d_gpf"] = a.grad.numpy(), b.grad.numpy()

    np.savez_compressed(OUT, **out)
    print("wrote %s: %d arrays, %d bytes" % (OUT, len(out), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
