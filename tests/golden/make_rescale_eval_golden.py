#!/usr/bin/env python
"""Generate tests/golden/rescale_eval_tiny.npz from the REFERENCE ITSELF (runs only in the build container).

    python tests/golden/make_rescale_eval_golden.py

The two tensors the rescaling test loop needs beside net_rescale_tiny*.npz (tests/test_gpu_rescale_eval.py,
tests/test_rescale_eval_cpu.py), from the same seeded nets and the same inputs, through the reference's own modules
(imported read-only by make_golden.import_reference, never copied):

    <net>_q0_out / _q0_raw   netG(lr=Quantization()(LR^), eps_std=0, reverse=True), clamped / through the flow alone: the inverse of
                             HCFLowRescalingModel.test() (HCFlow_Rescaling_model.py:306-324) at heat 0, which draws nothing
    <net>_z1_b1              fake_z1 of the batch-of-ONE forward call of every image, stacked [B, ...]
    <net>_z1_mean_b1         fake_z1.mean() of those calls as float32 [B]: the value test() returns (:324), the "nll" column

Data only (tiny net outputs); the weights come from the seeded recipe, the inputs from net_rescale_tiny*.npz."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from hcflow_amd.config import preset  # noqa: E402

NETS = ["net_rescale_tiny", "net_rescale_tiny_lu"]


def main():
    torch.set_num_threads(1)
    _, ref_rs = MG.import_reference()
    from models.modules import Basic
    out = {}
    for name in NETS:
        g = np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)
        cfg = preset(str(g["preset"]))
        net, _ = MG.build(ref_rs, cfg, int(g["seed"]))
        hr = torch.from_numpy(g["hr"])
        with torch.no_grad():
            lr_hat, z1, _ = net(hr=hr, reverse=False)
            assert torch.equal(lr_hat, torch.from_numpy(g["fwd_lr"])) and torch.equal(z1, torch.from_numpy(g["fwd_z1"])), name
            lrq = Basic.Quantization()(lr_hat)
            assert torch.equal(lrq, torch.from_numpy(g["rt_lrq"])), name
            with MG.Capture() as cap:
                y = net(lr=lrq, eps_std=0.0, reverse=True)
            eps = cap.normal
            assert all(float(e.abs().max()) == 0.0 for e in eps), "heat 0 draws zeros"
            with MG.Capture(replay_normal=eps):
                y_raw = net.flow(z=lrq, eps_std=0.0, reverse=True)
            assert torch.equal(torch.clamp(y_raw, 0, 1), y)
            z1_b1, means = [], []
            for b in range(hr.shape[0]):
                _, zb, _ = net(hr=hr[b:b + 1], reverse=False)
                z1_b1.append(zb)
                means.append(zb.mean().item())                     # HCFlow_Rescaling_model.py:324
            z1_b1 = torch.cat(z1_b1, 0)
        out[name + "_q0_out"] = MG.np_(y)
        out[name + "_q0_raw"] = MG.np_(y_raw)
        out[name + "_z1_b1"] = MG.np_(z1_b1)
        out[name + "_z1_mean_b1"] = np.array(means, dtype=np.float32)
        print("  %s: heat-0 raw range [%.3f, %.3f], z1 means %s, z1 batch-of-one == batched: %s" % (
            name, float(y_raw.min()), float(y_raw.max()), means, bool(torch.equal(z1_b1, z1))))
    path = os.path.join(HERE, "rescale_eval_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
