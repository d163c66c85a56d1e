#!/usr/bin/env python
"""Time the discriminators of hcflow_amd.gan beside stock PyTorch on the same GPU.

    python tools/discriminator_bench.py [--case patchgan|vgg128|all] [--modes exact,f16x3,stock] [--steps 10] [--warmup 3]

Per case and mode, two timings (device events around `steps` iterations after `warmup`, one stream):
  d_step: one discriminator step of HCFlow_SR_model.optimize_parameters (:270-283) -- forward on a real and a fake batch, the
          GANLoss (lsgan for PatchGAN, gan for VGG_128), backward into every parameter (no optimiser);
  g_pass: the generator side (:237-246) -- netD frozen but in train(), forward on a batch plus the gradient to that batch.
Cases: PatchGANDiscriminator(3, 64, 35) at B = 16 x 160^2, Discriminator_VGG_128(3, 64) at B = 16 x 128^2.
Modes: "exact" / "f16x3" are our classes (HIP convs + fused BN kernels); "stock" runs the SAME parameter modules through
stock nn ops the way the reference's forward does (nn.Conv2d via MIOpen, nn.BatchNorm2d, nn.LeakyReLU), NCHW fp32.
Prints one JSON line per (case, mode) and, with --out, writes all of them to a JSON file.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import gan  # noqa: E402

CASES = {
    "patchgan": (lambda: gan.PatchGANDiscriminator(3, 64, 35), (16, 3, 160, 160), "lsgan"),
    "vgg128": (lambda: gan.Discriminator_VGG_128(3, 64), (16, 3, 128, 128), "gan"),
}


def stock_forward(net):
    """The reference's forward (discriminator_vgg_arch.py:39-58, :187-189) on net's own stock nn modules."""
    if isinstance(net, gan.PatchGANDiscriminator):
        return net.model
    lrelu = lambda t: F.leaky_relu(t, 0.2)

    def fwd(x):
        fea = lrelu(net.conv0_0(x))
        fea = lrelu(net.bn0_1(net.conv0_1(fea)))
        for i in range(1, 5):
            fea = lrelu(getattr(net, "bn%d_0" % i)(getattr(net, "conv%d_0" % i)(fea)))
            fea = lrelu(getattr(net, "bn%d_1" % i)(getattr(net, "conv%d_1" % i)(fea)))
        fea = lrelu(net.linear1(fea.reshape(fea.size(0), -1)))
        return net.linear2(fea)
    return fwd


def criterion(gan_type):
    def cri(pred, real):
        t = torch.full_like(pred, 1.0 if real else 0.0)
        return F.mse_loss(pred, t) if gan_type == "lsgan" else F.binary_cross_entropy_with_logits(pred, t)
    return cri


def time_it(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def run(case, mode, steps, warmup):
    make, shape, gan_type = CASES[case]
    torch.manual_seed(0)
    net = make().cuda().train()
    if mode != "stock":
        net.set_precision(mode)
    fwd = net if mode != "stock" else stock_forward(net)
    cri = criterion(gan_type)
    g = torch.Generator(device="cuda").manual_seed(1)
    real = torch.rand(shape, device="cuda", generator=g)
    fake = torch.rand(shape, device="cuda", generator=g)
    params = list(net.parameters())

    def d_step():
        for p in params:
            p.requires_grad_(True)
            p.grad = None
        (cri(fwd(real), True) + cri(fwd(fake), False)).backward()

    def g_pass():
        for p in params:
            p.requires_grad_(False)
        x = fake.detach().requires_grad_(True)
        cri(fwd(x), True).backward()

    res = {"case": case, "mode": mode, "shape": list(shape), "steps": steps, "warmup": warmup,
           "d_step_ms": round(time_it(d_step, steps, warmup), 3), "g_pass_ms": round(time_it(g_pass, steps, warmup), 3),
           "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "device": torch.cuda.get_device_name(0)}
    torch.cuda.reset_peak_memory_stats()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=["all"] + list(CASES))
    ap.add_argument("--modes", default="exact,f16x3,stock")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("discriminator_bench.py needs a GPU (no CPU timing is meaningful here)")
    out = []
    for case in (CASES if a.case == "all" else [a.case]):
        for mode in a.modes.split(","):
            r = run(case, mode, a.steps, a.warmup)
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
