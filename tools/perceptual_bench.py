#!/usr/bin/env python
"""Time the HCFlow++ feature loss  cri_fea(netF(fake_H), netF(real_H).detach())  forward + backward to fake_H on one GPU.

    python tools/perceptual_bench.py [--modes fused,composed,stock] [--precisions exact,f16x3] [--rounds 7] [--steps 20]
                                     [--warmup 3] [--criterion l1] [--out profiles/r10_perceptual_bench.json]

Shape: B = 16 x 3 x 160 x 160 (the HCFlow++ recipes' GT batch), VGGFeatureExtractor(feature_layer=34, use_bn=False).
Modes, all on the SAME parameter modules:
  fused:    hcflow_amd.gan.PerceptualLoss -- one autograd node, glue on the kernels of hcf_vgg.hip;
  composed: F.l1_loss(netF(fake), netF(real).detach()) on hcflow_amd.gan.VGGFeatureExtractor -- our convs, stock PyTorch glue;
  stock:    the same expression through nn ops only (nn.Conv2d via MIOpen, NCHW fp32), as the reference runs it.
fused and composed run at each precision ("exact" / "f16x3" forward convs; the data gradient is fp32 MFMA in both); stock has none.
One iteration = forward + backward to fake_H. Every configuration is warmed up, then timed with device events around `steps`
iterations, `rounds` times, the configurations ALTERNATING inside each round so that drift of the clocks or of other tenants
hits all of them alike. Per configuration one JSON line: median, min, max of the per-round ms per iteration ("spread_ms" =
max - min), and the loss value (the modes must agree). fused is faster than composed only if the medians differ by more than
both spreads. All lines go to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import gan  # noqa: E402

SHAPE = (16, 3, 160, 160)


def make_netF():
    torch.manual_seed(0)
    net = gan.VGGFeatureExtractor(feature_layer=34, use_bn=False, use_input_norm=True, device=torch.device("cuda")).cuda().eval()
    with torch.no_grad():       # variance-preserving weights: the default init shrinks the activations to ~1e-8 over 16 layers
        for m in net.features:
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, nonlinearity="relu")
                m.bias.normal_(0, 0.05)
    return net


def make_step(netF, mode, precision, criterion, fake, real):
    cri = {"l1": F.l1_loss, "l2": F.mse_loss}[criterion]
    fused = gan.PerceptualLoss(netF, criterion=criterion)

    def step():
        if mode != "stock":
            netF.set_precision(precision)
        x = fake.detach().requires_grad_(True)
        if mode == "fused":
            loss = fused(x, real)
        elif mode == "composed":
            loss = cri(netF(x), netF(real).detach())
        else:
            loss = cri(netF.features((x - netF.mean) / netF.std), netF.features((real - netF.mean) / netF.std).detach())
        loss.backward()
        return loss.detach()
    return step


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="fused,composed,stock")
    ap.add_argument("--precisions", default="exact,f16x3")
    ap.add_argument("--criterion", default="l1", choices=["l1", "l2"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r10_perceptual_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("perceptual_bench.py needs a GPU (no CPU timing is meaningful here)")
    netF = make_netF()
    g = torch.Generator(device="cuda").manual_seed(1)
    fake = torch.rand(SHAPE, device="cuda", generator=g)
    real = torch.rand(SHAPE, device="cuda", generator=g)
    configs = []
    for mode in a.modes.split(","):
        for prec in (a.precisions.split(",") if mode != "stock" else ["fp32"]):
            configs.append((mode, prec, make_step(netF, mode, prec, a.criterion, fake, real)))
    losses, times = {}, {(m, p): [] for m, p, _ in configs}
    for mode, prec, fn in configs:
        for _ in range(a.warmup):
            losses[(mode, prec)] = float(fn())
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for mode, prec, fn in configs:
            times[(mode, prec)].append(timed(fn, a.steps))
    torch.cuda.reset_peak_memory_stats()
    out = []
    for mode, prec, fn in configs:
        fn()
        torch.cuda.synchronize()
        t = times[(mode, prec)]
        r = {"tool": "perceptual_bench", "mode": mode, "precision": prec, "criterion": a.criterion, "shape": list(SHAPE),
             "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "median_ms": round(statistics.median(t), 3),
             "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "spread_ms": round(max(t) - min(t), 3),
             "loss": losses[(mode, prec)], "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2),
             "device": torch.cuda.get_device_name(0)}
        torch.cuda.reset_peak_memory_stats()
        print(json.dumps(r), flush=True)
        out.append(r)
    netF.set_precision("exact")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
