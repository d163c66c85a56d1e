#!/usr/bin/env python
"""Time LPIPS as a loss -- forward + backward to ONE input -- on one GPU: hcflow_amd.lpips.LPIPSLoss beside stock PyTorch autograd.

    python tools/lpips_loss_bench.py [--shapes 16x160x160,16x640x640] [--rounds 7] [--steps 10] [--warmup 3]
                                     [--out profiles/r13_lpips_loss_bench.json]

Modes, on the SAME parameter tensors (hcflow_amd.lpips.LPIPS(seed=0)):
  native: LPIPSLoss(metric)(x, gt, normalize=True).backward() -- hcf_lpips_alex + hcf_lpips_alex_backward, exact fp32 MFMA;
  stock:  the same network through nn.functional ops only (F.conv2d via MIOpen, NCHW fp32, max_pool2d, the LPIPS head written
          out) and autograd, as the lpips package runs it.
One iteration = forward + backward to x (gt takes no gradient). Every configuration is warmed up, then timed with device events
around `steps` iterations, `rounds` times, the configurations ALTERNATING inside each round so that drift of the clocks or of other
tenants hits all of them alike. Per configuration one JSON line: median, min, max of the per-round ms per iteration ("spread_ms" =
max - min), the loss value (the modes must agree) and the relative-norm difference of the two gradients. One mode is faster than
the other only if the medians differ by more than both spreads. All lines go to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd.lpips import LPIPS, LPIPSLoss  # noqa: E402


def stock_lpips(metric, x0, x1):
    """mean over the batch of LPIPS(2 x0 - 1, 2 x1 - 1) through nn.functional ops on the metric's own parameters"""
    sl = metric.scaling_layer
    convs = metric.net.convs()

    def feats(x):
        h = ((2 * x - 1) - sl.shift) / sl.scale
        out = []
        for i, c in enumerate(convs):
            if i in (1, 2):
                h = F.max_pool2d(h, 3, 2)
            h = F.relu(F.conv2d(h, c.weight, c.bias, stride=c.stride, padding=c.padding))
            out.append(h)
        return out

    f0, f1 = feats(x0), feats(x1)
    d = 0
    for l in range(5):
        n0 = f0[l] / (f0[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        n1 = f1[l] / (f1[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = d + F.conv2d((n0 - n1) ** 2, getattr(metric, "lin%d" % l).model[1].weight).mean(dim=(1, 2, 3))
    return d.mean()


def make_step(metric, mode, sr, gt):
    crit = LPIPSLoss(metric, reduction="mean")

    def step():
        x = sr.detach().requires_grad_(True)
        loss = crit(x, gt, normalize=True) if mode == "native" else stock_lpips(metric, x, gt)
        loss.backward()
        return loss.detach(), x.grad
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
    ap.add_argument("--shapes", default="16x160x160,16x640x640")
    ap.add_argument("--modes", default="native,stock")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "r13_lpips_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lpips_loss_bench.py needs a GPU (no CPU timing is meaningful here)")
    metric = LPIPS(seed=0).cuda()
    out = []
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        gt = torch.rand(B, 3, H, W, device="cuda", generator=g)
        sr = (gt + 0.05 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp(0, 1)      # an SR sample near its GT
        configs = [(m, make_step(metric, m, sr, gt)) for m in a.modes.split(",")]
        res, times = {}, {m: [] for m, _ in configs}
        for m, fn in configs:
            for _ in range(a.warmup):
                res[m] = fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for m, fn in configs:
                times[m].append(timed(fn, a.steps))
        gref = res[configs[-1][0]][1].double()
        torch.cuda.reset_peak_memory_stats()
        for m, fn in configs:
            fn()
            torch.cuda.synchronize()
            t = times[m]
            r = {"tool": "lpips_loss_bench", "mode": m, "shape": [B, 3, H, W], "rounds": a.rounds, "steps": a.steps,
                 "warmup": a.warmup, "median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                 "max_ms": round(max(t), 3), "spread_ms": round(max(t) - min(t), 3), "loss": float(res[m][0]),
                 "grad_rel_diff_vs_%s" % configs[-1][0]: float((res[m][1].double() - gref).norm() / gref.norm()),
                 "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "device": torch.cuda.get_device_name(0)}
            torch.cuda.reset_peak_memory_stats()
            print(json.dumps(r), flush=True)
            out.append(r)
        del configs, res, gt, sr, gref
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
