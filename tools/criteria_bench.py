#!/usr/bin/env python
"""Time the device training criteria (hcflow_amd/losses.py) forward + backward beside the reference's torch expressions on one GPU.

    python tools/criteria_bench.py [--rounds 7] [--steps 50] [--warmup 5] [--out profiles/criteria_bench.json]

Pair criteria at 16 x 3 x 160^2 and 8 x 3 x 640^2, on the same inputs (the input requires a gradient, the target does not):
  pixel_l1 / pixel_l2   PixelLoss('l1' / 'l2')           beside nn.L1Loss() / nn.MSELoss()
  rec_l2 / rec_l1       ReconstructionLoss('l2' / 'l1')  beside loss.py:84 / :86-87 as written
  charbonnier           CharbonnierLoss()                beside loss.py:13-14
  latent_l2             latent_l2(z1, z2)                beside HCFlow_Rescaling_model.py:216 (z shapes of an HR image of that size)
  pixel_l1_gated        the HR pixel step of HCFlow_SR_model.py:210-216 as the caller runs it -- isnan(fake_H).any(), the loss,
                        .item(), backward -- beside finite_sum(w * PixelLoss) + backward + one values.tolist()
GAN discriminator step (HCFlow_SR_model.py:271-287, both predictions require a gradient) at [16, 1] and [16, 1, 17, 17]:
  gan_d / ragan_d       GANLoss(t).discriminator_loss + backward + logs.tolist()   beside the reference's sequence of GANLoss
                        calls (restated: empty_like().fill_() + BCEWithLogitsLoss), four .item() / mean reads, the isnan gate
Every configuration is warmed up, then timed with device events around `steps` iterations, `rounds` times, the two sides
ALTERNATING inside each round; per side the median, min and max of the per-round ms per iteration. "peak_extra_bytes": the
allocator's peak above what was live before one iteration (inputs excluded, gradients and temporaries included). One side is
"faster" only if the medians differ by more than both spreads; no threshold is set anywhere.
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
from hcflow_amd import losses  # noqa: E402

PAIR_SHAPES = [(16, 3, 160, 160), (8, 3, 640, 640)]
GAN_SHAPES = [(16, 1), (16, 1, 17, 17)]


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def bwd(leaves, value):
    for v in leaves:
        v.grad = None
    value.backward()


def pair_cases(shape):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape, generator=g).cuda().requires_grad_(True)
    y = torch.rand(shape, generator=g).cuda()
    B, _, H, W = shape
    z1 = torch.randn(B, 6, H // 2, W // 2, generator=g).cuda().requires_grad_(True)
    z2 = torch.randn(B, 21, H // 4, W // 4, generator=g).cuda().requires_grad_(True)
    eps = 1e-6
    ours = {"pixel_l1": losses.PixelLoss("l1"), "pixel_l2": losses.PixelLoss("l2"), "rec_l2": losses.ReconstructionLoss("l2"),
            "rec_l1": losses.ReconstructionLoss("l1", eps), "charbonnier": losses.CharbonnierLoss(eps)}
    l1, l2 = nn.L1Loss(), nn.MSELoss()

    def rec_l1(a, b):
        diff = a - b
        return torch.mean(torch.sum(torch.sqrt(diff * diff + eps), (1, 2, 3)))

    def charb(a, b):
        diff = a - b
        return torch.sum(torch.sqrt(diff * diff + eps))
    ref = {"pixel_l1": l1, "pixel_l2": l2, "rec_l2": lambda a, b: torch.mean(torch.sum((a - b) ** 2, (1, 2, 3))), "rec_l1": rec_l1,
           "charbonnier": charb}
    cases = {}
    for name in ours:
        cases[name] = (lambda c=ours[name]: bwd([x], c(x, y)), lambda c=ref[name]: bwd([x], c(x, y)))
    cases["latent_l2"] = (lambda: bwd([z1, z2], losses.latent_l2(z1, z2)),
                          lambda: bwd([z1, z2], (torch.cat([z1.flatten(), z2.flatten()], 0) ** 2).mean()))
    w = 1.0

    def gated_ours():
        total, vals = losses.finite_sum(w * ours["pixel_l1"](x, y))
        bwd([x], total)
        return vals.tolist()

    def gated_ref():
        x.grad = None
        total = 0
        if not torch.isnan(x).any():
            l_pix = w * l1(x, y)
            total += l_pix
            log = l_pix.item()
        if total != 0:
            total.backward()
        return log
    cases["pixel_l1_gated"] = (gated_ours, gated_ref)
    return cases


class RefGANLoss(nn.Module):
    """loss.py:19-51 for 'gan' / 'ragan', restated for the timing only."""

    def __init__(self):
        super().__init__()
        self.loss = nn.BCEWithLogitsLoss()

    def forward(self, input, target_is_real):
        return self.loss(input, torch.empty_like(input).fill_(1.0 if target_is_real else 0.0))


def gan_cases(shape):
    g = torch.Generator().manual_seed(2)
    pr = (torch.randn(shape, generator=g) * 3).cuda().requires_grad_(True)
    pf = (torch.randn(shape, generator=g) * 3).cuda().requires_grad_(True)
    ref = RefGANLoss()
    cases = {}
    for gt in ("gan", "ragan"):
        cri = losses.GANLoss(gt)

        def ours(cri=cri):
            total, logs = cri.discriminator_loss(pr, pf)
            gate, _ = losses.finite_sum(total)
            bwd([pr, pf], gate)
            return logs.tolist()

        def theirs(gt=gt):
            pr.grad = pf.grad = None
            if gt == "gan":
                l_r, l_f = ref(pr, True), ref(pf, False)
                tot = l_r + l_f
            else:
                l_r, l_f = ref(pr - torch.mean(pf), True), ref(pf - torch.mean(pr), False)
                tot = (l_r + l_f) / 2
            log = [l_r.item(), l_f.item(), float(torch.mean(pr.detach())), float(torch.mean(pf.detach()))]
            if not torch.isnan(tot):
                tot.backward()
            return log
        cases[gt + "_d"] = (ours, theirs)
    return cases


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "criteria_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "criteria_bench needs the GPU"
    rows = []
    groups = [("x".join(map(str, s)), pair_cases(s)) for s in PAIR_SHAPES] + [("x".join(map(str, s)), gan_cases(s)) for s in GAN_SHAPES]
    for shape, cases in groups:
        for name, (ours, ref) in cases.items():
            for fn in (ours, ref):
                for _ in range(a.warmup):
                    fn()
            mem = {"hcf": peak_extra(ours), "torch": peak_extra(ref)}
            t = {"hcf": [], "torch": []}
            for _ in range(a.rounds):
                t["hcf"].append(timed(ours, a.steps))
                t["torch"].append(timed(ref, a.steps))
            row = {"shape": shape, "criterion": name}
            for side in ("hcf", "torch"):
                row[side] = dict(stats(t[side]), peak_extra_bytes=mem[side])
            h, r = row["hcf"], row["torch"]
            row["faster"] = "hcf" if h["max_ms"] < r["min_ms"] else "torch" if r["max_ms"] < h["min_ms"] else "neither (spreads overlap)"
            rows.append(row)
            print("%-14s %-16s hcf %.4f ms (%.4f-%.4f) %9d B | torch %.4f ms (%.4f-%.4f) %9d B | %s" % (
                shape, name, h["median_ms"], h["min_ms"], h["max_ms"], h["peak_extra_bytes"], r["median_ms"], r["min_ms"], r["max_ms"],
                r["peak_extra_bytes"], row["faster"]), flush=True)
    out = {"tool": "tools/criteria_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "warmup": a.warmup, "timing": "forward + backward per iteration, device events, sides alternating per round", "rows": rows}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
