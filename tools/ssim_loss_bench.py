#!/usr/bin/env python
"""Time SSIMLoss (hcflow_amd/losses.py, hcf_ssim.hip) forward + backward to one input beside a stock-torch SSIM on one GPU.

    python tools/ssim_loss_bench.py [--rounds 7] [--steps 20] [--warmup 3] [--out profiles/ssim_loss_bench.json]
    python tools/ssim_loss_bench.py --once 8x3x640x640      # one forward + backward of the native node only (for a kernel trace)

At 16 x 3 x 160^2 and 8 x 3 x 640^2, on the same inputs (x requires a gradient, y does not), three sides:
  hcf         SSIMLoss()(x, y) + backward                    one node, fp64 terms from the fp32 inputs
  torch_fp32  tests/ssim_loss_oracle.py's expression         five grouped 11 x 11 conv2d's under autograd, in float32
  torch_fp64  the same expression on float64 copies          (what the GPU tests use as their reference, on the CPU)
Every side is warmed up, then timed with device events around `steps` iterations, `rounds` times, the sides ALTERNATING inside
each round; per side the median, min and max of the per-round ms per iteration. "peak_extra_bytes": the allocator's peak above
what was live before one iteration (inputs excluded, gradients and temporaries included). "accuracy": each side's value and
gradient against the float64 side on `y = x + 1e-3 * randn` (where a refinement loop ends up), the gradient relative to max|g|.
One side is "faster" than another only if the medians differ by more than both spreads; no threshold is set anywhere.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import losses  # noqa: E402
from tests import ssim_loss_oracle as O  # noqa: E402

SHAPES = [(16, 3, 160, 160), (8, 3, 640, 640)]
SIDES = ("hcf", "torch_fp32", "torch_fp64")


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


def make_inputs(shape):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(shape, generator=g, dtype=torch.float64)
    y = (x + 1e-3 * torch.randn(shape, generator=g, dtype=torch.float64)).float().cuda()
    return x.float().cuda().requires_grad_(True), y


def cases(shape):
    x, y = make_inputs(shape)
    x64, y64 = x.detach().double().requires_grad_(True), y.double()
    cri = losses.SSIMLoss()

    def run(leaf, value):
        leaf.grad = None
        value.backward()
        return value.detach(), leaf.grad

    return {"hcf": lambda: run(x, cri(x, y)), "torch_fp32": lambda: run(x, O.ssim_loss(x, y)),
            "torch_fp64": lambda: run(x64, O.ssim_loss(x64, y64))}


def stats(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "ssim_loss_bench.json"))
    ap.add_argument("--once", default=None, help="BxCxHxW: one native forward + backward, nothing timed or written")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ssim_loss_bench needs the GPU"
    if a.once:
        fn = cases(tuple(int(v) for v in a.once.split("x")))["hcf"]
        fn()
        torch.cuda.synchronize()
        v, _ = fn()
        torch.cuda.synchronize()
        print("once", a.once, "loss", float(v))
        return
    rows = []
    for shape in SHAPES:
        fns = cases(shape)
        for fn in fns.values():
            for _ in range(a.warmup):
                fn()
        ref_v, ref_g = fns["torch_fp64"]()
        acc, mem = {}, {}
        for side in SIDES:
            v, g = fns[side]()
            acc[side] = {"value_abs_err": abs(float(v.double() - ref_v)),
                         "grad_err_over_max_grad": float((g.double() - ref_g).abs().max() / ref_g.abs().max())}
            mem[side] = peak_extra(fns[side])
        t = {side: [] for side in SIDES}
        for _ in range(a.rounds):
            for side in SIDES:
                t[side].append(timed(fns[side], a.steps))
        row = {"shape": "x".join(map(str, shape)), "loss": float(ref_v), "max_grad": float(ref_g.abs().max())}
        for side in SIDES:
            row[side] = dict(stats(t[side]), peak_extra_bytes=mem[side], accuracy=acc[side])
        h = row["hcf"]
        for other in SIDES[1:]:
            r = row[other]
            row["hcf_vs_" + other] = ("hcf faster" if h["max_ms"] < r["min_ms"] else other + " faster" if r["max_ms"] < h["min_ms"]
                                      else "neither (spreads overlap)")
        rows.append(row)
        for side in SIDES:
            r = row[side]
            print("%-14s %-11s %.4f ms (%.4f-%.4f) %11d B | value err %.2e, grad err / max|g| %.2e" % (
                row["shape"], side, r["median_ms"], r["min_ms"], r["max_ms"], r["peak_extra_bytes"],
                r["accuracy"]["value_abs_err"], r["accuracy"]["grad_err_over_max_grad"]), flush=True)
    out = {"tool": "tools/ssim_loss_bench.py", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "steps": a.steps,
           "warmup": a.warmup, "timing": "forward + backward to x per iteration, device events, sides alternating per round",
           "inputs": "x uniform in [0, 1], y = x + 1e-3 * randn, both rounded to fp32", "rows": rows}
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
