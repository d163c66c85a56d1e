#!/usr/bin/env python
"""Time the LPIPS of a sample set -- one GT batch against M samples -- on one GPU: hcflow_amd.lpips.LPIPSMap beside M calls of the
metric.

    python tools/lpips_map_bench.py [--shapes 16x640x640,16x160x160] [--samples 10] [--modes metric,compare,sample_set]
                                    [--rounds 7] [--steps 3] [--warmup 2] [--out profiles/lpips_map_bench.json]

Modes, on the SAME parameter tensors (hcflow_amd.lpips.LPIPS(seed=0)) and the same inputs; one iteration = the whole set:
  metric:     M calls of metric(gt, sr, normalize=True): GT and sample through AlexNet every time (2 B M images);
  compare:    LPIPSMap.embed(gt) + M scalar compare(ref, sr): B (M + 1) images, the same values bit for bit;
  sample_set: LPIPSMap.sample_set(gt) + M add(sr) + result(): compare plus, per sample, the fused map kernel (five bilinear
              upsamplings, their sum, the per-pixel minimum into best_map, the two means) and the set statistics;
  spatial:    embed + M compare(ref, sr, spatial=True): the map kernel storing D instead of updating best_map (not a default mode).
Every configuration is warmed up, then timed with device events around `steps` iterations, `rounds` times, the configurations
ALTERNATING inside each round so that drift of the clocks or of other tenants hits all of them alike. Per configuration one JSON
line: median, min, max of the per-round ms per iteration ("spread_ms" = max - min). One mode is faster than another only if the
medians differ by more than both spreads. "map_kernel_bytes_per_call" is the map kernel's algorithmic traffic for the mode (one
store of D where it is kept; one read and one write of best_map, the first call of a set writes only): divide by the kernel's
time from a `rocprofv3 --kernel-trace --stats` run of this tool (with nothing else traced) for its bandwidth. All lines go to --out.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd.lpips import LPIPS, LPIPSMap  # noqa: E402


def make_step(metric, mapper, mode, gt, samples):
    def step():
        if mode == "metric":
            return torch.stack([metric(gt, s, normalize=True).reshape(-1) for s in samples])
        if mode == "compare":
            ref = mapper.embed(gt, normalize=True)
            return torch.stack([mapper.compare(ref, s).reshape(-1) for s in samples])
        if mode == "spatial":
            ref = mapper.embed(gt, normalize=True)
            return torch.stack([mapper.compare(ref, s, spatial=True)[0].reshape(-1) for s in samples])
        acc = mapper.sample_set(gt, normalize=True, capacity=len(samples))
        for s in samples:
            acc.add(s)
        return acc.result()["lpips"]
    return step


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def map_bytes(mode, B, H, W, M):
    """Algorithmic bytes of ONE map-kernel call, averaged over the M calls of a set (0: the mode launches none)."""
    px = 4 * B * H * W
    return {"spatial": px, "sample_set": px * (2 * M - 1) / M}.get(mode, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x640x640,16x160x160")
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--modes", default="metric,compare,sample_set")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "lpips_map_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lpips_map_bench.py needs a GPU (no CPU timing is meaningful here)")
    metric = LPIPS(seed=0).cuda()
    mapper = LPIPSMap(metric)
    out = []
    with torch.no_grad():
        for shape in a.shapes.split(","):
            B, H, W = (int(v) for v in shape.split("x"))
            g = torch.Generator(device="cuda").manual_seed(1)
            gt = torch.rand(B, 3, H, W, device="cuda", generator=g)
            samples = [(gt + 0.05 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp(0, 1) for _ in range(a.samples)]
            configs = [(m, make_step(metric, mapper, m, gt, samples)) for m in a.modes.split(",")]
            res, times = {}, {m: [] for m, _ in configs}
            for m, fn in configs:                                 # warm-up of every configuration of the shape
                for _ in range(a.warmup):
                    res[m] = fn()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for m, fn in configs:
                    times[m].append(timed(fn, a.steps))
            first = res[configs[0][0]]
            torch.cuda.reset_peak_memory_stats()
            for m, fn in configs:
                fn()
                torch.cuda.synchronize()
                t = times[m]
                r = {"tool": "lpips_map_bench", "mode": m, "shape": [B, 3, H, W], "samples": a.samples, "rounds": a.rounds,
                     "steps": a.steps, "warmup": a.warmup, "median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                     "max_ms": round(max(t), 3), "spread_ms": round(max(t) - min(t), 3),
                     "ms_per_sample": round(statistics.median(t) / a.samples, 3),
                     "images_through_alexnet": B * (2 * a.samples if m == "metric" else a.samples + 1),
                     "map_kernel_bytes_per_call": map_bytes(m, B, H, W, a.samples),
                     "lpips_bit_equal_to_%s" % configs[0][0]: bool(torch.equal(res[m], first)),
                     "peak_mem_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2), "device": torch.cuda.get_device_name(0)}
                torch.cuda.reset_peak_memory_stats()
                print(json.dumps(r), flush=True)
                out.append(r)
            del configs, res, gt, samples, first
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
