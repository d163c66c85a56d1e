#!/usr/bin/env python
"""Time metrics.PairMetrics (GT prepared once, device-resident rows) against the one-shot metrics.psnr_ssim on one GPU.

    python tools/pair_metrics_bench.py [--parts pairs,sweep] [--shapes 16x640x640,16x160x160,1x1356x2040] [--samples 10]
                                       [--preset SR_DF2K_4X] [--lr-size 160] [--heats 11] [--n-sample 5]
                                       [--rounds 7] [--steps 1] [--warmup 2] [--kernel-stats FILE.csv]
                                       [--out profiles/pair_metrics_bench.json]
    python tools/pair_metrics_bench.py --trace-run 16x640x640          # embed + M compares once, for a profiler to wrap

(a) pairs: M samples against one GT (crop 4, scale 4), generated once and held by the tool, per shape BxHxW:
  psnr_ssim:   M metrics.psnr_ssim calls, the one-shot wrapper per sample (each allocates, prepares the GT again, compares,
               synchronises and reads back): what preparing the GT on every call costs;
  pair:        PairMetrics.embed + M compare calls into one [M,B,8] device buffer, one synchronise at the end;
  sample_set:  PairMetrics.sample_set + M add + result() + the one readback of "mean".
  "peak_extra_mb": torch.cuda.max_memory_allocated over one iteration minus what was allocated before it (torch cannot see
  psnr_ssim's own hipMalloc calls: the reference buffer and workspace that `pair` gets from torch).
  "compares_ms": the M compare calls alone between device events (launch gaps included, not a kernel time).
  "equals_psnr_ssim": the last sample's rows equal psnr_ssim's exactly (one computation; the tool stops if they do not).
(b) sweep: loader.evaluate_sweep on ONE LR image WITH its GT, `heats` temperatures, `n_sample` samples each, seeded random
  weights.
--kernel-stats: the kernel statistics (or kernel trace) CSV of ONE profiler run of --trace-run (kernel trace only, no counters);
the total time of the kernels named pair_* joins the output per kernel, and summed over the compare kernels as
"compare_kernels_ms".
Every configuration is warmed up, then timed (host clock around `steps` iterations ending in a device synchronise) `rounds`
times, the configurations of a part ALTERNATING inside each round. Per configuration one JSON line: median, min, max of the
per-round ms per iteration. One is faster than the other only if the medians differ by more than both spreads."""
import argparse
import csv
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import HCFlowNet_SR, make_params, metrics, preset  # noqa: E402
from hcflow_amd.loader import evaluate_sweep  # noqa: E402

CROP, SCALE = 4, 4


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def run_part(configs, a, extra):
    """Warm up, alternate, report. configs: [(mode, fn)]; extra(mode) -> dict of further fields."""
    times = {m: [] for m, _ in configs}
    for m, fn in configs:
        for _ in range(a.warmup):
            fn()
    for _ in range(a.rounds):
        for m, fn in configs:
            times[m].append(timed(fn, a.steps))
    out = []
    for m, fn in configs:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        t = times[m]
        r = {"tool": "pair_metrics_bench", "mode": m, "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup,
             "median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
             "spread_ms": round(max(t) - min(t), 3),
             "peak_extra_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
             "device": torch.cuda.get_device_name(0)}
        r.update(extra(m))
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def make_samples(B, H, W, M):
    g = torch.Generator(device="cuda").manual_seed(1)
    gt = torch.rand(B, 3, H, W, device="cuda", generator=g)
    return gt, [(gt + 0.05 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp(0, 1) for _ in range(M)]


def part_pairs(a):
    out = []
    pm = metrics.PairMetrics()
    for shape in a.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        gt, samples = make_samples(B, H, W, a.samples)
        rows = torch.empty(a.samples, B, 8, dtype=torch.float64, device="cuda")
        res = {}

        def psnr_ssim():
            for s in samples:
                res["one_shot"] = metrics.psnr_ssim(gt, s, CROP, SCALE)

        def pair():
            ref = pm.embed(gt, CROP, SCALE)
            for i, s in enumerate(samples):
                pm.compare(ref, s, out=rows[i])

        def sample_set():
            acc = pm.sample_set(gt, CROP, SCALE, capacity=a.samples)
            for s in samples:
                acc.add(s)
            res["mean"] = acc.result()["mean"].cpu()

        def compares_ms():
            ref = pm.embed(gt, CROP, SCALE)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i, s in enumerate(samples):
                pm.compare(ref, s, out=rows[i])
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        part = run_part([("psnr_ssim", psnr_ssim), ("pair", pair), ("sample_set", sample_set)], a, lambda m: {
            "part": "pairs", "shape": [B, 3, H, W], "samples": a.samples, "crop_border": CROP, "scale": SCALE})
        cmp_ms = [compares_ms() for _ in range(a.rounds)]
        same = all(n[k] == o[k] or (math.isnan(n[k]) and math.isnan(o[k]))
                   for n, o in zip(metrics.rows_to_dicts(rows[-1]), res["one_shot"]) for k in metrics.KEYS)
        assert same, "psnr_ssim and PairMetrics.compare are one computation and must agree exactly"
        part[1].update({"compares_ms": round(statistics.median(cmp_ms), 3), "compares_min_ms": round(min(cmp_ms), 3),
                        "compares_max_ms": round(max(cmp_ms), 3), "equals_psnr_ssim": same,
                        "ratio_psnr_ssim_over_pair": round(part[0]["median_ms"] / part[1]["median_ms"], 2)})
        print(json.dumps(part[1]), flush=True)
        out += part
        del gt, samples, rows
        torch.cuda.empty_cache()
    return out


def part_sweep(a):
    cfg = preset(a.preset)
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 1234), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(3)
    lq = torch.rand(1, 3, a.lr_size, a.lr_size, generator=g)
    gt = torch.rand(1, 3, a.lr_size * cfg.scale, a.lr_size * cfg.scale, generator=g)
    heats = [i / max(1, a.heats - 1) for i in range(a.heats)]
    batch = {"LQ": lq.cuda(), "GT": gt.cuda()}
    mb = max(16, a.heats)
    configs = [("evaluate_sweep", lambda: evaluate_sweep(net, batch, heats, a.n_sample, cfg.scale, seed=7, max_batch=mb))]
    return run_part(configs, a, lambda m: {"part": "sweep", "preset": a.preset, "lr": [1, 3, a.lr_size, a.lr_size],
                                           "heats": a.heats, "n_sample": a.n_sample, "with_gt": True})


def kernel_stats(path):
    """{kernel: total ms} of the pair_* kernels in a profiler's CSV: kernel statistics (Name, TotalDurationNs) or kernel trace
    (Kernel_Name, Start_Timestamp, End_Timestamp)."""
    tot = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("Kernel_Name") or ""
            if "pair_" not in name:
                continue
            ns = float(row["TotalDurationNs"]) if "TotalDurationNs" in row else float(row["End_Timestamp"]) - float(row["Start_Timestamp"])
            short = name.split("(")[0].replace("void ", "").split("::")[-1]
            for src in ("LowSrc", "FullSrc"):
                if src in name:
                    short = "pair_tile_kernel<%s>" % src
            tot[short] = tot.get(short, 0.0) + ns / 1e6
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="pairs,sweep")
    ap.add_argument("--shapes", default="16x640x640,16x160x160,1x1356x2040")
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--lr-size", type=int, default=160)
    ap.add_argument("--heats", type=int, default=11)
    ap.add_argument("--n-sample", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--trace-run", default="")
    ap.add_argument("--kernel-stats", default="")
    ap.add_argument("--out", default=os.path.join("profiles", "pair_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pair_metrics_bench.py needs a GPU (no CPU timing is meaningful here)")
    if a.trace_run:
        B, H, W = (int(v) for v in a.trace_run.split("x"))
        gt, samples = make_samples(B, H, W, a.samples)
        pm = metrics.PairMetrics()
        ref = pm.embed(gt, CROP, SCALE)
        rows = torch.empty(a.samples, B, 8, dtype=torch.float64, device="cuda")
        for i, s in enumerate(samples):
            pm.compare(ref, s, out=rows[i])
        torch.cuda.synchronize()
        return
    out = []
    with torch.no_grad():
        for part in a.parts.split(","):
            out += {"pairs": part_pairs, "sweep": part_sweep}[part](a)
            torch.cuda.empty_cache()
    if a.kernel_stats:
        k = kernel_stats(a.kernel_stats)
        out.append({"tool": "pair_metrics_bench", "part": "kernel_trace", "samples": a.samples,
                    "kernels_ms": {n: round(v, 3) for n, v in sorted(k.items())},
                    "compare_kernels_ms": round(sum(v for n, v in k.items() if "quant" not in n and "embed" not in n), 3)})
        print(json.dumps(out[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
