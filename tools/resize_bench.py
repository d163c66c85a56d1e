#!/usr/bin/env python
"""Time hcflow_amd.resize.imresize on one GPU beside torch's antialiased bicubic, and report each kernel's achieved bandwidth.

    python tools/resize_bench.py [--rounds 7] [--steps 200] [--warmup 3] [--out profiles/resize_bench.json]
    rocprofv3 --kernel-trace -d DIR -- python tools/resize_bench.py --trace-case N [--steps 20]      # a run of its own, per case
    python tools/resize_bench.py --kernel-db DIR0,DIR1,DIR2 --out profiles/resize_bench.json         # folds the traces in

Cases: 16 x 3 x 640^2 at 1/4, 16 x 3 x 160^2 x4, 1 x 3 x 1356 x 2040 at 1/4. Configurations per case, on the same input:
  hcf_fwd / hcf_fwd_bwd:      imresize(x, scale) under no_grad / imresize(x.requires_grad_(), scale).backward(g)
  torch_fwd / torch_fwd_bwd:  F.interpolate(x, scale_factor=scale, mode="bicubic", antialias=True, align_corners=False) likewise.
The torch form computes DIFFERENT values (another kernel and another border rule); the largest
difference on the case's input is recorded as "max_abs_diff_torch_vs_hcf" so that nobody takes the two for interchangeable.
Every configuration is warmed up, then timed with device events around `steps` iterations, `rounds` times, the configurations
ALTERNATING inside each round; per configuration median, min and max of the per-round ms per iteration. One configuration is
faster than another only if the medians differ by more than both spreads.

Traffic. The op is two kernels through a [B, C, Ho, W] intermediate t: forward resize_h_kernel reads x and writes t, then
resize_w_kernel reads t and writes y; the backward runs resize_w_kernel (gy -> u, the same size as t) and resize_h_kernel
(u -> gx). "algorithmic_bytes" of a kernel = 4 x (elements it reads once + elements it writes once); tables and tile halos are
not counted. --trace-case runs the four launches of one case `steps` times through the C entries (nothing else is launched), so
that a kernel trace holds them in the fixed order fwd_h, fwd_w, bwd_w, bwd_h; --kernel-db reads such traces (rocpd sqlite) and
adds per kernel the median time, bytes/s and the fraction of the 6.3 TB/s element-wise roof (HBM float4 copy) to the JSON.
"""
import argparse
import glob
import json
import os
import sqlite3
import statistics
import sys
from fractions import Fraction

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import _lib  # noqa: E402
from hcflow_amd.resize import imresize, out_size  # noqa: E402

CASES = [(16, 3, 640, 640, 4, 0), (16, 3, 160, 160, 4, 1), (1, 3, 1356, 2040, 4, 0)]
ROOF = 6.3e12
ORDER = ["fwd_h", "fwd_w", "bwd_w", "bwd_h"]


def kernel_bytes(B, C, H, W, s, up):
    """Algorithmic bytes of the four launches of a case."""
    Ho, Wo = out_size(H, s, up), out_size(W, s, up)
    x, t, y = B * C * H * W, B * C * Ho * W, B * C * Ho * Wo
    return {"fwd_h": 4 * (x + t), "fwd_w": 4 * (t + y), "bwd_w": 4 * (y + t), "bwd_h": 4 * (t + x)}


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def configs_of(x, g, s, up):
    sc = s if up else Fraction(1, s)
    fs = float(s) if up else 1.0 / s
    xr = x.clone().requires_grad_(True)

    def interp(v):
        return F.interpolate(v, scale_factor=fs, mode="bicubic", antialias=True, align_corners=False)

    def hcf_fwd():
        with torch.no_grad():
            return imresize(x, sc)

    def torch_fwd():
        with torch.no_grad():
            return interp(x)

    def hcf_fwd_bwd():
        xr.grad = None
        imresize(xr, sc).backward(g)
        return xr.grad

    def torch_fwd_bwd():
        xr.grad = None
        interp(xr).backward(g)
        return xr.grad
    return [("hcf_fwd", hcf_fwd), ("torch_fwd", torch_fwd), ("hcf_fwd_bwd", hcf_fwd_bwd), ("torch_fwd_bwd", torch_fwd_bwd)]


def make_inputs(case):
    B, C, H, W, s, up = case
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(B, C, H, W, device="cuda", generator=gen)
    g = torch.randn(B, C, out_size(H, s, up), out_size(W, s, up), device="cuda", generator=gen)
    return x, g


def run_timed(a):
    out = []
    for case in CASES:
        B, C, H, W, s, up = case
        x, g = make_inputs(case)
        cfgs = configs_of(x, g, s, up)
        res, times = {}, {m: [] for m, _ in cfgs}
        for m, fn in cfgs:
            for _ in range(a.warmup):
                res[m] = fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for m, fn in cfgs:
                times[m].append(timed(fn, a.steps))
        diff = float((res["hcf_fwd"] - res["torch_fwd"]).abs().max()) if res["hcf_fwd"].shape == res["torch_fwd"].shape else None
        kb = kernel_bytes(*case)
        for m, _ in cfgs:
            t = times[m]
            r = {"tool": "resize_bench", "mode": m, "shape": [B, C, H, W], "scale": ("x%d" if up else "1/%d") % s,
                 "out_shape": list(res["hcf_fwd"].shape), "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup,
                 "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                 "spread_ms": round(max(t) - min(t), 4), "max_abs_diff_torch_vs_hcf": diff,
                 "device": torch.cuda.get_device_name(0)}
            if m.startswith("hcf"):
                names = ORDER[:2] if m == "hcf_fwd" else ORDER
                r["algorithmic_bytes"] = {k: kb[k] for k in names}
                r["op_bytes_per_s"] = round(sum(kb[k] for k in names) / (statistics.median(t) * 1e-3), 1)
                r["op_fraction_of_6.3TBps"] = round(r["op_bytes_per_s"] / ROOF, 4)
            print(json.dumps(r), flush=True)
            out.append(r)
        del cfgs, res, x, g
        torch.cuda.empty_cache()
    return out


def run_trace_case(a):
    """The four launches of one case, `steps` times, through the C entries alone (after one warm-up round that uploads the tables)."""
    case = CASES[a.trace_case]
    B, C, H, W, s, up = case
    x, g = make_inputs(case)
    y, gx = torch.empty_like(g), torch.empty_like(x)
    need = int(_lib.load().hcf_resize_workspace(B, C, H, W, s, up))
    work = torch.empty(need, dtype=torch.uint8, device="cuda")
    for _ in range(a.steps + 1):
        _lib.launch("hcf_resize_bicubic", x.device, x, B, C, H, W, s, up, y, work, need)
        _lib.launch("hcf_resize_bicubic_backward", x.device, g, B, C, H, W, s, up, gx, work, need)
    torch.cuda.synchronize()
    print(json.dumps({"tool": "resize_bench", "trace_case": a.trace_case, "shape": [B, C, H, W], "launches": 4 * (a.steps + 1)}))


def fold_kernel_db(a, out):
    for i, d in enumerate(a.kernel_db.split(",")):
        dbs = sorted(glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True)) if os.path.isdir(d) else [d]
        if not dbs:
            sys.exit("no *_results.db under %s" % d)
        cur = sqlite3.connect(dbs[0]).cursor()
        rows = list(cur.execute("select name, end - start from kernels where name like '%resize_%' order by start"))
        if len(rows) < 8 or len(rows) % 4:
            sys.exit("%s: %d resize launches, not a --trace-case run" % (dbs[0], len(rows)))
        want = ["resize_h_kernel", "resize_w_kernel", "resize_w_kernel", "resize_h_kernel"]
        assert all(want[j % 4] in rows[j][0] for j in range(len(rows))), "launch order is not fwd_h, fwd_w, bwd_w, bwd_h"
        B, C, H, W, s, up = CASES[i]
        kb = kernel_bytes(*CASES[i])
        r = {"tool": "resize_bench", "mode": "kernels", "shape": [B, C, H, W], "scale": ("x%d" if up else "1/%d") % s,
             "source": "rocprofv3 --kernel-trace of --trace-case %d, first round dropped" % i, "kernels": {}}
        for j, k in enumerate(ORDER):
            us = [rows[q][1] / 1e3 for q in range(4 + j, len(rows), 4)]
            med = statistics.median(us)
            r["kernels"][k] = {"kernel": want[j], "calls": len(us), "median_us": round(med, 2), "min_us": round(min(us), 2),
                               "max_us": round(max(us), 2), "algorithmic_bytes": kb[k],
                               "bytes_per_s": round(kb[k] / (med * 1e-6), 1), "fraction_of_6.3TBps": round(kb[k] / (med * 1e-6) / ROOF, 4)}
        print(json.dumps(r), flush=True)
        out.append(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-case", type=int, default=None)
    ap.add_argument("--kernel-db", default=None)
    ap.add_argument("--out", default=os.path.join("profiles", "resize_bench.json"))
    a = ap.parse_args()
    if a.kernel_db:                                            # post-processing: no GPU needed
        out = [r for r in json.load(open(a.out)) if r.get("mode") != "kernels"] if os.path.exists(a.out) else []
        fold_kernel_db(a, out)
    else:
        if not torch.cuda.is_available():
            sys.exit("resize_bench.py needs a GPU (no CPU timing is meaningful here)")
        if a.trace_case is not None:
            return run_trace_case(a)
        out = run_timed(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
