#!/usr/bin/env python
"""Time one training batch made on the device (hcflow_amd.data.prepare_batch) beside the same pipeline on the CPU.

    python tools/batch_prep_bench.py [--images 32] [--size 1356x2040] [--batch 16] [--gt-size 160] [--scale 4]
                                     [--rounds 7] [--steps 1000] [--warmup 20] [--threads 16]
                                     [--out profiles/r14_batch_prep_bench.json]

Bank: `images` seeded synthetic uint8 images of `size` (a DIV2K-sized image by default), decoded once into device memory.
Configurations, ALTERNATING inside each round so that drift of the clocks or of other tenants hits all of them alike:
  native: prepare_batch(bank, crops, gt_size, scale, out=...) -- one launch of the batch kernel; device events around `steps` calls
          on a fresh crop table each (the tables are drawn before the window: draw_crops is host work that overlaps the GPU);
  whole:  whole_image(bank, i, scale, out=...) -- the validation pair of one full image, same kernel, events around `steps` calls;
  cpu:    tests/data_oracle.py's torch_pipeline in fp32 on `threads` CPU threads -- per sample the reference's order of work
          (whole-image resize, then crop), host clock around ONE batch per round.
Per configuration one JSON line: median, min, max of the per-round ms per call ("spread_ms" = max - min). The native batch is
also compared with the CPU batch of the same crops (max |difference| of LQ, GT bit-equal). A difference between configurations
means something only beyond both spreads. All lines go to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hcflow_amd import data as D  # noqa: E402
from tests import data_oracle as O  # noqa: E402


def events_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--size", default="1356x2040")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--gt-size", type=int, default=160)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_batch_prep_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_prep_bench needs an MI355X: there is no CPU stand-in for the timed path")
    torch.set_num_threads(args.threads)
    H, W = (int(v) for v in args.size.split("x"))
    s, n = args.scale, args.gt_size // args.scale
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, size=(H, W, 3), dtype=np.uint8) for _ in range(args.images)]
    bank = D.ImageBank(imgs, "cuda:0")
    g = torch.Generator().manual_seed(0)
    tables = [D.draw_crops(bank, torch.randperm(len(bank), generator=g)[:args.batch], args.gt_size, s, generator=g)
              for _ in range(args.steps)]
    out = {"GT": torch.empty(args.batch, 3, args.gt_size, args.gt_size, device="cuda:0"),
           "LQ": torch.empty(args.batch, 3, n, n, device="cuda:0")}
    whole_ok = H % s == 0 and W % s == 0
    wout = {"GT": torch.empty(1, 3, H, W, device="cuda:0"), "LQ": torch.empty(1, 3, H // s, W // s, device="cuda:0")} if whole_ok else None
    cpu_imgs = [torch.from_numpy(im) for im in imgs]

    def native(i):
        D.prepare_batch(bank, tables[i % len(tables)], args.gt_size, s, out=out)

    def whole(i):
        D.whole_image(bank, i % len(bank), s, out=wout)

    def cpu_once(i):
        t0 = time.perf_counter()
        r = O.torch_pipeline(cpu_imgs, tables[i % len(tables)], n, s)
        return (time.perf_counter() - t0) * 1e3, r

    # agreement of the two pipelines on the same crops
    native(0)
    _, ref = cpu_once(0)
    gt_equal = bool(torch.equal(out["GT"].cpu(), ref["GT"]))
    lq_diff = float((out["LQ"].cpu() - ref["LQ"]).abs().max())
    for i in range(args.warmup):
        native(i)
        if whole_ok:
            whole(i)
    torch.cuda.synchronize()
    t = {"native": [], "whole": [], "cpu": []}
    for r in range(args.rounds):
        t["native"].append(events_ms(native, args.steps))
        if whole_ok:
            t["whole"].append(events_ms(whole, max(1, args.steps // 10)))
        t["cpu"].append(cpu_once(r)[0])
    lines = []
    common = {"images": args.images, "size": [H, W], "scale": s, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    for mode, v in t.items():
        if not v:
            continue
        rec = dict(common, mode=mode, median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v))
        if mode == "native":
            rec.update(batch=args.batch, gt_size=args.gt_size, calls_per_round=args.steps, bank_bytes=bank.nbytes,
                       gt_bit_equal_to_cpu=gt_equal, lq_max_abs_diff_to_cpu=lq_diff)
        elif mode == "whole":
            rec.update(calls_per_round=max(1, args.steps // 10))
        else:
            rec.update(batch=args.batch, gt_size=args.gt_size, calls_per_round=1, threads=args.threads, clock="host perf_counter")
        lines.append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
