#!/usr/bin/env python
"""Time paired training batches made on the device (hcflow_amd.data.prepare_paired_batch / whole_pair) beside the reference's
per-sample pipeline on the CPU.

    python tools/paired_batch_bench.py [--images 32] [--size 1356x2040] [--batch 16] [--gt-size 160] [--scale 4]
                                       [--rounds 7] [--steps 1000] [--warmup 20] [--threads 16]
                                       [--out profiles/r16_paired_batch_bench.json]

Banks of seeded synthetic uint8 pairs, packed once into device memory (the LQ images are random bytes of their own):
  div2k   `images` pairs of `size` HR / size / scale LQ (a DIV2K-sized pair by default);
  celeba  64 pairs of 160 x 160 HR / 20 x 20 LQ (the CelebA x8 shape of the LRHR_PKL configurations).
Configurations, ALTERNATING inside each round so that drift of the clocks or of other tenants hits all of them alike:
  paired_batch   prepare_paired_batch(div2k, crops, gt_size, out=...), rule="pkl" draws -- one launch; device events around
                 `steps` calls on a fresh crop table each (drawn before the window: the draws are host work);
  paired_celeba  the same on celeba with gt_size 160: every sample is its whole pair, augmented;
  paired_whole   whole_pair(div2k, i, out=...) -- the validation pair of one full image, events around steps / 10 calls;
  gt_mode_batch  prepare_batch(ImageBank of the same HR images, ...) -- the GT-mode kernel (bicubic LQ) at the same shapes;
  cpu_batch, cpu_celeba   the reference's LRHR_PKL per-sample work restated below (cpu_pkl_batch: crop, flip, rot90, / 255.0 in
                 float64, torch.Tensor, stack) and the host-to-device copy of the batch, host clock around ONE batch per round,
                 ending in a device synchronise.
Per configuration one JSON line: median, min, max of the per-round ms per call ("spread_ms" = max - min), and for the native
ones the bytes a call has to move (uint8 read + float32 written) over the median. The native batches are compared with the CPU
batches of the same crops: they must be identical tensors. A difference between configurations means something only beyond both
spreads. All lines go to --out.
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

FK_OF_FLAGS = {v: k for k, v in D.PKL_FLAGS.items()}


def cpu_pkl_batch(hr_chw, lr_chw, crops, n, s, device):
    """One batch the way the reference's LRHR_PKL dataset and its DataLoader make it, the draws given: per sample random_crop's
    slices, random_flip's np.flip(..., 2).copy(), random_rotation's np.rot90(..., axes=(1, 2)).copy(), / 255.0, torch.Tensor;
    then the default collate (stack) and the copy feed_data does."""
    gts, lqs = [], []
    for i, top, left, hf, vf, rot in (tuple(int(v) for v in r) for r in crops):
        f, k = FK_OF_FLAGS[(hf, vf, rot)]
        hr, lr = hr_chw[i], lr_chw[i]
        lr = lr[:, top:top + n, left:left + n]
        hr = hr[:, top * s:top * s + n * s, left * s:left * s + n * s]
        if f:
            hr, lr = np.flip(hr, 2).copy(), np.flip(lr, 2).copy()
        hr, lr = np.rot90(hr, k, axes=(1, 2)).copy(), np.rot90(lr, k, axes=(1, 2)).copy()
        hr, lr = hr / 255.0, lr / 255.0
        gts.append(torch.Tensor(hr))
        lqs.append(torch.Tensor(lr))
    out = {"GT": torch.stack(gts).to(device), "LQ": torch.stack(lqs).to(device)}
    torch.cuda.synchronize()
    return out


def events_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(steps):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def pairs(rs, count, lq_h, lq_w, s):
    return ([rs.randint(0, 256, size=(lq_h * s, lq_w * s, 3), dtype=np.uint8) for _ in range(count)],
            [rs.randint(0, 256, size=(lq_h, lq_w, 3), dtype=np.uint8) for _ in range(count)])


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_paired_batch_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paired_batch_bench needs an MI355X: there is no CPU stand-in for the timed path")
    torch.set_num_threads(args.threads)
    dev = "cuda:0"
    H, W = (int(v) for v in args.size.split("x"))
    s, n, B = args.scale, args.gt_size // args.scale, args.batch
    if H % s or W % s:
        raise SystemExit("--size must be a multiple of --scale")
    rs = np.random.RandomState(0)
    g = torch.Generator().manual_seed(0)

    def tables(bank, gt_size):
        return [D.draw_paired_crops(bank, torch.randperm(len(bank), generator=g)[:B], gt_size, "pkl", generator=g)
                for _ in range(args.steps)]

    def outputs(gh, gw, sc, b=B):
        return {"GT": torch.empty(b, 3, gh, gw, device=dev), "LQ": torch.empty(b, 3, gh // sc, gw // sc, device=dev)}

    gts, lqs = pairs(rs, args.images, H // s, W // s, s)
    div2k = D.PairedBank(gts, lqs, dev, order="rgb")
    gt_only = D.ImageBank(gts, dev, order="rgb")
    t_div, out_div, out_gtm, out_whole = tables(div2k, args.gt_size), outputs(args.gt_size, args.gt_size, s), \
        outputs(args.gt_size, args.gt_size, s), outputs(H, W, s, 1)
    t_gtm = [D.draw_crops(gt_only, t[:, 0], args.gt_size, s, generator=g) for t in t_div[:64]]
    cgts, clqs = pairs(rs, 64, 20, 20, 8)
    celeba = D.PairedBank(cgts, clqs, dev, order="rgb")
    t_cel, out_cel = tables(celeba, 160), outputs(160, 160, 8)
    chw = lambda imgs: [np.transpose(im, [2, 0, 1]) for im in imgs]      # noqa: E731  (load_pkls keeps transposed views)
    cpu_div, cpu_cel = (chw(gts), chw(lqs)), (chw(cgts), chw(clqs))

    native = {
        "paired_batch": (lambda i: D.prepare_paired_batch(div2k, t_div[i % len(t_div)], args.gt_size, out=out_div), args.steps),
        "paired_celeba": (lambda i: D.prepare_paired_batch(celeba, t_cel[i % len(t_cel)], 160, out=out_cel), args.steps),
        "paired_whole": (lambda i: D.whole_pair(div2k, i % len(div2k), out=out_whole), max(1, args.steps // 10)),
        "gt_mode_batch": (lambda i: D.prepare_batch(gt_only, t_gtm[i % len(t_gtm)], args.gt_size, s, out=out_gtm), args.steps),
    }
    cpu = {
        "cpu_batch": lambda i: cpu_pkl_batch(cpu_div[0], cpu_div[1], t_div[i % len(t_div)], n, s, dev),
        "cpu_celeba": lambda i: cpu_pkl_batch(cpu_cel[0], cpu_cel[1], t_cel[i % len(t_cel)], 20, 8, dev),
    }

    # the two pipelines make identical tensors from the same crops
    same = {}
    for name, ref_name, out in (("paired_batch", "cpu_batch", out_div), ("paired_celeba", "cpu_celeba", out_cel)):
        native[name][0](3)
        ref = cpu[ref_name](3)
        same[name] = bool(torch.equal(out["GT"], ref["GT"]) and torch.equal(out["LQ"], ref["LQ"]))
        if not same[name]:
            raise SystemExit("%s differs from the CPU restatement" % name)
    native["paired_whole"][0](1)
    w_gt = torch.from_numpy(gts[1]).permute(2, 0, 1).float().div(255.).to(dev)      # a true division, on the host
    if not torch.equal(out_whole["GT"][0], w_gt):
        raise SystemExit("paired_whole differs from the stored image")

    for i in range(args.warmup):
        for fn, _ in native.values():
            fn(i)
    for fn in cpu.values():
        fn(0)
    torch.cuda.synchronize()
    t = {k: [] for k in list(native) + list(cpu)}
    for r in range(args.rounds):
        for name, (fn, steps) in native.items():
            t[name].append(events_ms(fn, steps))
        for name, fn in cpu.items():
            t0 = time.perf_counter()
            fn(r)
            t[name].append((time.perf_counter() - t0) * 1e3)

    px = {"paired_batch": B * (args.gt_size ** 2 + n * n), "paired_celeba": B * (160 * 160 + 20 * 20),
          "paired_whole": H * W + (H // s) * (W // s)}
    common = {"rounds": args.rounds, "device": torch.cuda.get_device_name(0)}
    lines = []
    for mode, v in t.items():
        rec = dict(common, mode=mode, median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v), spread_ms=max(v) - min(v))
        if mode in native:
            rec.update(calls_per_round=native[mode][1], clock="device events")
            if mode in px:
                rec.update(bytes_per_call=px[mode] * 3 * 5, gbytes_per_s=px[mode] * 3 * 5 / (rec["median_ms"] * 1e-3) / 1e9)
            if mode in same:
                rec.update(identical_to_cpu=same[mode])
        else:
            rec.update(calls_per_round=1, threads=args.threads, clock="host perf_counter, ends in a device synchronise")
        if mode in ("paired_batch", "gt_mode_batch", "cpu_batch"):
            rec.update(batch=B, gt_size=args.gt_size, scale=s, images=args.images, size=[H, W])
        elif mode in ("paired_celeba", "cpu_celeba"):
            rec.update(batch=B, gt_size=160, scale=8, images=64, size=[160, 160])
        else:
            rec.update(batch=1, scale=s, size=[H, W])
        lines.append(rec)
        print(json.dumps(rec))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
