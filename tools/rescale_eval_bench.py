#!/usr/bin/env python
"""Time the rescaling test step (loader.evaluate_batch on an HCFlowNet_Rescaling) against the same numbers computed the
reference's way from the pieces the project had before it, and the two image kernels alone, on one GPU.

    python tools/rescale_eval_bench.py [--parts eval,kernels] [--preset Rescaling_DF2K_4X] [--batch 8] [--size 640]
                                       [--heats 0.0,1.0] [--n-sample 1] [--rounds 7] [--steps 1] [--warmup 2]
                                       [--kernel-shapes 8x160x160,8x640x640,32x640x640] [--launches 50]
                                       [--out profiles/rescale_eval_bench.json]

(a) eval: one batch of `batch` HR images of `size` x `size` with a bicubic-sized LQ, seeded random weights, two configurations
  ALTERNATING inside each round:
  evaluate_batch:  loader.evaluate_batch(net, {"GT", "LQ"}, heats, n_sample, scale=4, seed=...): one forward pass over the batch,
                   metrics.quantize, every sample drawn from the one quantised LR^ (cache_cond hits), PairMetrics rows on the
                   device, one readback per heat;
  reference_way:   what HCFLowRescalingModel.test() under test_HCFlow.py does, ONE IMAGE AT A TIME, from public pieces that
                   predate evaluate_batch's rescaling branch: net(hr=gt[b:b+1]), the torch expression of Quantization,
                   fake_z1.mean().item(), net(lr=lr_q, eps_std=heat, reverse=True) per heat and sample, and one
                   metrics.psnr_ssim one-shot per compared pair (LQ vs LR^, GT vs every sample).
  The two produce the same dict layout; the tool checks the deterministic entries: "nll" and "lr" must agree exactly, the heat-0
  entries (inverse passes at B = `batch` and at B = 1, whose launch plans may round differently) to 1e-4 relative, the largest
  gap being recorded; if they do not, the output says which and the tool exits non-zero after writing it. Host clock around `steps`
  iterations ending in a device synchronise; median, min, max over `rounds`.
(b) kernels: metrics.quantize (q + image, q only) and metrics.from_image alone per shape BxHxW, `launches` back-to-back calls into
  preallocated outputs between two device events (launch gaps included: at the LR size of the eval batch, 8x160x160, a call is a
  launch, not a stream of bytes). "bytes" is what the algorithm moves (fp32 planes read / written, 3 bytes per pixel of image),
  "fraction_of_roof" is bytes / time over the 6.3 TB/s element-wise roof the README quotes for SampleStats; a tensor that fits
  the 256 MB last-level cache is re-read from it between launches, which the "fits_llc" field says.
One JSON line per configuration; one is faster than the other only if the medians differ by more than both spreads."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import HCFlowNet_Rescaling, make_params, metrics, preset  # noqa: E402
from hcflow_amd.loader import evaluate_batch  # noqa: E402

CROP, SCALE = 4, 4
ROOF_TBS = 6.3


def timed(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4)}


def reference_way(net, batch, heats, n_sample, seed):
    """The per-image loop of test_HCFlow.py:85-182 around HCFLowRescalingModel.test() (HCFlow_Rescaling_model.py:306-324)."""
    res = []
    for b in range(batch["GT"].shape[0]):
        gt, lq = batch["GT"][b:b + 1], batch["LQ"][b:b + 1]
        lr_hat, z1, _ = net(hr=gt, reverse=False)
        lr_q = (torch.clamp(lr_hat, 0, 1) * 255.).round() / 255.                # Basic.Quant.forward
        ent = {"nll": z1.mean().item()}
        m = metrics.psnr_ssim(lq, lr_q, 0, 0)[0]
        ent["lr"] = {k: m[k] for k in ("psnr", "ssim", "psnr_y", "ssim_y")}
        for hi, heat in enumerate(heats):
            samples = [net(lr=lr_q, z=None, u=None, eps_std=heat, reverse=True, training=False, seed=seed + 1000 * hi + s)
                       for s in range(n_sample)]
            rows = [metrics.psnr_ssim(gt, sr, CROP, SCALE)[0] for sr in samples]
            e = {k: sum(r[k] for r in rows) / n_sample for k in metrics.KEYS}
            e["diversity"] = metrics.diversity(samples) if n_sample > 1 else 0.0
            ent[float(heat)] = e
        res.append(ent)
    return res


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def part_eval(a):
    cfg = preset(a.preset)
    net = HCFlowNet_Rescaling(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 1234), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(3)
    batch = {"GT": torch.rand(a.batch, 3, a.size, a.size, generator=g).cuda(),
             "LQ": torch.rand(a.batch, 3, a.size // cfg.scale, a.size // cfg.scale, generator=g).cuda()}
    heats = [float(v) for v in a.heats.split(",")]
    res = {}

    def batched():
        res["evaluate_batch"] = evaluate_batch(net, batch, heats, a.n_sample, cfg.scale, seed=7)

    def one_by_one():
        res["reference_way"] = reference_way(net, batch, heats, a.n_sample, 7)

    configs = [("evaluate_batch", batched), ("reference_way", one_by_one)]
    times = {m: [] for m, _ in configs}
    for _, fn in configs:
        for _ in range(a.warmup):
            fn()
    for _ in range(a.rounds):
        for m, fn in configs:
            times[m].append(timed(fn, a.steps))
    # one computation: "nll" and "lr" (forward pass, quantisation, metrics) agree exactly, image by image; the heat-0 entries come
    # from inverse passes of different batch sizes, whose launch plans may round differently: their largest relative gap is
    # recorded and held to the 1e-4 of the engine's parity gates
    differ, gap = [], 0.0
    for b, (x, y) in enumerate(zip(res["evaluate_batch"], res["reference_way"])):
        if not same(x["nll"], y["nll"]):
            differ.append(("nll", b, x["nll"], y["nll"]))
        differ += [("lr." + k, b, x["lr"][k], y["lr"][k]) for k in x["lr"] if not same(x["lr"][k], y["lr"][k])]
        if 0.0 in x:
            for k in metrics.KEYS:
                if not same(x[0.0][k], y[0.0][k]):
                    gap = max(gap, abs(x[0.0][k] - y[0.0][k]) / max(abs(y[0.0][k]), 1e-300))
    agree = not differ and gap <= 1e-4
    out = []
    for m, _ in configs:
        r = {"tool": "rescale_eval_bench", "part": "eval", "mode": m, "preset": a.preset, "gt": [a.batch, 3, a.size, a.size],
             "heats": heats, "n_sample": a.n_sample, "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup,
             "device": torch.cuda.get_device_name(0), "deterministic_entries_agree": agree, "nll_lr_entries_that_differ": differ[:8],
             "heat0_max_relative_gap": gap}
        r.update(summary(times[m]))
        r["ms_per_image"] = round(r["median_ms"] / a.batch, 4)
        out.append(r)
    out[0]["ratio_reference_way_over_evaluate_batch"] = round(out[1]["median_ms"] / out[0]["median_ms"], 3)
    for r in out:
        print(json.dumps(r), flush=True)
    return out


def part_kernels(a):
    out = []
    for shape in a.kernel_shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand(B, 3, H, W, device="cuda", generator=g) * 1.2 - 0.1
        q = torch.empty_like(x)
        img = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
        back = torch.empty_like(x)
        pix = B * H * W
        configs = [("quantize q+image", lambda: metrics.quantize(x, out=q, image_out=img), 27 * pix),
                   ("quantize q", lambda: metrics.quantize(x, out=q), 24 * pix),
                   ("from_image", lambda: metrics.from_image(img, out=back), 15 * pix)]
        times = {m: [] for m, _, _ in configs}
        for _, fn, _ in configs:
            for _ in range(a.warmup + 3):
                fn()
        for _ in range(a.rounds):
            for m, fn, _ in configs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[m].append(e0.elapsed_time(e1) / a.launches)
        assert torch.equal(metrics.quantize(metrics.from_image(img), image=True)[1], img)       # stored images are fixed points
        for m, _, nbytes in configs:
            r = {"tool": "rescale_eval_bench", "part": "kernels", "mode": m, "shape": [B, 3, H, W], "launches": a.launches,
                 "rounds": a.rounds, "bytes": nbytes, "fits_llc": nbytes <= 256 * 2 ** 20, "device": torch.cuda.get_device_name(0)}
            r.update(summary(times[m]))
            r["tb_per_s"] = round(nbytes / (r["median_ms"] * 1e-3) / 1e12, 4)
            r["fraction_of_roof"] = round(r["tb_per_s"] / ROOF_TBS, 4)
            r["roof_tb_per_s"] = ROOF_TBS
            print(json.dumps(r), flush=True)
            out.append(r)
        del x, q, img, back
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="eval,kernels")
    ap.add_argument("--preset", default="Rescaling_DF2K_4X")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--heats", default="0.0,1.0")
    ap.add_argument("--n-sample", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-shapes", default="8x160x160,8x640x640,32x640x640")
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "rescale_eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rescale_eval_bench.py needs a GPU (no CPU timing is meaningful here)")
    out = []
    with torch.no_grad():
        for part in a.parts.split(","):
            out += {"eval": part_eval, "kernels": part_kernels}[part](a)
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    if any(r.get("deterministic_entries_agree") is False for r in out):
        sys.exit("rescale_eval_bench.py: evaluate_batch and the per-image loop disagree on a deterministic entry (see the output)")


if __name__ == "__main__":
    main()
