#!/usr/bin/env python
"""Time the two pieces of judging a model by its sample SET on one GPU: a heat sweep whose heats share calls, and the streaming
per-pixel statistics.

    python tools/sample_set_bench.py [--parts sweep,stats] [--preset SR_DF2K_4X] [--lr-size 160] [--heats 11] [--n-sample 5]
                                     [--stats-shape 16x640x640] [--samples 10] [--rounds 7] [--steps 1] [--warmup 2]
                                     [--out profiles/sample_set_bench.json]

(a) sweep: ONE LR image, `heats` temperatures 0 .. 1, `n_sample` samples each, seeded random weights (f16x3, the module default).
  calls_scalar:   the heats x n_sample B = 1 calls as loader.evaluate_batch issues them (scalar eps_std, cache_cond=True);
  calls_sweep:    the n_sample calls of `heats` rows as loader.evaluate_sweep issues them (eps_std vector, cache_cond=True);
  evaluate_batch / evaluate_sweep: the two functions themselves on a batch without GT (sampling + diversity: held samples and
                  torch's std against metrics.SampleStats).
(b) stats: M samples of --stats-shape, generated once and held by the tool for both modes.
  stats:  metrics.SampleStats: M add + result() (mean, std, diversity);
  stock:  st = torch.stack(samples); torch.std_mean(st, 0); (255 std).mean per image -- what metrics.diversity computes, kept
          per pixel.
  "peak_extra_mb" is torch.cuda.max_memory_allocated over one iteration minus what was allocated before it (the held samples,
  "samples_held_mb", are not in it: a streaming caller of SampleStats never holds them, stock must). "add_ms" times the M adds
  alone; "add_gbs" = their algorithmic bytes (4 B sample in, 16 B state in and out per element, the first add writes only) over
  that time: an end-to-end rate from device events, launch gaps included, not a kernel time.
Every configuration is warmed up, then timed (host clock around `steps` iterations ending in a device synchronise) `rounds`
times, the configurations of a part ALTERNATING inside each round so that clock drift and other tenants hit them alike. Per
configuration one JSON line: median, min, max of the per-round ms per iteration. One is faster than the other only if the medians
differ by more than both spreads. All lines go to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import HCFlowNet_SR, make_params, metrics, preset  # noqa: E402
from hcflow_amd.loader import evaluate_batch, evaluate_sweep  # noqa: E402


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
        r = {"tool": "sample_set_bench", "mode": m, "rounds": a.rounds, "steps": a.steps, "warmup": a.warmup,
             "median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
             "spread_ms": round(max(t) - min(t), 3),
             "peak_extra_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1),
             "device": torch.cuda.get_device_name(0)}
        r.update(extra(m))
        print(json.dumps(r), flush=True)
        out.append(r)
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
    lq = torch.rand(1, 3, a.lr_size, a.lr_size, generator=g).cuda()
    heats = [i / max(1, a.heats - 1) for i in range(a.heats)]
    rows = lq.expand(a.heats, -1, -1, -1).contiguous()
    taus = torch.tensor(heats, dtype=torch.float32)
    batch = {"LQ": lq}

    def calls_scalar():
        for hi, heat in enumerate(heats):
            for s in range(a.n_sample):
                net(lr=lq, z=None, u=None, eps_std=heat, reverse=True, training=False, cache_cond=True, seed=7 + 1000 * hi + s)

    def calls_sweep():
        for s in range(a.n_sample):
            net(lr=rows, z=None, u=None, eps_std=taus, reverse=True, training=False, cache_cond=True, seed=7 + s, sample_offset=0)

    configs = [("calls_scalar", calls_scalar), ("calls_sweep", calls_sweep),
               ("evaluate_batch", lambda: evaluate_batch(net, batch, heats, a.n_sample, cfg.scale, seed=7)),
               ("evaluate_sweep", lambda: evaluate_sweep(net, batch, heats, a.n_sample, cfg.scale, seed=7, max_batch=max(16, a.heats)))]
    with torch.no_grad():
        # the definition of a row, at the timed size: row hi of the sweep call against the scalar call with its sample index
        full = net(lr=rows, eps_std=taus, reverse=True, seed=7, sample_offset=0)
        hi = a.heats - 1
        one = net(lr=lq, eps_std=heats[hi], reverse=True, seed=7, sample_offset=hi)
        dev = float((full[hi:hi + 1] - one).abs().max())
        del full, one
        n_img = a.heats * a.n_sample
        return run_part(configs, a, lambda m: {
            "part": "sweep", "preset": a.preset, "lr": [1, 3, a.lr_size, a.lr_size], "heats": a.heats, "n_sample": a.n_sample,
            "inverse_calls": n_img if m in ("calls_scalar", "evaluate_batch") else a.n_sample,
            "rows_per_call": 1 if m in ("calls_scalar", "evaluate_batch") else a.heats,
            "last_row_max_abs_dev_from_scalar_call": dev})


def part_stats(a):
    B, H, W = (int(v) for v in a.stats_shape.split("x"))
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.rand(B, 3, H, W, device="cuda", generator=g)
    samples = [(x + 0.05 * torch.randn(B, 3, H, W, device="cuda", generator=g)).clamp(0, 1) for _ in range(a.samples)]
    del x
    st = metrics.SampleStats(B, H, W, "cuda")
    res = {}

    def stats():
        st.reset()
        for s in samples:
            st.add(s)
        res["stats"] = st.result()

    def stock():
        stack = torch.stack(samples)
        sd, mean = torch.std_mean(stack, 0)
        res["stock"] = {"mean": mean, "std": sd, "diversity": (255 * sd).mean(dim=(1, 2, 3))}

    def adds_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.reset()
        e0.record()
        for s in samples:
            st.add(s)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    with torch.no_grad():
        out = run_part([("stats", stats), ("stock", stock)], a, lambda m: {
            "part": "stats", "shape": [B, 3, H, W], "samples": a.samples,
            "samples_held_mb": round(a.samples * B * 3 * H * W * 4 / 2 ** 20, 1),
            "state_mb": round(st._bytes / 2 ** 20, 1)})
        add = [adds_ms() for _ in range(a.rounds)]
        n = B * 3 * H * W
        by = n * (4 + 16) + (a.samples - 1) * n * (4 + 16 + 16)
        out[0].update({"add_ms": round(statistics.median(add), 3), "add_min_ms": round(min(add), 3), "add_max_ms": round(max(add), 3),
                       "add_gbs": round(by / (statistics.median(add) * 1e-3) / 1e9, 1)})
        for k in ("mean", "std"):
            out[0]["max_abs_dev_from_stock_" + k] = float((res["stats"][k] - res["stock"][k]).abs().max())
        out[0]["max_abs_dev_from_stock_diversity"] = float((res["stats"]["diversity"] - res["stock"]["diversity"].double()).abs().max())
        print(json.dumps(out[0]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="sweep,stats")
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--lr-size", type=int, default=160)
    ap.add_argument("--heats", type=int, default=11)
    ap.add_argument("--n-sample", type=int, default=5)
    ap.add_argument("--stats-shape", default="16x640x640")
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "sample_set_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sample_set_bench.py needs a GPU (no CPU timing is meaningful here)")
    out = []
    for part in a.parts.split(","):
        out += {"sweep": part_sweep, "stats": part_stats}[part](a)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
