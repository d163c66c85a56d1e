"""ms per backward pass of the taped inverse pass in its two forms, in the SAME run: the input-gradient-only backward
(hcf_train_backward_inverse_ex with dparams = NULL: dL/d lr and dL/d eps, no parameter-gradient work) beside the full
hcf_train_backward_inverse (every parameter gradient + dL/d lr) of the same taped pass, at config 5's shape: SR_DF2K_4X, seeded
weights, B = 16, LR 40 x 40 -> HR 160 x 160, both conv precisions.

Method: inputs resident in HBM; a backward pass consumes its tape, so every sample is one untimed hcf_train_inverse followed by ONE
backward between two HIP events on the launch stream; warm-up samples of both forms first, then `--rounds` rounds that ALTERNATE the
two forms (`--iters` samples each, a device synchronise after each), Python's cyclic GC off inside the timed region. Reported per
backward pass: the median over the rounds and the spread (min, max) -- a difference inside the full pass's own spread is not a
difference. The counters of hcf_train_backward_counts of the last pass of each form go with it. One JSON line (stdout, and appended
to --out).

    python tools/latent_grad_bench.py [--iters 3] [--rounds 5] [--warmup 2] [--B 16] [--lr 40] [--out profiles/r09_latent_grad_bench.json]
"""
import argparse
import ctypes as C
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import HCFlowNet_SR, _lib, eps_shapes, preset, make_params  # noqa: E402


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--lr", type=int, default=40)
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--precisions", default="f16x3,exact")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "latent_grad_bench needs an MI355X"
    dev = torch.device("cuda:0")
    cfg = preset(args.preset)
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 21), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    B, h = args.B, args.lr
    lr = torch.rand(B, 3, h, h, device=dev, generator=g)
    shapes = eps_shapes(cfg, B, h, h)
    eps = [torch.randn(s, device=dev, generator=g) * 0.8 for s in shapes]
    out = torch.empty(B, 3, h * cfg.scale, h * cfg.scale, device=dev)
    g_out = torch.randn(out.shape, device=dev, generator=g) / out.numel()
    g_lr = torch.empty_like(lr)
    g_eps = [torch.empty_like(e) for e in eps]
    total = sum(p.numel() for p in net._params())
    flat = torch.empty(total, device=dev)
    eps_arr = (C.c_void_p * len(eps))(*[e.data_ptr() for e in eps])
    geps_arr = (C.c_void_p * len(eps))(*[e.data_ptr() for e in g_eps])
    res = {"what": "input-gradient-only backward vs the full backward of the taped inverse pass", "preset": args.preset, "B": B,
           "lr": [h, h], "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup, "parameters": total}
    for prec in [p for p in args.precisions.split(",") if p]:
        net.set_precision(prec)
        eng, idx = net._engine_for(dev)
        lib, hd = eng.lib, eng.handle
        stream = C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
        _lib.check(lib.hcf_train_select_tape(hd, 1), hd, "hcf_train_select_tape")

        def sample(inputs_only):
            _lib.check(lib.hcf_train_inverse(hd, lr.data_ptr(), eps_arr, len(eps), 1.0, 0, out.data_ptr(), B, h, h,
                                             _lib.FLAG_NO_CLAMP, stream), hd, "hcf_train_inverse")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if inputs_only:
                rc = lib.hcf_train_backward_inverse_ex(hd, g_out.data_ptr(), None, 0, g_lr.data_ptr(), geps_arr, len(eps), stream)
            else:
                rc = lib.hcf_train_backward_inverse(hd, g_out.data_ptr(), flat.data_ptr(), total, g_lr.data_ptr(), stream)
            e1.record()
            _lib.check(rc, hd, "backward")
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def counts():
            c = (C.c_int64 * 4)()
            _lib.check(lib.hcf_train_backward_counts(hd, c), hd, "hcf_train_backward_counts")
            return [int(v) for v in c]

        forms = {"full": False, "inputs_only": True}
        for io in forms.values():
            for _ in range(args.warmup):
                sample(io)
        times = {k: [] for k in forms}
        cnt = {}
        gc.disable()
        try:
            for _ in range(args.rounds):
                for k, io in forms.items():
                    times[k].append(sum(sample(io) for _ in range(args.iters)) / args.iters)
                    cnt[k] = counts()
        finally:
            gc.enable()
        o = {k: summary(v) for k, v in times.items()}
        for k in forms:
            o[k]["counts_wgrad_batched_sum_axpy"] = cnt[k]
        o["full_spread_ms"] = round(o["full"]["max_ms"] - o["full"]["min_ms"], 3)
        o["inputs_only"]["minus_full_median_ms"] = round(o["inputs_only"]["median_ms"] - o["full"]["median_ms"], 3)
        o["fallbacks"] = eng.fallback_count()          # taped f16x3 passes re-run exactly (an activation beyond the f16 range)
        res[prec] = o
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
