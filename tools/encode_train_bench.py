"""ms per training step (taped forward + full backward) of the TRAINABLE ENCODE -- hcf_train_encode_sr, then
hcf_train_backward_encode_ex with a gradient buffer: every parameter gradient from seeds on z, every eps_l and logp (per sample) --
beside the NLL step (hcf_train_forward_sr + hcf_train_backward) in the SAME run, at config 5's shape: SR_DF2K_4X, seeded weights,
B = 16, HR 160 x 160, both conv precisions.

The two steps share every launch but the output end: the encode has the fused prior kernels (eps out + logp) where the NLL has the
logp-only ones, an NCHW copy of z where the NLL has the Dirac-LR term, the seed-sum launch (sum_b g_logp[b] on the device) in
front of the backward pass, and the NCHW seed adds. Expectation: the same time within the run's spread.

Method (tools/input_grad_bench.py's): inputs resident in HBM; every sample is one taped forward and ONE backward between two HIP
events on the launch stream; warm-up samples of both forms first, then `--rounds` rounds that ALTERNATE the forms (`--iters`
samples each, a device synchronise after each), Python's cyclic GC off inside the timed region. Reported per step: the median over
the rounds and the spread (min, max), the ratio of the medians and the difference beside the NLL step's own spread -- a difference
inside that spread is not a difference. The counters of hcf_train_backward_counts of the last pass of each form (the launch list
of the parameter-gradient work) go with it. One JSON line (stdout, and appended to --out).

    python tools/encode_train_bench.py [--iters 3] [--rounds 5] [--warmup 2] [--B 16] [--hr 160] [--out profiles/encode_train_bench.json]
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
    ap.add_argument("--hr", type=int, default=160)
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--precisions", default="f16x3,exact")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encode_train_bench needs an MI355X"
    dev = torch.device("cuda:0")
    cfg = preset(args.preset)
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 21), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(dev).eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    B, H = args.B, args.hr
    h = H // cfg.scale
    hr = torch.rand(B, 3, H, H, device=dev, generator=g)
    noise = torch.rand(B, 3, H, H, device=dev, generator=g)
    lr = torch.rand(B, 3, h, h, device=dev, generator=g)
    out_lr, nll, logdet = torch.empty_like(lr), torch.empty(1, device=dev), torch.empty(B, device=dev)
    z, logp = torch.empty_like(lr), torch.empty(B, device=dev)
    eps = [torch.empty(s, device=dev) for s in eps_shapes(cfg, B, h, h)]
    g_z = torch.randn(z.shape, device=dev, generator=g) / z.numel()
    g_eps = [torch.randn(e.shape, device=dev, generator=g) / e.numel() for e in eps]
    g_logp = torch.rand(B, device=dev, generator=g) / (B * H * H)
    total = sum(p.numel() for p in net._params())
    flat = torch.empty(total, device=dev)
    eps_arr = (C.c_void_p * len(eps))(*[e.data_ptr() for e in eps])
    geps_arr = (C.c_void_p * len(eps))(*[e.data_ptr() for e in g_eps])
    res = {"what": "trainable encode step (taped forward + full backward) vs the NLL step", "preset": args.preset, "B": B,
           "hr": [H, H], "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup, "parameters": total}
    for prec in [p for p in args.precisions.split(",") if p]:
        net.set_precision(prec)
        eng, idx = net._engine_for(dev)
        lib, hd = eng.lib, eng.handle
        stream = C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
        _lib.check(lib.hcf_train_select_tape(hd, 0), hd, "hcf_train_select_tape")

        def sample(form):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if form == "encode_step":
                _lib.check(lib.hcf_train_encode_sr(hd, hr.data_ptr(), noise.data_ptr(), z.data_ptr(), eps_arr, len(eps), logp.data_ptr(),
                                                   B, H, H, 0, stream), hd, "hcf_train_encode_sr")
                rc = lib.hcf_train_backward_encode_ex(hd, g_z.data_ptr(), geps_arr, len(eps), g_logp.data_ptr(), flat.data_ptr(), total,
                                                   None, stream)
            else:
                _lib.check(lib.hcf_train_forward_sr(hd, hr.data_ptr(), lr.data_ptr(), noise.data_ptr(), out_lr.data_ptr(), nll.data_ptr(),
                                                    logdet.data_ptr(), B, H, H, stream), hd, "hcf_train_forward_sr")
                rc = lib.hcf_train_backward(hd, 1.0, flat.data_ptr(), total, stream)
            e1.record()
            _lib.check(rc, hd, "backward")
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def counts():
            c = (C.c_int64 * 4)()
            _lib.check(lib.hcf_train_backward_counts(hd, c), hd, "hcf_train_backward_counts")
            return [int(v) for v in c]

        forms = ["nll_step", "encode_step"]
        for f in forms:
            for _ in range(args.warmup):
                sample(f)
        times = {k: [] for k in forms}
        cnt = {}
        gc.disable()
        try:
            for _ in range(args.rounds):
                for k in forms:
                    times[k].append(sum(sample(k) for _ in range(args.iters)) / args.iters)
                    cnt[k] = counts()
        finally:
            gc.enable()
        o = {k: summary(v) for k, v in times.items()}
        for k in forms:
            o[k]["counts_wgrad_batched_sum_axpy"] = cnt[k]
        o["nll_step_spread_ms"] = round(o["nll_step"]["max_ms"] - o["nll_step"]["min_ms"], 3)
        o["encode_minus_nll_median_ms"] = round(o["encode_step"]["median_ms"] - o["nll_step"]["median_ms"], 3)
        o["encode_over_nll"] = round(o["encode_step"]["median_ms"] / o["nll_step"]["median_ms"], 4)
        o["fallbacks"] = eng.fallback_count()          # taped f16x3 passes re-run exactly (an activation beyond the f16 range)
        res[prec] = o
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
