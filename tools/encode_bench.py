"""ms per call of HCFlowNet_SR.encode (hcf_encode_sr) beside the unchanged NLL forward pass normal_flow_diracLR (hcf_forward_sr) in
the SAME run, at config 2's shape: SR_DF2K_4X, seeded weights, B = 16, HR 640 x 640, both conv precisions.

The forward pass is the yardstick: encode walks the same graph and additionally writes the eps tensors
(16 x (21 x 160^2 + 6 x 320^2) x 4 B = 74 MB per call). Method: inputs resident in HBM, warm-up calls of both first, then `--rounds`
rounds that ALTERNATE the two (each: `--iters` back-to-back calls between two HIP events on the launch stream, ended by a device
synchronise), Python's cyclic GC off inside the timed region. Reported per call: the median over the rounds and the spread
(min, max) -- a difference inside the forward pass's own spread is not a difference. `--streams 1` (default) runs encode on one
stream like the forward pass; `--streams 2` times the module default (two half batches on two side streams) as well.
One JSON line (stdout, and appended to --out).

    python tools/encode_bench.py [--iters 5] [--rounds 5] [--warmup 2] [--B 16] [--hr 640] [--out profiles/encode_bench.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd import HCFlowNet_SR, preset, make_params  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--hr", type=int, default=640)
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--precisions", default="f16x3,exact")
    ap.add_argument("--streams", default="1,2")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encode_bench needs an MI355X"
    cfg = preset(args.preset)
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 21), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to("cuda:0").eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    B, H = args.B, args.hr
    hr = torch.rand(B, 3, H, H, device="cuda", generator=g)
    lr = torch.rand(B, 3, H // cfg.scale, H // cfg.scale, device="cuda", generator=g)
    noise = torch.rand(B, 3, H, H, device="cuda", generator=g)
    streams = [int(s) for s in args.streams.split(",") if s]
    res = {"what": "encode vs the NLL forward pass", "preset": args.preset, "B": B, "hr": [H, H], "iters": args.iters,
           "rounds": args.rounds, "warmup": args.warmup,
           "eps_bytes_per_call": 4 * sum(int(torch.Size(s).numel()) for s in
                                         __import__("hcflow_amd").eps_shapes(cfg, B, H // cfg.scale, H // cfg.scale))}
    with torch.no_grad():
        for prec in [p for p in args.precisions.split(",") if p]:
            net.set_precision(prec)
            fns = {"forward": lambda: net.normal_flow_diracLR(hr, lr, noise=noise)}
            for s in streams:
                def enc(s=s):
                    net.set_streams(s)
                    return net.encode(hr, noise=noise)
                fns["encode_streams%d" % s] = enc
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            gc.disable()
            try:
                for _ in range(args.rounds):
                    for k, fn in fns.items():
                        times[k].append(timed(fn, args.iters))
            finally:
                gc.enable()
                net.set_streams(2)
            out = {k: summary(v) for k, v in times.items()}
            f = out["forward"]
            out["forward_spread_ms"] = round(f["max_ms"] - f["min_ms"], 3)
            for k in fns:
                if k != "forward":
                    out[k]["minus_forward_median_ms"] = round(out[k]["median_ms"] - f["median_ms"], 3)
            res[prec] = out
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
