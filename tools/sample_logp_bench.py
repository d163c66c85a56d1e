"""ms per call of the three ways to a sample and its log-density, in the SAME run, at config 2's shape (SR_DF2K_4X, seeded weights,
B = 16, LR 160 x 160, tau 0.8) and at config 1's (B = 1):

  (a) inverse          net(lr=lr, eps_std=tau, reverse=True): the plain sampling call, which returns no density
  (b) inverse_encode   (a) followed by net.encode(sr): today's way to log p(x | lr) of the sample -- a second full pass
  (c) sample_with_logp HCFlowNet_SR.sample_with_logp (hcf_inverse_logp): the density out of the sampling pass itself

Method (tools/encode_bench.py's): inputs resident in HBM, warm-up calls of all three first, then `--rounds` rounds that ALTERNATE
the three (each: `--iters` back-to-back calls between two HIP events on the launch stream, ended by a device synchronise),
Python's cyclic GC off inside the timed region, one seed for every call. Reported per call: the median over the rounds and the
spread (min, max), (c) - (a) beside the spread of (a) -- a difference inside that spread is not a difference -- and (c) against
(b). The module defaults apply (f16x3, a batch of >= 4 as two half batches on two side streams).
One JSON line per shape (stdout, and appended to --out).

    python tools/sample_logp_bench.py [--iters 5] [--rounds 5] [--warmup 2] [--batches 16,1] [--lr 160] [--out profiles/sample_logp_bench.json]
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
    ap.add_argument("--batches", default="16,1")
    ap.add_argument("--lr", type=int, default=160)
    ap.add_argument("--tau", type=float, default=0.8)
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sample_logp_bench needs an MI355X"
    cfg = preset(args.preset)
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 21), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to("cuda:0").eval().set_precision(args.precision)
    g = torch.Generator(device="cuda").manual_seed(0)
    tau, h = args.tau, args.lr
    for B in [int(b) for b in args.batches.split(",") if b]:
        lr = torch.rand(B, 3, h, h, device="cuda", generator=g)
        res = {"what": "sample + log-density: inverse / inverse + encode / sample_with_logp", "preset": args.preset, "B": B,
               "lr": [h, h], "tau": tau, "precision": args.precision, "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup}

        def inv_enc():
            return net.encode(net(lr=lr, eps_std=tau, reverse=True, seed=1))

        fns = {"inverse": lambda: net(lr=lr, eps_std=tau, reverse=True, seed=1), "inverse_encode": inv_enc,
               "sample_with_logp": lambda: net.sample_with_logp(lr, tau, seed=1)}
        with torch.no_grad():
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
        out = {k: summary(v) for k, v in times.items()}
        a, b, c = out["inverse"], out["inverse_encode"], out["sample_with_logp"]
        res.update(out)
        res["inverse_spread_ms"] = round(a["max_ms"] - a["min_ms"], 3)
        res["logp_minus_inverse_median_ms"] = round(c["median_ms"] - a["median_ms"], 3)
        res["logp_over_inverse_encode"] = round(c["median_ms"] / b["median_ms"], 4)
        line = json.dumps(res)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
