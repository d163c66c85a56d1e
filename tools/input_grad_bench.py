"""ms per backward pass of the taped FORWARD passes differentiated w.r.t. their images, in the SAME run: the input-gradient-only
NLL backward (hcf_train_backward_ex with dparams = NULL: d nll / d hr and d nll / d lr, no parameter-gradient work) and the
input-gradient-only encode backward (hcf_train_backward_encode: dL/d hr from seeds on z, every eps_l and logp) beside the full NLL
backward (hcf_train_backward: every parameter gradient -- the reference point, the same code as before the image gradients
existed), at config 5's shape: SR_DF2K_4X, seeded weights, B = 16, HR 160 x 160, both conv precisions.

Method (tools/latent_grad_bench.py's): inputs resident in HBM; a backward pass consumes its tape, so every sample is one untimed
taped forward followed by ONE backward between two HIP events on the launch stream; warm-up samples of every form first, then
`--rounds` rounds that ALTERNATE the forms (`--iters` samples each, a device synchronise after each), Python's cyclic GC off inside
the timed region. Reported per backward pass: the median over the rounds and the spread (min, max) -- a difference inside the full
pass's own spread is not a difference. Expectation: an input-gradient-only pass runs a strict subset of the full pass's launches and
is not slower; slower by more than the spread is a finding to explain. The counters of hcf_train_backward_counts of the last pass of
each form go with it. One JSON line (stdout, and appended to --out).

    python tools/input_grad_bench.py [--iters 3] [--rounds 5] [--warmup 2] [--B 16] [--hr 160] [--out profiles/r12_input_grad_bench.json]
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
    assert torch.cuda.is_available(), "input_grad_bench needs an MI355X"
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
    g_hr, g_lr = torch.empty_like(hr), torch.empty_like(lr)
    total = sum(p.numel() for p in net._params())
    flat = torch.empty(total, device=dev)
    eps_arr = (C.c_void_p * len(eps))(*[e.data_ptr() for e in eps])
    geps_arr = (C.c_void_p * len(eps))(*[e.data_ptr() for e in g_eps])
    res = {"what": "input-gradient-only NLL and encode backward vs the full NLL backward of the taped forward pass",
           "preset": args.preset, "B": B, "hr": [H, H], "iters": args.iters, "rounds": args.rounds, "warmup": args.warmup,
           "parameters": total}
    for prec in [p for p in args.precisions.split(",") if p]:
        net.set_precision(prec)
        eng, idx = net._engine_for(dev)
        lib, hd = eng.lib, eng.handle
        stream = C.c_void_p(torch.cuda.current_stream(idx).cuda_stream)
        _lib.check(lib.hcf_train_select_tape(hd, 0), hd, "hcf_train_select_tape")

        def sample(form):
            if form == "encode_inputs_only":
                _lib.check(lib.hcf_train_encode_sr(hd, hr.data_ptr(), noise.data_ptr(), z.data_ptr(), eps_arr, len(eps), logp.data_ptr(),
                                                   B, H, H, 0, stream), hd, "hcf_train_encode_sr")
            else:
                _lib.check(lib.hcf_train_forward_sr(hd, hr.data_ptr(), lr.data_ptr(), noise.data_ptr(), out_lr.data_ptr(), nll.data_ptr(),
                                                    logdet.data_ptr(), B, H, H, stream), hd, "hcf_train_forward_sr")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if form == "encode_inputs_only":
                rc = lib.hcf_train_backward_encode(hd, g_z.data_ptr(), geps_arr, len(eps), g_logp.data_ptr(), None, 0, g_hr.data_ptr(),
                                                   stream)
            elif form == "nll_inputs_only":
                rc = lib.hcf_train_backward_ex(hd, 1.0, None, 0, g_hr.data_ptr(), g_lr.data_ptr(), stream)
            else:
                rc = lib.hcf_train_backward(hd, 1.0, flat.data_ptr(), total, stream)
            e1.record()
            _lib.check(rc, hd, "backward")
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        def counts():
            c = (C.c_int64 * 4)()
            _lib.check(lib.hcf_train_backward_counts(hd, c), hd, "hcf_train_backward_counts")
            return [int(v) for v in c]

        forms = ["nll_full", "nll_inputs_only", "encode_inputs_only"]
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
        o["nll_full_spread_ms"] = round(o["nll_full"]["max_ms"] - o["nll_full"]["min_ms"], 3)
        for k in forms[1:]:
            o[k]["minus_full_median_ms"] = round(o[k]["median_ms"] - o["nll_full"]["median_ms"], 3)
        o["fallbacks"] = eng.fallback_count()          # taped f16x3 passes re-run exactly (an activation beyond the f16 range)
        res[prec] = o
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
