"""ms per call of hcflow_amd.lpips.LPIPS (hcf_lpips_alex) beside the stock-PyTorch restatement of the same network on the same GPU
(F.conv2d / relu / max_pool2d in fp32 through MIOpen, the head in torch ops), for the two HR shapes of the test loop:
B = 16 pairs at 640 x 640 (config 2) and B = 32 pairs at 160 x 160 (config 3).

Method as DESIGN.md section 5: inputs resident in HBM, warm-up calls first, then `--iters` back-to-back calls between two HIP events
on the launch stream, Python's cyclic GC off inside the timed region. Besides the times it reports the FLOPs the native path
EXECUTES (conv1 as the 5x5 conv on the 4x4 space-to-depth grid, every conv over its whole launch grid, both inputs) against the
157.3 TFLOP/s fp32-matrix peak, and the algorithmic FLOPs of the five AlexNet convs. One JSON line per shape.

    python tools/lpips_bench.py [--iters 20] [--warmup 3]
"""
import argparse
import gc
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hcflow_amd.lpips import LPIPS  # noqa: E402

FP32_MATRIX_PEAK = 157.3e12


def stock(m, x0, x1):
    """The same network and head on stock PyTorch ops (fp32), NCHW."""
    sd = m.state_dict()
    keys = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
    w = [(sd[k + ".weight"], sd[k + ".bias"]) for k in keys]
    x = torch.cat([x0, x1], 0)
    x = (x - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    h1 = F.relu(F.conv2d(x, *w[0], stride=4, padding=2))
    h2 = F.relu(F.conv2d(F.max_pool2d(h1, 3, 2), *w[1], padding=2))
    h3 = F.relu(F.conv2d(F.max_pool2d(h2, 3, 2), *w[2], padding=1))
    h4 = F.relu(F.conv2d(h3, *w[3], padding=1))
    h5 = F.relu(F.conv2d(h4, *w[4], padding=1))
    B = x0.shape[0]
    val = 0
    for l, h in enumerate((h1, h2, h3, h4, h5)):
        n = h / (h.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        val = val + F.conv2d((n[:B] - n[B:]) ** 2, sd["lin%d.model.1.weight" % l]).mean(dim=(2, 3), keepdim=True)
    return val


def flops(B, H, W):
    """(executed by the native path, algorithmic) FLOPs of the five convs for B pairs."""
    N = 2 * B
    Hs, Ws = (H + 3) // 4, (W + 3) // 4
    H1, W1 = (H - 7) // 4 + 1, (W - 7) // 4 + 1
    H2, W2 = (H1 - 3) // 2 + 1, (W1 - 3) // 2 + 1
    H3, W3 = (H2 - 3) // 2 + 1, (W2 - 3) // 2 + 1
    # launch grids: 8 x 32 pixel tiles, 64 output channels per block
    tiles = lambda h, w: ((h + 7) // 8) * 8 * ((w + 31) // 32) * 32
    ex = 2 * N * (tiles(Hs, Ws) * 25 * 48 * 64 + tiles(H2, W2) * 25 * 64 * 192
                  + tiles(H3, W3) * 9 * (192 * 384 + 384 * 256 + 256 * 256))
    alg = 2 * N * (H1 * W1 * 121 * 3 * 64 + H2 * W2 * 25 * 64 * 192 + H3 * W3 * 9 * (192 * 384 + 384 * 256 + 256 * 256))
    return ex, alg


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    gc.disable()
    try:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
    finally:
        gc.enable()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    m = LPIPS(seed=0).cuda()
    g = torch.Generator(device="cuda").manual_seed(0)
    for B, H, W, tag in ((16, 640, 640, "config 2 HR"), (32, 160, 160, "config 3 HR")):
        x0 = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
        x1 = torch.rand(B, 3, H, W, device="cuda", generator=g) * 2 - 1
        with torch.no_grad():
            a, b = m(x0, x1), stock(m, x0, x1)
            rel = float(((a - b).abs() / b.abs()).max())
            t_nat = timed(lambda: m(x0, x1), args.iters, args.warmup)
            t_ref = timed(lambda: stock(m, x0, x1), args.iters, args.warmup)
        ex, alg = flops(B, H, W)
        print(json.dumps({
            "shape": "%s: B=%d pairs %dx%d" % (tag, B, H, W), "native_ms": round(t_nat, 3), "stock_pytorch_ms": round(t_ref, 3),
            "speedup": round(t_ref / t_nat, 2), "executed_gflop": round(ex / 1e9, 1), "algorithmic_gflop": round(alg / 1e9, 1),
            "executed_frac_of_fp32_matrix_peak": round(ex / (t_nat * 1e-3) / FP32_MATRIX_PEAK, 3),
            "max_rel_diff_native_vs_stock": rel, "iters": args.iters, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
