#!/usr/bin/env python
"""Encode fixtures written by the REFERENCE (runs only where a checkout of the reference is at hand).

    python tests/golden/make_encode_golden.py --reference <reference checkout>/codes     # writes tests/golden/encode_*.npz

The reference's HCFlowNet_SR is built as make_golden.build does (seeded parameter recipe, strict load). For the duration of ONE
normal_flow_diracLR call Basic.GaussianDiag.logp is wrapped so that it records (mean, logs, x) of every conditional prior and the
value of the Dirac-LR call (told apart by its constant logs = -6, HCFlowNet_SR_arch.py:63); the torch.rand draw is captured by
make_golden's recorder. Stored: hr, the noise draw, the pre-quantisation latent z, eps_i = (x - mean) * exp(-logs) in the order the
inverse pass takes, the per-sample log-density WITHOUT the Dirac term (objective - recorded Dirac value), and the reference's own
reverse_flow fed those eps from the unquantised z. Fixtures are DATA only.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402
from hcflow_amd.config import preset, eps_shapes  # noqa: E402
from hcflow_amd.params import param_digest  # noqa: E402


class RecordLogp:
    def __init__(self, Basic):
        self.G = Basic.GaussianDiag
        self.priors, self.dirac = [], []

    def __enter__(self):
        self.old = self.G.__dict__["logp"]
        fn = self.old.__func__

        def logp(mean, logs, x):
            out = fn(mean, logs, x)
            if tuple(mean.shape[1:2]) == (3,) and bool((logs == -6).all()):
                self.dirac.append(out.clone())
            else:
                self.priors.append((mean.clone(), logs.clone(), x.clone()))
            return out

        self.G.logp = staticmethod(logp)
        return self

    def __exit__(self, *exc):
        self.G.logp = self.old


def gen(name, preset_name, ref_sr, B, h, w, seed):
    from models.modules import Basic
    cfg = preset(preset_name)
    net, params = MG.build(ref_sr, cfg, seed)
    g = torch.Generator().manual_seed(seed + 29)
    H, W = h * cfg.scale, w * cfg.scale
    hr = torch.rand(B, 3, H, W, generator=g)
    lr = torch.rand(B, 3, h, w, generator=g)
    dg = param_digest(params)
    out = {"preset": preset_name, "seed": seed, "hr": MG.np_(hr), "lr": MG.np_(lr),
           "digest": np.array([dg["n"], dg["sum"], dg["sumsq"], dg["probe"]], dtype=np.float64)}
    with torch.no_grad():
        with MG.Capture() as cap, RecordLogp(Basic) as rec:
            lr_hat, nll = net(hr=hr, lr=lr, reverse=False)
        noise = cap.rand[0]
        assert len(rec.dirac) == 1 and len(rec.priors) == cfg.L
        pixels = H * W
        x = hr + noise / net.quant
        logdet0 = torch.zeros_like(hr[:, 0, 0, 0]) + float(-np.log(net.quant) * pixels)
        z, objective_wo_dirac = net.flow(hr=x, u=None, logdet=logdet0, reverse=False, training=True)
        objective = objective_wo_dirac + rec.dirac[0]
        assert abs(float(((-objective) / float(np.log(2.) * pixels)).mean()) - float(nll)) <= 1e-6 * abs(float(nll))
        # the priors are evaluated deepest level first (FlowNet_SR_x4.py:95-99): already the order of the inverse pass
        eps = [(xx - mean) * torch.exp(-logs) for mean, logs, xx in rec.priors]
        assert [tuple(e.shape) for e in eps] == [tuple(s) for s in eps_shapes(cfg, B, h, w)], [e.shape for e in eps]
        with MG.Capture(replay_normal=eps):
            rt = net.flow(z=z, eps_std=1.0, reverse=True)
        err = float((rt - x).abs().max())
        print("  %s nll %.6f  |eps| max %.3f  z range [%.3f, %.3f]  reference round trip max|diff| %.3e" % (
            name, float(nll), max(float(e.abs().max()) for e in eps), float(z.min()), float(z.max()), err))
        assert err <= 1e-4
        out.update(fwd_noise=MG.np_(noise), z=MG.np_(z), logp=MG.np_(objective_wo_dirac), dirac=MG.np_(rec.dirac[0]),
                   nll=np.float64(float(nll)), rt_raw=MG.np_(rt))
        for i, e in enumerate(eps):
            out["eps%d" % i] = MG.np_(e)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("wrote", path, "%.1f KB" % (os.path.getsize(path) / 1024))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("HCFLOW_REFERENCE", MG.REF), help="the reference's codes/ directory")
    args = ap.parse_args()
    MG.REF = args.reference
    ref_sr, _ = MG.import_reference()
    gen("encode_sr4_tiny", "SR_4X_tiny", ref_sr, 2, 12, 16, 11)
    gen("encode_sr8_tiny", "SR_8X_tiny", ref_sr, 2, 5, 7, 12)


if __name__ == "__main__":
    main()
