"""Latent-space demo of HCFlowNet_SR.encode / decode and hcflow_amd.latent: encode two images, then write

    recon.npy        decode(encode(hr)) of both images (the exact reconstruction) and its max |diff| to the inputs
    tau_sweep.npy    image 0 re-decoded at scale(eps, tau) for tau in --taus
    slerp_path.npy   decode along slerp(eps of image 0, eps of image 1, t), the LR latent interpolated linearly, for --steps values of t
    refined.npy      latent.refine_image: a tau = 0.8 sample of image 0's 8-bit LR latent after --refine-steps gradient steps on its
                     NLL with the weights frozen (the flow as an image prior), and the NLL before / after

The images are crops of the bundled example pair (tests/golden/real_images.npz) or, with --seeded, seeded random inputs; the weights
are the seeded recipe (a trained checkpoint loads with --state-dict PATH: a torch.save'd state dict). Not run by any test.

    python tools/latent_demo.py [--preset SR_DF2K_4X] [--size 160] [--out latent_demo_out] [--taus 0,0.5,0.8,1] [--steps 5]
                                [--refine-steps 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hcflow_amd import HCFlowNet_SR, preset, make_params, latent  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="SR_DF2K_4X")
    ap.add_argument("--size", type=int, default=160, help="HR crop size (a multiple of the scale)")
    ap.add_argument("--out", default="latent_demo_out")
    ap.add_argument("--taus", default="0,0.5,0.8,1")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--refine-steps", type=int, default=20)
    ap.add_argument("--seeded", action="store_true")
    ap.add_argument("--state-dict", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "latent_demo needs an MI355X"
    cfg = preset(args.preset)
    S = args.size
    assert S % cfg.scale == 0
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(torch.load(args.state_dict, map_location="cpu") if args.state_dict else make_params(cfg, 21), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to("cuda:0").eval()
    if args.seeded:
        hr = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(0))
    else:
        im = np.load(os.path.join(ROOT, "tests", "golden", "real_images.npz"), allow_pickle=False)
        crops = []
        for key in ("butterfly_hr", "face_hr"):
            a = im[key]
            a = a[0] if a.ndim == 4 else a
            assert a.shape[0] >= S and a.shape[1] >= S, (key, a.shape, S)
            crops.append(torch.from_numpy(np.ascontiguousarray(a[:S, :S].transpose(2, 0, 1))).float() / 255.)
        hr = torch.stack(crops)
    hr = hr.cuda()
    os.makedirs(args.out, exist_ok=True)
    with torch.no_grad():
        z, eps, logp = net.encode(hr)
        recon = net.decode(z, eps)
        err = float((recon - hr).abs().max())
        print("reconstruction max|diff| %.3e; log-density per sample (nats, without the Dirac-LR term): %s" % (err, logp.tolist()))
        np.save(os.path.join(args.out, "recon.npy"), recon.cpu().numpy())
        e0, e1 = [e[:1] for e in eps], [e[1:2] for e in eps]
        taus = [float(v) for v in args.taus.split(",")]
        sweep = torch.cat([net.decode(z[:1], latent.scale(e0, tau), clamp=True) for tau in taus])
        np.save(os.path.join(args.out, "tau_sweep.npy"), sweep.cpu().numpy())
        ts = [i / max(1, args.steps - 1) for i in range(args.steps)]
        path = torch.cat([net.decode(torch.lerp(z[:1], z[1:2], tt), latent.slerp(e0, e1, tt), clamp=True) for tt in ts])
        np.save(os.path.join(args.out, "slerp_path.npy"), path.cpu().numpy())
        # likelihood-guided refinement: an SR sample of the 8-bit LR latent, moved down its own NLL (weights frozen inside)
        lq = (torch.clamp(z[:1], 0, 1) * 255.).round() / 255.
        sample = net.decode(lq, latent.scale(e0, 0.8))
    refined, _, nlls = latent.refine_image(net, sample, lq, steps=args.refine_steps)
    if nlls:
        print("refine_image: nll %.4f -> %.4f bits/dim over %d steps, max |move| %.3e" % (nlls[0], nlls[-1], len(nlls),
                                                                                       float((refined - sample).abs().max())))
    np.save(os.path.join(args.out, "refined.npy"), refined.cpu().numpy())
    print("wrote refined.npy, recon.npy, tau_sweep.npy %s, slerp_path.npy %s under %s" % (tuple(sweep.shape), tuple(path.shape), args.out))


if __name__ == "__main__":
    main()
