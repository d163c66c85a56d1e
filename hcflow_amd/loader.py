"""Batch > 1 test loading and batched evaluation.

The reference's test loader is hard-wired to one image per step (``codes/data/__init__.py:24``: ``DataLoader(dataset,
batch_size=1, shuffle=False, num_workers=0)``) and its metrics loop (``test_HCFlow.py:85-182``) converts every sample to a
uint8 numpy image on the host. On an MI355X a single 160x160 LR image leaves the GPU idle most of the time (B = 1: 21.6 ms per
image, B = 16: 8.6 ms per image). This module is the drop-in for those two pieces:

* ``batched_test_loader(dataset, batch_size)`` walks ANY reference dataset (``__len__`` / ``__getitem__`` returning the
  reference's dict: ``LQ`` [3,h,w], optional ``GT`` [3,H,W], ``LQ_path`` / ``GT_path``) in order and stacks consecutive items of
  identical shape into one batch (test sets mix image sizes: a size change closes the batch), yielding the dict
  ``feed_data`` expects (``HCFlow_SR_model.py:177-182``) with lists of paths;
* ``evaluate_batch(net, batch, heats, n_sample, scale, crop_border)`` runs what ``HCFlowSRModel.test()`` runs
  (``HCFlow_SR_model.py:281-301``: NLL pass + one sampling pass per heat and sample) on the whole batch and computes the log
  line's numbers per image on the device (hcflow_amd/metrics.py: PSNR / SSIM / PSNR_Y / SSIM_Y of SR vs GT with the border
  crop, the same on the bicubic down-scaled pair, LR consistency, sample diversity). LPIPS is computed when an ``lpips_fn`` is
  passed, e.g. ``hcflow_amd.lpips.LPIPS(...).cuda()`` (AlexNet v0.1 on the HIP kernels, weights from local files);
* ``evaluate_sample_set(net, batch, heats, n_sample, lpips_map)`` judges the same samples as a SET with an
  ``hcflow_amd.lpips.LPIPSMap``: per image and heat the mean LPIPS, the best whole sample, the mean of the per-pixel best over the
  samples and their relative gap (defined in ``hcflow_amd/lpips.py``), the GT going through AlexNet once per heat;
* ``evaluate_sweep(net, batch, heats, n_sample, scale)`` returns ``evaluate_batch``'s dict with the heats sharing calls: the rows
  of one call are (image, heat) pairs, each with its own temperature, and the diversity comes from a streaming
  ``metrics.SampleStats`` instead of the held samples;
* ``most_likely_samples(net, batch, heat, n_sample)`` keeps, per image, the most likely of ``n_sample`` draws under the model
  itself (``HCFlowNet_SR.sample_with_logp``): best-of-M selection that needs no GT.

``net`` is an ``HCFlowNet_SR`` or an ``HCFlowNet_Rescaling``; the three ``evaluate_*`` functions dispatch on ``net.cfg.sr`` and share
everything behind the first pass. An SR net runs ``HCFlowSRModel.test()``: the NLL pass of (GT, LQ), then samples drawn from the
dataset's LQ. A rescaling net runs ``HCFLowRescalingModel.test()`` (``HCFlow_Rescaling_model.py:306-324``): GT -> LR^ in one forward
pass over the batch, ``metrics.quantize`` (the reference's ``Quantization``, ``Basic.py:186-202``), then every heat and sample is
the inverse from the QUANTISED LR^ -- one tensor held for the whole call, so ``cache_cond=True`` hits. Its batch must hold "GT"; "LQ"
is optional and only feeds the "lr" entry (bicubic LQ against the quantised LR^, the "LR" columns of the log line); its "nll" is the
reference's ``fake_z1.mean()`` per image, the mean of the first split latent (not a likelihood: the log line's column name is kept).

The numbers per image are identical to feeding the images one at a time (every op of the path is per sample)."""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

import torch

from . import metrics as M


def batched_test_loader(dataset, batch_size: int = 16, keys: Sequence[str] = ("LQ", "GT")) -> Iterator[Dict]:
    """Order-preserving batches of same-shaped items of a reference test dataset."""
    assert batch_size >= 1
    pend: List[Dict] = []

    def shape_of(item):
        return tuple(tuple(item[k].shape) for k in keys if k in item and torch.is_tensor(item[k]))

    def flush():
        out: Dict = {}
        for k in pend[0]:
            vals = [it[k] for it in pend]
            out[k] = torch.stack(vals, 0) if torch.is_tensor(vals[0]) else vals
        pend.clear()
        return out

    for i in range(len(dataset)):
        item = dataset[i]
        if pend and (len(pend) == batch_size or shape_of(item) != shape_of(pend[0])):
            yield flush()
        pend.append(item)
    if pend:
        yield flush()


def evaluate_batch(net, batch: Dict, heats: Iterable[float], n_sample: int, scale: int, crop_border: Optional[int] = None,
                   seed: Optional[int] = None, noise: Optional[torch.Tensor] = None, lpips_fn=None) -> List[Dict]:
    """Per image of the batch: {"nll": float, "lr": {psnr, ssim, psnr_y, ssim_y} of LR^ vs LQ (SR nets), and per heat:
    {"psnr", "ssim", "psnr_y", "ssim_y", "bic_psnr", ... (means over the samples), "diversity"}} -- the numbers of the
    reference's per-image log line (test_HCFlow.py:166-175). LPIPS needs the ``lpips`` package's pretrained AlexNet: pass the
    caller's own module as ``lpips_fn`` (``lpips.LPIPS(net='alex').to('cuda')``, test_HCFlow.py:48) and every heat entry gets
    "lpips" = the mean over the samples of ``lpips_fn(2 gt - 1, 2 sr - 1)`` per image (:132-133, :168), evaluated on the whole
    batch at once; without it the key is absent. ``net`` is an eval()-mode HCFlowNet_SR or HCFlowNet_Rescaling on a GPU; the
    family (``net.cfg.sr``) decides what runs in front of the sampling and what the samples are drawn from (``_nll_pass``): for a
    rescaling net the batch must hold "GT" (ValueError otherwise), "nll" is the reference's ``fake_z1.mean()`` per image, "lr"
    (only with an "LQ" in the batch) compares the bicubic LQ with the quantised LR^, and every sample is drawn from that quantised
    LR^ (HCFlow_Rescaling_model.py:306-324); ``noise`` must stay None.
    ``seed`` fixes the device draws of the samples, ``noise`` ([B,3,H,W] in [0,1)) replaces the dequantisation noise of the
    NLL pass (HCFlowNet_SR_arch.py:52); both default to fresh draws, as in the reference.
    The PSNR / SSIM block stays on the device (``metrics.PairMetrics``): the GT is prepared once per call, every sample is one
    ``compare`` into a device row, the per-sample LPIPS values stay on the device too, the means over the samples are taken
    there in float64 and each heat's numbers are read back once."""
    pm = M.PairMetrics()
    crop = scale if crop_border is None else crop_border          # test_HCFlow.py:48
    with torch.no_grad():
        res, lq, gt = _nll_pass(net, batch, pm, noise)
        _heat_entries(res, net, pm, lq, gt, heats, n_sample, scale, crop, seed, lpips_fn)
    return res


def _nll_pass(net, batch: Dict, pm: "M.PairMetrics", noise: Optional[torch.Tensor] = None):
    """The part of a test step in front of the sampling, by model family (``net.cfg.sr``) -> (res, cond, gt): ``res`` the per-image
    dicts holding "nll" and "lr", ``cond`` the ONE tensor every sample of the call is drawn from, ``gt`` the GT batch or None.

    SR net (HCFlowSRModel.test(), HCFlow_SR_model.py:281-301): the NLL pass of (GT, LQ) when there is a GT; cond = LQ.
    Rescaling net (HCFLowRescalingModel.test(), HCFlow_Rescaling_model.py:306-324): one forward pass GT -> LR^ over the batch, then
    ``metrics.quantize``; cond = the quantised LR^ (``net.downscale``). "nll" is the reference's return value ``fake_z1.mean()``
    per image (the mean of the first split latent, NOT a likelihood: the column name is the log line's); "lr" compares the
    dataset's bicubic LQ with the quantised LR^ ("LR" columns of the line) and is present only when the batch has an "LQ"."""
    dev = next(net.parameters()).device
    if not net.cfg.sr:
        if "GT" not in batch:
            raise ValueError("evaluating a rescaling net needs the batch's \"GT\": its test step starts from the HR image")
        if noise is not None:
            raise ValueError("noise= belongs to the SR nets' NLL pass; a rescaling net's forward pass draws nothing")
        gt = batch["GT"].to(dev)
        B = gt.shape[0]
        res: List[Dict] = [dict() for _ in range(B)]
        lr_q, z1, _ = net.downscale(gt)
        # fake_z1.mean() of a batch of one, image by image (the same reduction as the reference's call); one readback
        for b, v in enumerate(torch.stack([z1[b:b + 1].mean() for b in range(B)]).cpu().tolist()):
            res[b]["nll"] = v
        if "LQ" in batch:
            for b, m in enumerate(M.rows_to_dicts(pm.compare(pm.embed(batch["LQ"].to(dev), 0, 0), lr_q))):
                res[b]["lr"] = {k: m[k] for k in ("psnr", "ssim", "psnr_y", "ssim_y")}
        return res, lr_q, gt
    lq = batch["LQ"].to(dev)
    gt = batch["GT"].to(dev) if "GT" in batch else None
    B = lq.shape[0]
    res = [dict() for _ in range(B)]
    if gt is not None:
        # per-image NLL: the engine returns the objective (logdet + log p) of every sample; nll_b = -obj_b / (ln 2 * H W)
        # (HCFlowNet_SR_arch.py:62-66: the reference's nll.mean() over a batch of one is exactly this)
        lr_hat, _, obj, _ = net.normal_flow_diracLR(gt, lq, noise=noise, return_internals=True)
        pix = float(gt.shape[2] * gt.shape[3])
        for b, o in enumerate(obj.double().cpu().tolist()):
            res[b]["nll"] = -o / (0.6931471805599453 * pix)
        for b, m in enumerate(M.rows_to_dicts(pm.compare(pm.embed(lq, 0, 0), lr_hat))):
            res[b]["lr"] = {k: m[k] for k in ("psnr", "ssim", "psnr_y", "ssim_y")}
    return res, lq, gt


def _heat_entries(res: List[Dict], net, pm: "M.PairMetrics", lq: torch.Tensor, gt: Optional[torch.Tensor], heats: Iterable[float],
                  n_sample: int, scale: int, crop: int, seed: Optional[int], lpips_fn) -> None:
    """``evaluate_batch``'s entry per heat, for either family: ``n_sample`` draws from ``lq`` (an SR net's LQ, a rescaling net's
    quantised LR^) per heat, compared with the GT prepared once."""
    B = lq.shape[0]
    ref = pm.embed(gt, crop, scale) if gt is not None and n_sample > 0 else None      # the GT is prepared once per call
    for hi, heat in enumerate(heats):
        samples, lps = [], []
        pset = M.PairSampleSet(pm, ref, n_sample) if ref is not None else None
        for s in range(n_sample):
            kw = {} if seed is None else {"seed": seed + 1000 * hi + s}
            # every heat / sample of the sweep conditions on the SAME lq: the deepest level's conditional features (the RRDB
            # trunk: most of a Face x8 call) are computed once and reused, bit-identical outputs (arch.py: cache_cond)
            sr = net(lr=lq, z=None, u=None, eps_std=heat, reverse=True, training=False, cache_cond=True, **kw)
            samples.append(sr)
            if pset is not None:                                   # one compare into a device row; LPIPS stays there too
                pset.add(sr)
                if lpips_fn is not None:
                    lps.append(lpips_fn(2 * gt - 1, 2 * sr - 1).reshape(B, -1).mean(dim=1))      # [B, 1, 1, 1] -> one value per image
        rows = _heat_rows(pset, lps) if pset is not None else [[0.0] * 9] * B             # no samples: zeros, as a sum of none
        for b in range(B):
            ent = dict(zip(M.KEYS, rows[b][:8])) if gt is not None else {}
            if gt is not None and lpips_fn is not None:
                ent["lpips"] = rows[b][-1]
            ent["diversity"] = M.diversity([s[b:b + 1] for s in samples]) if n_sample > 1 else 0.0
            res[b][float(heat)] = ent


def _heat_rows(pset: "M.PairSampleSet", lps: List[torch.Tensor]) -> List[List[float]]:
    """One readback of a sample set's numbers: per image the eight float64 means over the samples and, when ``lps`` (the samples'
    per-image LPIPS vectors) is not empty, their float64 mean as a ninth column."""
    cols = [pset.result()["mean"]]
    if lps:
        cols.append(torch.stack(lps, 0).double().mean(dim=0).unsqueeze(1))
    return torch.cat(cols, 1).cpu().tolist()


def sweep_chunks(B: int, n_heats: int, max_batch: int = 16) -> List[Tuple[int, int]]:
    """The call plan of ``evaluate_sweep``: the R = B * n_heats rows (image b, heat hi) -> r = b * n_heats + hi, cut in order into
    contiguous chunks [(row0, rows)] of at most ``max_batch`` rows, one inverse call each."""
    if B < 0 or n_heats < 0 or max_batch < 1:
        raise ValueError("sweep_chunks: B >= 0, n_heats >= 0 and max_batch >= 1 expected, got %r, %r, %r" % (B, n_heats, max_batch))
    R = B * n_heats
    return [(r0, min(max_batch, R - r0)) for r0 in range(0, R, max_batch)]


def evaluate_sweep(net, batch: Dict, heats: Iterable[float], n_sample: int, scale: int, crop_border: Optional[int] = None,
                   seed: Optional[int] = None, lpips_fn=None, max_batch: int = 16) -> List[Dict]:
    """``evaluate_batch``'s per-image dict ("nll", "lr", and per heat the eight metric keys, the optional "lpips", "diversity")
    with the heats SHARING calls: the reference's validation loop draws every (heat, sample) pair of an image in a call of its
    own (test_HCFlow.py:116-131, HCFlow_SR_model.py:296-316); here the rows of a call each carry their temperature
    (``eps_std`` as a vector, hcflow_amd/arch.py).

    Rows are the (image b, heat hi) pairs, r = b * len(heats) + hi. Sample s is ONE pass over all rows with ``seed + s``, cut by
    ``sweep_chunks`` into calls of at most ``max_batch`` rows: ``lr`` = the rows' images, ``eps_std`` = the rows' heats,
    ``sample_offset`` = the chunk's first row, ``cache_cond=True`` (which pays when a pass is a single chunk: the kept features
    are those of the last call). Row r of sample s therefore IS
    ``net(lr=lq[b:b+1], eps_std=heats[hi], seed=seed + s, sample_offset=r, reverse=True, training=False)`` whatever ``max_batch``
    is -- other draws than ``evaluate_batch``'s (seed + 1000 hi + s over the image batch), the same distribution. ``seed=None``
    draws a fresh seed per sample pass. The samples are not kept: one ``metrics.SampleStats`` over the R rows accumulates the
    diversity; PSNR / SSIM / LPIPS are evaluated per chunk against the matching GT rows and averaged as in ``evaluate_batch``.
    Each chunk's GT rows are prepared once, every (sample, chunk) is one ``compare`` into a device row, and a chunk's means are
    read back once at the end (see ``evaluate_batch``)."""
    heats = [float(t) for t in heats]
    dev = next(net.parameters()).device
    crop = scale if crop_border is None else crop_border          # test_HCFlow.py:48
    with torch.no_grad():
        res, lq, gt = _nll_pass(net, batch, M.PairMetrics())      # "nll" and "lr"; lq: the LQ, or a rescaling net's quantised LR^
    B, nH = lq.shape[0], len(heats)
    chunks = sweep_chunks(B, nH, max_batch)
    if not chunks or n_sample < 1:
        return res
    R = B * nH
    image_of = torch.arange(R, device=dev) // nH
    taus = torch.tensor(heats, dtype=torch.float32).repeat(B)                        # host: validated there, per call
    # one tensor per chunk, held for the whole sweep: the kept conditional features are keyed by the tensor they came from
    lq_rows = lq[image_of]
    lq_c = [lq_rows[r0:r0 + n] for r0, n in chunks]
    gt_c = None if gt is None else [gt[image_of[r0:r0 + n]] for r0, n in chunks]
    stats = None
    if gt is not None:
        pm = M.PairMetrics()
        psets = [M.PairSampleSet(pm, pm.embed(g, crop, scale), n_sample) for g in gt_c]
        lps: List[List[torch.Tensor]] = [[] for _ in chunks]
    with torch.no_grad():
        for s in range(n_sample):
            sd = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else seed + s
            outs = []
            for ci, (r0, n) in enumerate(chunks):
                sr = net(lr=lq_c[ci], z=None, u=None, eps_std=taus[r0:r0 + n], reverse=True, training=False, seed=sd,
                         sample_offset=r0, cache_cond=True)
                outs.append(sr)
                if gt is not None:
                    psets[ci].add(sr)
                    if lpips_fn is not None:
                        lps[ci].append(lpips_fn(2 * gt_c[ci] - 1, 2 * sr - 1).reshape(n, -1).mean(dim=1))
            if n_sample > 1:
                rows = outs[0] if len(outs) == 1 else torch.cat(outs, 0)
                stats = M.SampleStats.like(rows) if stats is None else stats
                stats.add(rows)
        div = stats.result()["diversity"].cpu().tolist() if stats is not None else [0.0] * R
        means = [] if gt is None else [row for ci in range(len(chunks)) for row in _heat_rows(psets[ci], lps[ci])]
    for r in range(R):
        ent = dict(zip(M.KEYS, means[r][:8])) if gt is not None else {}
        if gt is not None and lpips_fn is not None:
            ent["lpips"] = means[r][-1]
        ent["diversity"] = div[r]
        res[r // nH][heats[r % nH]] = ent
    return res


def evaluate_sample_set(net, batch: Dict, heats: Iterable[float], n_sample: int, lpips_map, seed: Optional[int] = None) -> List[Dict]:
    """Per image of the batch and per heat: {"lpips": mean over the samples of the scalar LPIPS (``evaluate_batch``'s "lpips"),
    "lpips_best": the best whole sample's map mean, "local_best": the mean of the per-pixel best over the samples, "score":
    (lpips_best - local_best) / lpips_best} as floats -- ``global_best`` / ``local_best`` / ``score`` of
    ``hcflow_amd.lpips.LPIPSMap.sample_set`` (defined there). ``lpips_map`` is an ``LPIPSMap`` on the net's device. Per heat the
    samples are those of ``evaluate_batch`` (seeds ``seed + 1000 * hi + s``, ``cache_cond=True``; drawn from the LQ for an SR net,
    from the quantised LR^ of ``net.downscale(gt)`` for a rescaling net, which needs no "LQ"); the GT goes through AlexNet once
    per heat, the samples accumulate on the device, and each result vector is read back once per heat."""
    dev = next(net.parameters()).device
    gt = batch["GT"].to(dev)
    with torch.no_grad():
        # an SR net samples from the dataset's LQ, a rescaling net from its own quantised LR^ (one tensor for the whole call)
        lq = batch["LQ"].to(dev) if net.cfg.sr else net.downscale(gt)[0]
    B = lq.shape[0]
    res: List[Dict] = [dict() for _ in range(B)]
    with torch.no_grad():
        for hi, heat in enumerate(heats):
            acc = lpips_map.sample_set(gt, normalize=True, capacity=n_sample)
            for s in range(n_sample):
                kw = {} if seed is None else {"seed": seed + 1000 * hi + s}
                acc.add(net(lr=lq, z=None, u=None, eps_std=heat, reverse=True, training=False, cache_cond=True, **kw))
            r = acc.result()
            lp = r["lpips"].double().cpu().tolist()                                # [M][B]
            best, local, score = (r[k].double().cpu().tolist() for k in ("global_best", "local_best", "score"))
            for b in range(B):
                mean = 0.0
                for s in range(n_sample):
                    mean += lp[s][b] / n_sample
                res[b][float(heat)] = {"lpips": mean, "lpips_best": best[b], "local_best": local[b], "score": score[b]}
    return res


def most_likely_samples(net, batch: Dict, heat, n_sample: int, seed: Optional[int] = None) -> Dict:
    """{"sr": [B,3,H,W], "logp": [B], "index": [B]}: per image of the batch the sample with the highest log-density
    log p(x | lr) among ``n_sample`` draws at temperature ``heat`` (a scalar or one value per image), its ``logp``
    (``HCFlowNet_SR.sample_with_logp``'s: nats, temperature 1, no Dirac term) and the number of the draw it came from (int64; the
    first of equal ones). Best-of-M without a ground truth, where ``evaluate_sample_set`` ranks by LPIPS against the GT. Draw s uses
    ``seed + s`` (``seed=None``: fresh seeds) and ``cache_cond=True``, so the LR-only features are computed once. Only the running
    best image and its ``logp`` live on the device: a row mask and ``torch.where`` per draw, no host read inside the loop. SR
    nets only (a rescaling net has no ``sample_with_logp``)."""
    if not net.cfg.sr:
        raise ValueError("most_likely_samples needs an SR net: a rescaling net's forward pass tracks no log-det, so its samples have no density")
    if n_sample < 1:
        raise ValueError("most_likely_samples: n_sample >= 1 expected, got %r" % (n_sample,))
    dev = next(net.parameters()).device
    lq = batch["LQ"].to(dev)
    best_sr = best_lp = best_ix = None
    with torch.no_grad():
        for s in range(n_sample):
            kw = {} if seed is None else {"seed": seed + s}
            sr, lp = net.sample_with_logp(lq, heat, cache_cond=True, **kw)
            if best_sr is None:
                best_sr, best_lp, best_ix = sr, lp, torch.zeros(lp.shape, dtype=torch.int64, device=lp.device)
                continue
            better = lp > best_lp
            best_sr = torch.where(better.view(-1, 1, 1, 1), sr, best_sr)
            best_lp = torch.where(better, lp, best_lp)
            best_ix = torch.where(better, torch.full_like(best_ix, s), best_ix)
    return {"sr": best_sr, "logp": best_lp, "index": best_ix}
