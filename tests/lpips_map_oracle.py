"""CPU restatement of the per-pixel LPIPS map and of the sample-set statistics of ``hcflow_amd.lpips.LPIPSMap``: the oracle of
tests/test_gpu_lpips_map.py, on top of tests/lpips_oracle.py (the AlexNet features and the state-dict keys are taken from there).

* layer maps: ``d_l[b, y, x] = sum_c w_lc (f0_c / (sqrt n0 + 1e-10) - f1_c / (sqrt n1 + 1e-10))^2``: ``lpips_oracle.lpips_alex``
  without the spatial mean;
* ``upsample``: PyTorch's bilinear resize with ``align_corners=False`` written out: source row of output row y on an h-row grid
  ``sy = max(0, (y + 0.5) h / H - 0.5)``, rows ``i0 = floor(sy)``, ``i1 = min(i0 + 1, h - 1)``, weight ``sy - i0``; columns alike
  (tests/test_lpips_map_cpu.py holds it to ``F.interpolate``);
* the map ``D = sum_l upsample(d_l)``, l = 0..4 in that order: the value of ``lpips.LPIPS(net='alex', spatial=True)``;
* ``set_stats``: ``map_mean[m, b] = mean_yx D_m[b]``, ``global_best[b] = min_m map_mean[m, b]``, ``best_map = min_m D_m`` per pixel,
  ``local_best[b] = mean_yx best_map[b]``, ``score = (global_best - local_best) / global_best`` (0 where ``global_best == 0``).

Everything runs in ``dtype``: float64 is the reference, float32 the same restatement at the kernels' precision (the measure of
what fp32 arithmetic alone costs: ``e32`` of the tests)."""
import torch
import torch.nn.functional as F

from tests import lpips_oracle as O


def alex_features(x, sd, dtype=torch.float64):
    """``lpips_oracle.alex_features`` in ``dtype`` (float64: that function itself)."""
    if dtype == torch.float64:
        return O.alex_features(x, sd)
    g = lambda k: sd[k].detach().to("cpu", dtype)
    w = [(g(k + ".weight"), g(k + ".bias")) for k in O.CONV_KEYS]
    h1 = F.relu(F.conv2d(x, *w[0], stride=4, padding=2))
    h2 = F.relu(F.conv2d(F.max_pool2d(h1, 3, 2), *w[1], padding=2))
    h3 = F.relu(F.conv2d(F.max_pool2d(h2, 3, 2), *w[2], padding=1))
    h4 = F.relu(F.conv2d(h3, *w[3], padding=1))
    h5 = F.relu(F.conv2d(h4, *w[4], padding=1))
    return [h1, h2, h3, h4, h5]


def layer_maps(in0, in1, sd, normalize=False, dtype=torch.float64):
    """The five per-pixel layer maps [B, h_l, w_l] for NCHW inputs in [-1, 1] (normalize: in [0, 1])."""
    x0, x1 = in0.detach().to("cpu", dtype), in1.detach().to("cpu", dtype)
    if normalize:
        x0, x1 = 2 * x0 - 1, 2 * x1 - 1
    shift = sd["scaling_layer.shift"].to("cpu", dtype)
    scale = sd["scaling_layer.scale"].to("cpu", dtype)
    f0 = alex_features((x0 - shift) / scale, sd, dtype)
    f1 = alex_features((x1 - shift) / scale, sd, dtype)
    maps = []
    for l in range(5):
        n0 = f0[l] / (f0[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        n1 = f1[l] / (f1[l].pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        lin = sd["lin%d.model.1.weight" % l].to("cpu", dtype)
        maps.append(F.conv2d((n0 - n1) ** 2, lin)[:, 0])
    return maps


def axis(n_out, n_in, dtype=torch.float64):
    """(i0, i1, weight of i1) of every output index of a bilinear resize n_in -> n_out, align_corners=False."""
    y = torch.arange(n_out, dtype=dtype)
    s = ((y + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0.to(dtype)


def upsample(d, H, W):
    """[B, h, w] -> [B, H, W] by the explicit index / weight formula."""
    r0, r1, ty = axis(H, d.shape[1], d.dtype)
    c0, c1, tx = axis(W, d.shape[2], d.dtype)
    ty, tx = ty[None, :, None], tx[None, None, :]
    rows = d[:, r0, :] * (1 - ty) + d[:, r1, :] * ty
    return rows[:, :, c0] * (1 - tx) + rows[:, :, c1] * tx


def lpips_map(in0, in1, sd, normalize=False, dtype=torch.float64):
    """D [B, H, W] in ``dtype``: the five upsampled layer maps added in layer order."""
    H, W = in0.shape[2:]
    D = None
    for d in layer_maps(in0, in1, sd, normalize, dtype):
        u = upsample(d, H, W)
        D = u if D is None else D + u
    return D


def set_stats(maps):
    """The sample-set statistics of the maps D_1..D_M ([B, H, W] each), in the maps' dtype."""
    Dm = torch.stack(maps)                                        # [M, B, H, W]
    map_mean = Dm.mean(dim=(2, 3))
    global_best, index = map_mean.min(dim=0)
    best_map = Dm.min(dim=0).values
    local_best = best_map.mean(dim=(1, 2))
    score = torch.where(global_best == 0, torch.zeros_like(global_best), (global_best - local_best) / global_best)
    return {"map_mean": map_mean, "global_best": global_best, "global_best_index": index, "best_map": best_map,
            "local_best": local_best, "score": score}
