"""float64 restatement of the reference's training-sample pipeline (codes/data/GT_dataset.py:79-118 with data/util.py's
imresize_np :407-474 and augment :116-129), the oracle of hcflow_amd.data / hcf_data_prepare_batch.

For the integer factor 1 / scale the antialiased cubic weights of calculate_weights_indices (:283-335) do not depend on the
output pixel: u - left = 0.5 - 0.5 s - floor(0.5 - 2.5 s), P = 4 s + 2 taps, tap k of output o reads source index
o s + k + c0 with c0 = s - 1 + floor(0.5 - 2.5 s), reflected once at each border (the reference's symmetric copies).
Everything is float64 except the input conversion uint8 -> float32 / 255 (the reference's read_img), which is exact to restate.

`torch_pipeline` is the same pipeline in torch fp32 (tools/batch_prep_bench.py times it as the CPU figure).
"""
import math

import numpy as np


def cubic(x):
    ax = np.abs(x)
    return np.where(ax <= 1, 1.5 * ax ** 3 - 2.5 * ax ** 2 + 1,
                    np.where(ax <= 2, -0.5 * ax ** 3 + 2.5 * ax ** 2 - 4 * ax + 2, 0.0))


def tap_weights(scale):
    """(weights float64 [4 s + 2] summing to 1, c0)."""
    s = int(scale)
    fl = math.floor(0.5 - 2.5 * s)
    k = np.arange(4 * s + 2, dtype=np.float64)
    w = cubic((0.5 - 0.5 * s - fl - k) / s) / s
    return w / w.sum(), s - 1 + fl


def source_indices(n_in, n_out, scale):
    """int64 [n_out, P]: source index of every tap, reflected once at each border."""
    w, c0 = tap_weights(scale)
    i = np.arange(n_out)[:, None] * scale + np.arange(w.size)[None, :] + c0
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n_in, 2 * n_in - 1 - i, i)
    assert i.min() >= 0 and i.max() < n_in, "image smaller than one reflection reaches"
    return i


def imresize_down(img, scale):
    """imresize_np(img, 1 / scale) for HWC input, in the input's float type promoted to float64: H pass, then W pass on its result."""
    img = np.asarray(img, dtype=np.float64)
    H, W, _ = img.shape
    w, _ = tap_weights(scale)
    oh, ow = math.ceil(H / scale), math.ceil(W / scale)
    ih, iw = source_indices(H, oh, scale), source_indices(W, ow, scale)
    out1 = np.zeros((oh, W, img.shape[2]))
    for k in range(w.size):
        out1 += w[k] * img[ih[:, k]]
    out2 = np.zeros((oh, ow, img.shape[2]))
    for k in range(w.size):
        out2 += w[k] * out1[:, iw[:, k]]
    return out2


def augment(img, hflip, vflip, rot90):
    if hflip:
        img = img[:, ::-1, :]
    if vflip:
        img = img[::-1, :, :]
    if rot90:
        img = img.transpose(1, 0, 2)
    return img


def to_chw(img, bgr=True):
    if bgr:
        img = img[:, :, [2, 1, 0]]
    return np.ascontiguousarray(np.transpose(img, (2, 0, 1)))


def sample(img_u8, scale, top_lr, left_lr, lr_h, lr_w, hflip=0, vflip=0, rot90=0, bgr=True, lr_whole=None):
    """(GT float32 [3, lr_h s, lr_w s], LQ float64 [3, lr_h, lr_w]) of one training sample; lr_whole = imresize_down of the
    image when the caller has it already."""
    s = int(scale)
    img = img_u8.astype(np.float32) / 255.
    if lr_whole is None:
        lr_whole = imresize_down(img, s)
    gt = img[top_lr * s:(top_lr + lr_h) * s, left_lr * s:(left_lr + lr_w) * s, :]
    lq = lr_whole[top_lr:top_lr + lr_h, left_lr:left_lr + lr_w, :]
    assert gt.shape[:2] == (lr_h * s, lr_w * s) and lq.shape[:2] == (lr_h, lr_w), "crop outside the image"
    return to_chw(augment(gt, hflip, vflip, rot90), bgr), to_chw(augment(lq, hflip, vflip, rot90), bgr)


def torch_imresize_down(img, scale):
    """imresize_down on a torch HWC tensor, in its dtype."""
    import torch
    H, W, C = img.shape
    w, _ = tap_weights(scale)
    oh, ow = math.ceil(H / scale), math.ceil(W / scale)
    ih, iw = torch.from_numpy(source_indices(H, oh, scale)), torch.from_numpy(source_indices(W, ow, scale))
    out1 = torch.zeros(oh, W, C, dtype=img.dtype)
    for k in range(w.size):
        out1.add_(img[ih[:, k]], alpha=float(w[k]))
    out2 = torch.zeros(oh, ow, C, dtype=img.dtype)
    for k in range(w.size):
        out2.add_(out1[:, iw[:, k]], alpha=float(w[k]))
    return out2


def torch_pipeline(images_u8, crops, lr_size, scale, bgr=True):
    """The whole batch as the reference's dataset makes it, in torch fp32: per sample the whole-image resize, crop, augment,
    BGR -> RGB, HWC -> CHW. images_u8: list of torch uint8 HWC; crops: [B, 6] rows as hcflow_amd.data.draw_crops."""
    import torch
    s, n = int(scale), int(lr_size)
    gts, lqs = [], []
    for img_i, top, left, hf, vf, rot in (tuple(int(v) for v in r) for r in crops):
        img = images_u8[img_i].to(torch.float32) / 255.
        lr = torch_imresize_down(img, s)
        pair = [img[top * s:(top + n) * s, left * s:(left + n) * s], lr[top:top + n, left:left + n]]
        for j, t in enumerate(pair):
            if hf:
                t = t.flip(1)
            if vf:
                t = t.flip(0)
            if rot:
                t = t.transpose(0, 1)
            if bgr:
                t = t.flip(2)
            pair[j] = t.permute(2, 0, 1).contiguous()
        gts.append(pair[0])
        lqs.append(pair[1])
    return {"GT": torch.stack(gts), "LQ": torch.stack(lqs)}


def load_fixture_cases(path):
    """tests/golden/data_prep.npz (make_data_golden.py) -> (npz, [dict(scale, image, top, left, h, w, hflip, vflip, rot90, gt, lq)]):
    gt = the reference's float32 GT decoded from its lossless uint8 code, lq = the reference's float32 LQ."""
    z = np.load(path)
    cases, g0, l0 = [], 0, 0
    for row in z["cases"]:
        s, i, top, left, h, w, hf, vf, rot = (int(v) for v in row)
        oh, ow = (w, h) if rot else (h, w)
        n = 3 * h * w
        gt = z["gt255"][g0:g0 + n * s * s].reshape(3, oh * s, ow * s).astype(np.float32) / 255.
        lq = z["lq"][l0:l0 + n].reshape(3, oh, ow)
        g0, l0 = g0 + n * s * s, l0 + n
        cases.append(dict(scale=s, image=i, top=top, left=left, h=h, w=w, hflip=hf, vflip=vf, rot90=rot, gt=gt, lq=lq))
    assert g0 == z["gt255"].size and l0 == z["lq"].size
    return z, cases
