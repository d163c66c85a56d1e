"""numpy index-map restatement of the reference's paired training samples (codes/data/LRHR_PKL_dataset.py:96-135, 146-185;
GTLQnpy_dataset.py:42-78; GTLQx_dataset.py:82-122 with data/util.py's augment :116-135), the oracle of hcflow_amd.data's paired
path / hcf_data_prepare_paired: crop, then [:, ::-1], [::-1], transpose, then the channel order, then / 255.

Both images of a pair are data: the LQ window is read from the LQ image, never computed from the HR image. uint8 -> float is
exact in every mode -- float32(double(u) / 255.0) (PKL: float64 divide, then torch.Tensor) equals float32(u) / float32(255)
(GTLQ: read_img) for all 256 byte values (`conversions_agree`) -- so everything here compares bit for bit.
"""
import numpy as np

from tests.data_oracle import augment, to_chw      # the kernel's index map (data/util.py:122-129) and HWC -> CHW RGB, on HWC

# (f, k) of the PKL mode -- np.flip(axis=2) when f, then np.rot90(k, axes=(1, 2)) on CHW -- as (hflip, vflip, rot90)
PKL_FLAGS = {(0, 0): (0, 0, 0), (1, 0): (1, 0, 0), (0, 1): (1, 0, 1), (1, 1): (0, 0, 1), (0, 3): (0, 1, 1), (1, 3): (1, 1, 1)}

MODE_PKL_TRAIN, MODE_PKL_CENTER, MODE_GTLQ_TRAIN, MODE_GTLQ_WHOLE = 0, 1, 2, 3


def conversions_agree():
    u = np.arange(256, dtype=np.uint8)
    return np.array_equal((u / 255.0).astype(np.float32), u.astype(np.float32) / np.float32(255.))


def pkl_augment(img_chw, f, k):
    """CHW; LRHR_PKL_dataset.py:146-157 with its two draws given."""
    if f:
        img_chw = np.flip(img_chw, 2)
    return np.rot90(img_chw, k, axes=(1, 2))


def window(img_u8, top, left, h, w, hflip=0, vflip=0, rot90=0, bgr=True):
    """float32 CHW RGB of one window of an HWC uint8 image."""
    crop = img_u8[top:top + h, left:left + w, :]
    assert crop.shape[:2] == (h, w), "crop outside the image"
    return to_chw(augment(crop, hflip, vflip, rot90), bgr).astype(np.float32) / np.float32(255.)


def sample(gt_u8, lq_u8, scale, top_lr, left_lr, lr_h, lr_w, hflip=0, vflip=0, rot90=0, bgr=True):
    """(GT float32 [3, lr_h s, lr_w s], LQ float32 [3, lr_h, lr_w]) of one pair."""
    s = int(scale)
    return (window(gt_u8, top_lr * s, left_lr * s, lr_h * s, lr_w * s, hflip, vflip, rot90, bgr),
            window(lq_u8, top_lr, left_lr, lr_h, lr_w, hflip, vflip, rot90, bgr))


def whole(gt_u8, lq_u8, scale, bgr=True):
    """The validation pair: no crop, GT mod-cropped to scale times the LQ size (GTLQx_dataset.py:118-120)."""
    H, W, _ = lq_u8.shape
    return sample(gt_u8, lq_u8, scale, 0, 0, H, W, bgr=bgr)


def load_fixture_cases(path):
    """tests/golden/data_paired.npz (make_paired_golden.py) -> (npz, [dict(mode, scale, image, top, left, h, w, hflip, vflip,
    rot90, f, k, bgr, gt_src, lq_src, gt, lq)]): gt / lq = the reference's float32 outputs decoded from their lossless uint8
    codes; gt_src / lq_src = names of the pair's source arrays in the npz; f, k = the PKL mode's recorded draws (-1 elsewhere)."""
    z = np.load(path)
    cases, g0, l0 = [], 0, 0
    for row, (f, k) in zip(z["cases"], z["fk"]):
        mode, s, i, top, left, h, w, hf, vf, rot = (int(v) for v in row)
        oh, ow = (w, h) if rot else (h, w)
        n = 3 * h * w
        gt = z["gt255"][g0:g0 + n * s * s].reshape(3, oh * s, ow * s).astype(np.float32) / np.float32(255.)
        lq = z["lq255"][l0:l0 + n].reshape(3, oh, ow).astype(np.float32) / np.float32(255.)
        g0, l0 = g0 + n * s * s, l0 + n
        kind = "pkl" if mode in (MODE_PKL_TRAIN, MODE_PKL_CENTER) else "gtlq"
        cases.append(dict(mode=mode, scale=s, image=i, top=top, left=left, h=h, w=w, hflip=hf, vflip=vf, rot90=rot, f=int(f),
                          k=int(k), bgr=kind == "gtlq", gt_src="%s_s%d_gt%d" % (kind, s, i), lq_src="%s_s%d_lq%d" % (kind, s, i),
                          gt=gt, lq=lq))
    assert g0 == z["gt255"].size and l0 == z["lq255"].size
    return z, cases


def fixture_pairs(z, kind, scale):
    """[(gt_u8, lq_u8)] of one mode family ("pkl": RGB, "gtlq": BGR) and scale, in image order."""
    out, i = [], 0
    while "%s_s%d_gt%d" % (kind, scale, i) in z:
        out.append((z["%s_s%d_gt%d" % (kind, scale, i)], z["%s_s%d_lq%d" % (kind, scale, i)]))
        i += 1
    return out
