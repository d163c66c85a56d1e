#!/usr/bin/env python
"""Generates tests/golden/data_prep.npz: what the reference's GT_dataset (codes/data/GT_dataset.py:79-118, train phase) makes of
small seeded uint8 images -- data only.

Runs the reference's own data/util.py (imresize_np, augment) from /root/reference/codes (read-only, never copied) with a stand-in
`cv2` module (imported at module level only; nothing here calls it). `random.random` of that module is patched so that augment
takes each of the 8 flag combinations. The lines of __getitem__ between the two calls are index expressions, written out below
with their line numbers.

Contents:
  img{i}                uint8 HWC "BGR" source images (37x50, 45x61, 64x96)
  whole_s{s}_img{i}     float32 HWC: imresize_np(img / 255, 1 / s) of the whole image, s in 2, 3, 4, 8
  cases                 int32 [N, 9]: scale, image, top_lr, left_lr, lr_h, lr_w, hflip, vflip, rot90
  lq                    float32, flat: LQ of every case in case order, each CHW RGB [3, h, w] (after augment, BGR -> RGB,
                        HWC -> CHW; rot90 cases are square)
  gt255                 uint8, flat: GT of every case in case order, each CHW RGB [3, h s, w s], in a lossless code -- the
                        reference's float32 GT is EXACTLY gt255.astype(float32) / 255. (asserted bit for bit below, value by
                        value); as float32 the GT crops alone would be 240 KB of the file
                        (tests/data_oracle.py load_fixture_cases splits both)
Crops per scale: one case per flag combination. The four with rot90 are 6 x 6 (the smallest square crop of the tiny presets) at
the four corners of the LR grid [H // s, W // s]; the four without are 5 x 7 (non-square) at an interior position and at the
top-right, bottom-left and bottom-right corners.

    python tests/golden/make_data_golden.py
"""
import importlib.util as ilu
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/codes"
OUT = os.path.join(ROOT, "tests", "golden", "data_prep.npz")

SIZES = [(37, 50), (45, 61), (64, 96)]
IMAGE_OF_SCALE = {2: 0, 3: 1, 4: 0, 8: 2}


def import_reference_util():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = ilu.spec_from_file_location("ref_data_util", os.path.join(REF, "data", "util.py"))
    du = ilu.module_from_spec(spec)
    spec.loader.exec_module(du)
    return du


def positions(hl, wl, h, w):
    return [(0, 0), (0, wl - w), (hl - h, 0), (hl - h, wl - w), ((hl - h) // 2, (wl - w) // 2)]


def main():
    du = import_reference_util()
    rs = np.random.RandomState(20)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SIZES]
    out = {"img%d" % i: im for i, im in enumerate(imgs)}
    cases, gts, lqs = [], [], []
    for s in (2, 3, 4, 8):
        whole = {}
        for i, im in enumerate(imgs):
            img_GT = im.astype(np.float32) / 255.                       # read_img, data/util.py:91
            whole[i] = du.imresize_np(img_GT, 1 / s)                    # GT_dataset.py:82
            out["whole_s%d_img%d" % (s, i)] = whole[i]
        i = IMAGE_OF_SCALE[s]
        H, W, _ = imgs[i].shape
        img_GT = imgs[i].astype(np.float32) / 255.
        hl, wl = H // s, W // s
        plan = [(1, 6, 6, pos) for pos in positions(hl, wl, 6, 6)[:4]]
        p57 = positions(hl, wl, 5, 7)
        plan += [(0, 5, 7, pos) for pos in (p57[4], p57[1], p57[2], p57[3])]
        for j, (rot90, h, w, (top, left)) in enumerate(plan):
            hflip, vflip = j & 1, (j >> 1) & 1
            gt = img_GT[top * s:(top + h) * s, left * s:(left + w) * s, :]          # GT_dataset.py:93
            lq = whole[i][top:top + h, left:left + w, :]                            # :94
            draws = iter([0.0 if f else 0.9 for f in (hflip, vflip, rot90)])
            real_random = du.random.random
            du.random.random = lambda: next(draws)
            try:
                gt, lq = du.augment([gt, lq], True, True, "GTLQ")                   # :97
            finally:
                du.random.random = real_random
            gt, lq = (np.ascontiguousarray(np.transpose(t[:, :, [2, 1, 0]], (2, 0, 1))) for t in (gt, lq))      # :106-111
            assert gt.dtype == np.float32 and lq.dtype == np.float32
            code = np.rint(gt * 255.).astype(np.uint8)
            assert np.array_equal(code.astype(np.float32) / 255., gt)
            gts.append(code.ravel())
            lqs.append(lq.ravel())
            cases.append([s, i, top, left, h, w, hflip, vflip, rot90])
    out["cases"] = np.asarray(cases, dtype=np.int32)
    out["gt255"] = np.concatenate(gts)
    out["lq"] = np.concatenate(lqs)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
