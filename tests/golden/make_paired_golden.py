#!/usr/bin/env python
"""Generates tests/golden/data_paired.npz: what the reference's paired datasets make of small seeded uint8 pairs -- data only.

    python tests/golden/make_paired_golden.py <reference>/codes

Runs the reference's own code from the given directory (read, never copied):
  * LRHR_PKLDataset (data/LRHR_PKL_dataset.py) itself, on an HR and an LR pickle written to a temp dir. Train phase: use_crop,
    use_flip and use_rot on, with np.random.randint and np.random.choice wrapped so that the draws of every item are recorded;
    items are taken until each of the six (f, k) has occurred, the first sample of each is kept. Validation phase:
    center_crop_hr_size.
  * For the GTLQ family, data/util.py's read_img_fromnpy and augment([gt, lq], True, True, "GTLQnpy") behind a stand-in `cv2`
    module (imported at module level only; nothing here calls it), `random.random` of that module patched so that augment takes
    each flag combination. The lines of __getitem__ around them (GTLQnpy_dataset.py:52-59, 71-76) and the validation mod-crop
    (GTLQx_dataset.py:118-120) are index expressions, written out below with their line numbers.

The LQ images are independent random bytes, not resized HR images: an implementation that recomputes LR from HR cannot pass. The
GTLQ HR images are larger than scale times their LQ images by 1 row and scale - 1 columns (the mod-crop case).

Contents:
  pkl_s{s}_gt{i}, pkl_s{s}_lq{i}      uint8 HWC RGB pairs of the PKL mode, s in 2, 4, 8, two pairs each (square, HR = s LQ)
  gtlq_s{s}_gt{i}, gtlq_s{s}_lq{i}    uint8 HWC "BGR" pairs of the GTLQ modes, s in 2, 3, 4, 8, one pair each
  cases   int32 [N, 10]: mode, scale, image, top_lr, left_lr, lr_h, lr_w, hflip, vflip, rot90
          mode 0 PKL train, 1 PKL center crop, 2 GTLQ train, 3 GTLQ whole pair (tests/paired_data_oracle.py MODE_*)
  fk      int32 [N, 2]: the recorded (f, k) of a PKL train case -- f: the flip was applied, k: of np.rot90 -- else (-1, -1);
          its flags in `cases` are PKL_FLAGS[(f, k)], so the oracle on them reproducing the output is the check of that table
  gt255, lq255   uint8, flat: GT / LQ of every case in case order, each CHW RGB, in a lossless code -- the reference's float32
          output is EXACTLY code.astype(float32) / 255. (asserted below, value by value)
"""
import importlib.util as ilu
import os
import pickle
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.paired_data_oracle import (MODE_GTLQ_TRAIN, MODE_GTLQ_WHOLE, MODE_PKL_CENTER, MODE_PKL_TRAIN,  # noqa: E402
                                      PKL_FLAGS)

OUT = os.path.join(ROOT, "tests", "golden", "data_paired.npz")

# PKL: scale -> (LQ sides of the two square pairs, train crop in LQ pixels, center crop in LQ pixels)
PKL = {2: ((10, 8), 6, 6), 4: ((10, 8), 4, 6), 8: ((6, 4), 2, 4)}
# GTLQ: scale -> (LQ size, square crop for rot90 cases, non-square crop, flag triples taken)
ALL8 = [(h, v, r) for r in (0, 1) for v in (0, 1) for h in (0, 1)]
GTLQ = {2: ((7, 9), 4, (3, 5), ALL8), 3: ((7, 9), 4, (3, 5), ALL8), 4: ((7, 9), 4, (3, 5), ALL8),
        8: ((5, 6), 3, (2, 4), [(1, 0, 0), (0, 1, 1)])}


def load(ref, rel, name):
    spec = ilu.spec_from_file_location(name, os.path.join(ref, rel))
    mod = ilu.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def encode(t):
    """float32 CHW -> its uint8 code, asserted lossless value by value."""
    a = np.asarray(t, dtype=np.float32)
    code = np.rint(a * 255.).astype(np.uint8)
    assert a.dtype == np.float32 and np.array_equal(code.astype(np.float32) / 255., a)
    return code


def positions(hl, wl, h, w):
    return [(0, 0), (0, wl - w), (hl - h, 0), (hl - h, wl - w), ((hl - h) // 2, (wl - w) // 2)]


class Recorder:
    """np.random.randint / np.random.choice, wrapped: every draw of the dataset is kept with what it was drawn from."""

    def __enter__(self):
        self.draws, self._randint, self._choice = [], np.random.randint, np.random.choice
        np.random.randint = lambda *a, **k: self._keep("randint", self._randint(*a, **k))
        np.random.choice = lambda a, *r, **k: self._keep(tuple(a), self._choice(a, *r, **k))
        return self

    def _keep(self, what, v):
        self.draws.append((what, v))
        return v

    def __exit__(self, *exc):
        np.random.randint, np.random.choice = self._randint, self._choice


def pkl_cases(ref, rs, out, rows):
    ds_mod = load(ref, "data/LRHR_PKL_dataset.py", "ref_lrhr_pkl")
    for s, (sides, n, n_center) in PKL.items():
        lqs = [rs.randint(0, 256, size=(m, m, 3)).astype(np.uint8) for m in sides]
        gts = [rs.randint(0, 256, size=(m * s, m * s, 3)).astype(np.uint8) for m in sides]
        for i in range(2):
            out["pkl_s%d_gt%d" % (s, i)], out["pkl_s%d_lq%d" % (s, i)] = gts[i], lqs[i]
        with tempfile.TemporaryDirectory() as tmp:
            paths = {}
            for name, imgs in (("hr", gts), ("lr", lqs)):
                paths[name] = os.path.join(tmp, name + ".pklv4")
                with open(paths[name], "wb") as f:
                    pickle.dump(imgs, f, protocol=4)
            opt = {"dataroot_GT": paths["hr"], "dataroot_LQ": paths["lr"], "dataroot_y_labels": None}
            train = ds_mod.LRHR_PKLDataset(dict(opt, GT_size=n * s, use_crop=True, use_flip=True, use_rot=True))
            val = ds_mod.LRHR_PKLDataset(dict(opt, center_crop_hr_size=n_center * s))
            np.random.seed(100 + s)
            seen, t = {}, 0
            while len(seen) < 6:
                item = t % 2
                t += 1
                assert t < 1000
                with Recorder() as rec:
                    smp = train[item]
                (w0, top), (w1, left), (w2, keep), (w3, k) = rec.draws                  # LRHR_PKL_dataset.py:166-167, 147, 154
                assert (w0, w1, w2, w3) == ("randint", "randint", (True, False), (0, 1, 3))
                f = 0 if keep else 1                                                    # :148: the flip happens when the draw is False
                if (f, int(k)) not in seen:
                    seen[(f, int(k))] = (item, int(top), int(left), smp)
            for (f, k), (item, top, left, smp) in sorted(seen.items()):
                rows.append(([MODE_PKL_TRAIN, s, item, top, left, n, n] + list(PKL_FLAGS[(f, k)]), (f, k),
                             encode(smp["GT"].numpy()), encode(smp["LQ"].numpy())))
            smp = val[0]
            b = (sides[0] - n_center) // 2                                              # :183-185
            assert b > 0 and tuple(smp["LQ"].shape) == (3, n_center, n_center)
            rows.append(([MODE_PKL_CENTER, s, 0, b, b, n_center, n_center, 0, 0, 0], (-1, -1),
                         encode(smp["GT"].numpy()), encode(smp["LQ"].numpy())))


def to_chw_rgb(img):
    img = img[:, :, [2, 1, 0]]                                                          # GTLQnpy_dataset.py:71-74
    return np.ascontiguousarray(np.transpose(img, (2, 0, 1)))                          # :75-76


def gtlq_cases(ref, rs, out, rows):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    du = load(ref, "data/util.py", "ref_data_util")
    for s, ((hl, wl), sq, (rh, rw), triples) in GTLQ.items():
        lq_u8 = rs.randint(0, 256, size=(hl, wl, 3)).astype(np.uint8)
        gt_u8 = rs.randint(0, 256, size=(hl * s + 1, wl * s + s - 1, 3)).astype(np.uint8)
        out["gtlq_s%d_gt0" % s], out["gtlq_s%d_lq0" % s] = gt_u8, lq_u8
        img_GT_whole = du.read_img_fromnpy(gt_u8)                                       # GTLQnpy_dataset.py:47
        img_LR_whole = du.read_img_fromnpy(lq_u8)                                       # :48
        psq, prect = positions(hl, wl, sq, sq), positions(hl, wl, rh, rw)
        for j, (hflip, vflip, rot90) in enumerate(triples):
            (h, w), (top, left) = ((sq, sq), psq[j % 4]) if rot90 else ((rh, rw), prect[(j + 1) % 5])
            assert h == w or not rot90
            gt_size_h, gt_size_w = h * s, w * s
            img_GT = img_GT_whole[top * s:top * s + gt_size_h, left * s:left * s + gt_size_w, :]          # :55-58
            img_LR = img_LR_whole[top:top + h, left:left + w, :]                                          # :59
            draws = iter([0.0 if f else 0.9 for f in (hflip, vflip, rot90)])
            real_random = du.random.random
            du.random.random = lambda: next(draws)
            try:
                img_GT, img_LR = du.augment([img_GT, img_LR], True, True, "GTLQnpy")                      # :62-63
            finally:
                du.random.random = real_random
            rows.append(([MODE_GTLQ_TRAIN, s, 0, top, left, h, w, hflip, vflip, rot90], (-1, -1),
                         encode(to_chw_rgb(img_GT)), encode(to_chw_rgb(img_LR))))
        img_GT, img_LR = to_chw_rgb(img_GT_whole), to_chw_rgb(img_LR_whole)             # GTLQx_dataset.py:110-115
        _, H, W = img_LR.shape                                                          # :119
        img_GT = img_GT[:, :H * s, :W * s]                                              # :120
        rows.append(([MODE_GTLQ_WHOLE, s, 0, 0, 0, hl, wl, 0, 0, 0], (-1, -1), encode(img_GT), encode(img_LR)))


def main():
    if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "data", "LRHR_PKL_dataset.py")):
        sys.exit(__doc__)
    ref = sys.argv[1]
    rs = np.random.RandomState(21)
    out, rows = {}, []
    pkl_cases(ref, rs, out, rows)
    gtlq_cases(ref, rs, out, rows)
    out["cases"] = np.asarray([r[0] for r in rows], dtype=np.int32)
    out["fk"] = np.asarray([r[1] for r in rows], dtype=np.int32)
    out["gt255"] = np.concatenate([r[2].ravel() for r in rows])
    out["lq255"] = np.concatenate([r[3].ravel() for r in rows])
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases, %d bytes" % (OUT, len(rows), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
