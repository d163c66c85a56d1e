#!/usr/bin/env python
"""Generates tests/golden/data_draws.json: what hcflow_amd.data draws under fixed seeds and what the two C entries of
hcf_data.hip answer to inputs that break two rules at once -- recorded results only, no pixel data, no device.

    python tests/golden/make_data_draws.py            # run ONCE on the commit whose behaviour is to be held

tests/test_data_draws_cpu.py calls `record()` of this file on the tree under test and compares with the stored file, entry by
entry: the numbers come from the commit the file was written on (367b6cf, before the single and the paired path were folded
into shared pieces), never from the code under test.

Contents:
  draw_crops          {gate: table} for the four (use_flip, use_rot) gates, [B, 6] rows, and one table at x2
  draw_paired_crops   {rule/gate: table} for both rules and the four gates
  bank_loader         the first two batches of a BankLoader epoch: crop table (column 0 = the index order) and path lists
  paired_loader       the same for PairedBankLoader, {world/rank/epoch: batches}, world 1 and 2, epoch 0 and 1
  return_codes        {name: code} of hcf_data_prepare_batch / hcf_data_prepare_paired for the compound faults below
All banks are on "cpu": drawing and sharding need no device. The loaders run up to the point of the launch -- prepare_batch /
prepare_paired_batch of the module are replaced by a stand-in that keeps the crop table it is handed -- so the tables are the
ones the loader itself drew, from its own generator, after its own permutation. The C entries get null or made-up device
pointers: every refusal comes before any HIP call.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "data_draws.json")
GATES = [(True, True), (True, False), (False, True), (False, False)]


def _images(sizes):
    return [np.zeros((h, w, 3), dtype=np.uint8) for h, w in sizes]


def _paired_bank(D, lq_sizes, scale, **kw):
    return D.PairedBank(_images([(h * scale + 1, w * scale + 2) for h, w in lq_sizes]), _images(lq_sizes), "cpu", **kw)


def _batches(D, loader, name, count=2):
    """The first `count` batches of one epoch, the launch replaced: [{crops, GT_path, LQ_path}]."""
    tables, real = [], getattr(D, name)

    def stand_in(bank, crops, *args, **kw):
        tables.append(torch.as_tensor(crops).tolist())
        return {"GT": None, "LQ": None}
    setattr(D, name, stand_in)
    try:
        out = []
        for i, b in enumerate(loader):
            if i == count:
                break
            out.append({"crops": tables[i], "GT_path": b["GT_path"], "LQ_path": b["LQ_path"]})
    finally:
        setattr(D, name, real)
    return out


def draws(D):
    out = {"draw_crops": {}, "draw_paired_crops": {}, "paired_loader": {}}
    gen = lambda seed: torch.Generator().manual_seed(seed)                             # noqa: E731
    bank = D.ImageBank(_images(((37, 50), (45, 61), (64, 96))), "cpu")
    idx = [0, 1, 2, 2, 1, 0, 0, 1]
    for flip, rot in GATES:
        out["draw_crops"]["x4 flip=%d rot=%d" % (flip, rot)] = D.draw_crops(bank, idx, 24, 4, flip, rot, gen(11)).tolist()
    out["draw_crops"]["x2 flip=1 rot=1"] = D.draw_crops(bank, idx, 12, 2, True, True, gen(12)).tolist()
    pairs = _paired_bank(D, ((9, 12), (10, 10), (12, 9)), 4)
    for rule in ("augment", "pkl"):
        for flip, rot in GATES:
            out["draw_paired_crops"]["%s flip=%d rot=%d" % (rule, flip, rot)] = \
                D.draw_paired_crops(pairs, idx, 24, rule, flip, rot, gen(13)).tolist()

    nine = D.ImageBank(_images([(64 + 4 * i, 96) for i in range(9)]), "cpu", paths=["img_%d.png" % i for i in range(9)])
    out["bank_loader"] = _batches(D, D.BankLoader(nine, 4, 48, 4, generator=gen(5)), "prepare_batch")
    nine = _paired_bank(D, [(16 + i, 24) for i in range(9)], 4, paths=[("gt_%d.npy" % i, "lq_%d.npy" % i) for i in range(9)])
    for world in (1, 2):
        for rank in range(world):
            for epoch in (0, 1):
                rule = "pkl" if rank == 0 else "augment"
                loader = D.PairedBankLoader(nine, 4 // world, 48, rule, True, True, generator=gen(6 + rank), rank=rank, world=world,
                                            seed=2)
                loader.set_epoch(epoch)
                out["paired_loader"]["world=%d rank=%d epoch=%d" % (world, rank, epoch)] = \
                    {"shard": loader.shard().tolist(), "batches": _batches(D, loader, "prepare_paired_batch")}
    return out


# ---- the C entries: inputs that break two rules at once; which of the two is reported is the order of the checks ----
def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, 3))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(v):
    return C.c_void_p(v) if v else None         # made-up non-null device addresses: never dereferenced on a refusal


def call_batch(lib, images, crops, lr_h=6, lr_w=6, scale=4, bank_bytes=1 << 20, gt=0x2000, lq=0x3000):
    img = None if images is None else _table(images)
    crp = np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 6))
    return lib.hcf_data_prepare_batch(_dev(0x1000), bank_bytes, _ptr(img), 2 if img is None else img.shape[0], _ptr(crp), crp.shape[0],
                                      lr_h, lr_w, scale, 1, _dev(gt), _dev(lq), None)


def call_paired(lib, gt_images, lq_images, crops, lr_h=6, lr_w=6, scale=4, gt_bytes=1 << 20, lq_bytes=1 << 20, gt=0x2000, lq=0x3000):
    gi, li = (None if t is None else _table(t) for t in (gt_images, lq_images))
    crp = np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 6))
    n = next(t.shape[0] for t in (gi, li) if t is not None)
    return lib.hcf_data_prepare_paired(_dev(0x1000), gt_bytes, _ptr(gi), _dev(0x4000), lq_bytes, _ptr(li), n, _ptr(crp), crp.shape[0],
                                       lr_h, lr_w, scale, 1, _dev(gt), _dev(lq), None)


OK_ROW, BAD_FLAG, OUTSIDE, ROT = [0, 0, 0, 0, 0, 0], [0, 0, 0, 2, 0, 0], [0, 4, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1]
GOOD, SMALL, FAR = [0, 37, 50], [5552, 15, 50], [1 << 30, 37, 50]          # x4: fine / below 4 * scale / outside a 1 MiB bank
GT1, LQ1, GT_SHORT = [0, 37, 50], [0, 9, 12], [0, 35, 50]                  # x4 pair; an HR image below 4 x its LQ image


def return_codes(lib):
    b = lambda *a, **k: int(call_batch(lib, *a, **k))                                   # noqa: E731
    p = lambda *a, **k: int(call_paired(lib, *a, **k))                                  # noqa: E731
    return {
        "batch: image 0 too small, image 1 outside the bank": b([SMALL, FAR], [OK_ROW]),
        "batch: image 0 outside the bank, image 1 too small": b([FAR, SMALL], [OK_ROW]),
        "batch: image 0 too small AND outside the bank": b([[1 << 30, 15, 50]], [OK_ROW]),
        "batch: image 0 too small at a negative offset": b([[-16, 15, 50]], [OK_ROW]),
        "batch: image 0 fine, image 1 too small, bad crop": b([GOOD, SMALL], [OUTSIDE]),
        "batch: bad flag in record 0, crop outside in record 1": b([GOOD], [BAD_FLAG, OUTSIDE]),
        "batch: image index outside the table, image too small": b([SMALL], [[1, 0, 0, 0, 0, 0]]),
        "batch: rot90 on a non-square crop, image too small": b([SMALL], [ROT], lr_h=2, lr_w=3),
        "batch: scale 9, null table": b(None, [OK_ROW], scale=9),
        "batch: no output wanted, image too small": b([SMALL], [OK_ROW], gt=0, lq=0),
        "batch: lr_h beyond 2^20, image too small": b([SMALL], [OK_ROW], lr_h=(1 << 20) + 1),
        "batch: image 4 * scale - 1 wide at x8, crop outside": b([[0, 64, 31]], [OUTSIDE], scale=8),
        "batch: accepted, B = 0": b([GOOD, [5552, 16, 16]], np.zeros((0, 6))),
        "paired: HR below scale x LQ, crop outside": p([GT_SHORT], [LQ1], [OUTSIDE]),
        "paired: HR below scale x LQ, bad flag": p([GT_SHORT], [LQ1], [BAD_FLAG]),
        "paired: HR below scale x LQ, HR outside its bank": p([[1 << 30, 35, 50]], [LQ1], [OK_ROW]),
        "paired: HR below scale x LQ, LQ outside its bank": p([GT_SHORT], [[1 << 30, 9, 12]], [OK_ROW]),
        "paired: pair 0 HR below scale x LQ, pair 1 LQ outside its bank": p([GT_SHORT, GT1], [LQ1, [1 << 30, 9, 12]], [OK_ROW]),
        "paired: pair 0 HR below scale x LQ, pair 1 LQ of height 0": p([GT_SHORT, GT1], [LQ1, [336, 0, 12]], [OK_ROW]),
        "paired: bad flag in record 0, crop outside in record 1": p([GT1], [LQ1], [BAD_FLAG, OUTSIDE]),
        "paired: scale 9, null LQ table": p([GT1], None, [OK_ROW], scale=9),
        "paired: scale 9, null HR table": p(None, [LQ1], [OK_ROW], scale=9),
        "paired: no output wanted, HR below scale x LQ": p([GT_SHORT], [LQ1], [OK_ROW], gt=0, lq=0),
        "paired: HR image below 4 * scale is legal, crop outside": p([[0, 12, 12]], [[0, 3, 3]], [[0, 2, 0, 0, 0, 0]], lr_h=2, lr_w=2),
        "paired: accepted, LQ 1 x 1, B = 0": p([[0, 4, 4]], [[0, 1, 1]], np.zeros((0, 6))),
    }


def record():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    from hcflow_amd import _lib
    from hcflow_amd import data as D
    return dict(draws(D), return_codes=return_codes(_lib.load()))


if __name__ == "__main__":
    with open(OUT, "w") as f:
        json.dump(record(), f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))
