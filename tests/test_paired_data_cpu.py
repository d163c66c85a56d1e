"""Paired image banks, the parts that need no GPU: the numpy oracle (tests/paired_data_oracle.py) against the reference fixture
(tests/golden/data_paired.npz, make_paired_golden.py), the (f, k) -> flags table of the PKL mode, the crop draws, the loader's
sharding, and the launcher's argument checks (they come before any HIP call). Every comparison of pixel values is bit equality."""
import ctypes as C
import math
import os
import pickle

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd import data as D
from tests import paired_data_oracle as O
from tests.conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "data_paired.npz")
AUGMENT_TRIPLES = {(h, v, r) for h in (0, 1) for v in (0, 1) for r in (0, 1)}
PKL_TRIPLES = set(O.PKL_FLAGS.values())


@pytest.fixture(scope="module")
def fixture_cases():
    return O.load_fixture_cases(FIXTURE)


def test_byte_conversions_of_both_modes_agree():
    assert O.conversions_agree()


def test_oracle_matches_reference_samples(fixture_cases):
    z, cases = fixture_cases
    for n, c in enumerate(cases):
        gt, lq = O.sample(z[c["gt_src"]], z[c["lq_src"]], c["scale"], c["top"], c["left"], c["h"], c["w"], c["hflip"], c["vflip"],
                          c["rot90"], c["bgr"])
        assert gt.dtype == np.float32 and lq.dtype == np.float32
        assert np.array_equal(gt, c["gt"]) and np.array_equal(lq, c["lq"]), n


def test_fixture_covers_both_modes_and_their_flags(fixture_cases):
    z, cases = fixture_cases
    for s in (2, 4, 8):
        mine = [c for c in cases if c["mode"] == O.MODE_PKL_TRAIN and c["scale"] == s]
        assert {(c["f"], c["k"]) for c in mine} == set(O.PKL_FLAGS)
        assert all((c["hflip"], c["vflip"], c["rot90"]) == O.PKL_FLAGS[(c["f"], c["k"])] for c in mine)
        assert len([c for c in cases if c["mode"] == O.MODE_PKL_CENTER and c["scale"] == s]) == 1
    for s in (2, 3, 4):
        mine = [c for c in cases if c["mode"] == O.MODE_GTLQ_TRAIN and c["scale"] == s]
        assert {(c["hflip"], c["vflip"], c["rot90"]) for c in mine} == AUGMENT_TRIPLES
    for s in (2, 3, 4, 8):
        (gt, lq), = O.fixture_pairs(z, "gtlq", s)
        assert gt.shape[0] > s * lq.shape[0] and gt.shape[1] > s * lq.shape[1]          # the mod-crop case, both dimensions
        whole, = [c for c in cases if c["mode"] == O.MODE_GTLQ_WHOLE and c["scale"] == s]
        assert whole["gt"].shape == (3, lq.shape[0] * s, lq.shape[1] * s)


def test_whole_pair_oracle_mod_crops(fixture_cases):
    z, cases = fixture_cases
    for c in [c for c in cases if c["mode"] == O.MODE_GTLQ_WHOLE]:
        gt, lq = O.whole(z[c["gt_src"]], z[c["lq_src"]], c["scale"])
        assert np.array_equal(gt, c["gt"]) and np.array_equal(lq, c["lq"])


def test_pkl_flag_table_is_flip_then_rot90():
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, size=(5, 5, 3)).astype(np.uint8)                           # HWC
    assert D.PKL_FLAGS == O.PKL_FLAGS and len(O.PKL_FLAGS) == 6
    for (f, k), flags in O.PKL_FLAGS.items():
        ref = O.pkl_augment(np.transpose(img, (2, 0, 1)), f, k)                         # the reference works on CHW
        got = np.transpose(O.augment(img, *flags), (2, 0, 1))
        assert np.array_equal(ref, got), (f, k)
    assert (0, 1, 0) not in PKL_TRIPLES and (1, 1, 0) not in PKL_TRIPLES


# ---- PairedBank / draws ----
def _bank(lq_sizes=((9, 12),), scale=4, extra=(0, 0), order="bgr", **kw):
    rs = np.random.RandomState(3)
    lq = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in lq_sizes]
    gt = [rs.randint(0, 256, size=(h * scale + extra[0], w * scale + extra[1], 3)).astype(np.uint8) for h, w in lq_sizes]
    return D.PairedBank(gt, lq, "cpu", order=order, **kw), gt, lq


def test_paired_bank_layout():
    b, gt, lq = _bank(((9, 12), (5, 7), (8, 8)), scale=3, extra=(2, 1), paths=["a", ("g.npy", "l.npy"), "c"])
    assert len(b) == 3 and b.scale == 3 and b.nbytes == b.gt.data.numel() + b.lq.data.numel() and b.device.type == "cpu"
    assert b.shape(1) == (5, 7) and b.bgr
    assert b.paths == ["a", "g.npy", "c"] and b.lq_paths == ["a", "l.npy", "c"]
    for half, imgs in ((b.gt, gt), (b.lq, lq)):
        for i, im in enumerate(imgs):
            off, H, W = (int(v) for v in half.table[i])
            assert off % 16 == 0 and (H, W) == im.shape[:2]
            assert np.array_equal(half.data[off:off + im.size].numpy().reshape(im.shape), im)
    assert _bank()[0].paths == ["0"]                                                    # the PKL dataset's str(item)


def test_paired_bank_rejects_bad_pairs():
    z = lambda h, w: np.zeros((h, w, 3), dtype=np.uint8)                                # noqa: E731
    with pytest.raises(ValueError, match="pair 1"):
        D.PairedBank([z(16, 16), z(15, 16)], [z(4, 4), z(4, 4)], "cpu")                 # HR one row short
    with pytest.raises(ValueError, match="pair 1"):
        D.PairedBank([z(16, 16), z(16, 15)], [z(4, 4), z(4, 4)], "cpu")
    with pytest.raises(ValueError, match="pair 0"):
        D.PairedBank([z(4, 4)], [z(4, 4)], "cpu")                                       # scale 1
    with pytest.raises(ValueError, match="pair 0"):
        D.PairedBank([z(36, 36)], [z(4, 4)], "cpu")                                     # scale 9
    with pytest.raises(ValueError):
        D.PairedBank([z(16, 16)], [z(4, 4), z(4, 4)], "cpu")
    with pytest.raises(ValueError):
        D.PairedBank([z(16, 16)], [np.zeros((4, 4, 3), dtype=np.float32)], "cpu")
    with pytest.raises(ValueError):
        D.PairedBank([z(16, 16)], [z(4, 4)], "cpu", paths=["a", "b"])
    with pytest.raises(ValueError):
        D.PairedBank([z(16, 16)], [z(4, 4)], "cpu", order="gbr")
    D.PairedBank([z(16, 16), z(19, 17)], [z(4, 4), z(4, 4)], "cpu")                      # larger HR: legal


def test_from_pkl(tmp_path):
    _, gt, lq = _bank(((6, 6), (5, 8), (4, 4)), scale=2)
    paths = []
    for name, imgs in (("hr.pkl", gt), ("lr.pkl", lq), ("empty.pkl", []), ("dict.pkl", {"a": 1})):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            pickle.dump(imgs, f)
    b = D.PairedBank.from_pkl(paths[0], paths[1], "cpu")
    assert len(b) == 3 and b.scale == 2 and not b.bgr and b.shape(1) == (5, 8) and b.paths == ["0", "1", "2"]
    assert np.array_equal(b.lq.data[:lq[0].size].numpy().reshape(lq[0].shape), lq[0])
    assert len(D.PairedBank.from_pkl(paths[0], paths[1], "cpu", n_max=2)) == 2
    with pytest.raises(ValueError):
        D.PairedBank.from_pkl(paths[0], paths[2], "cpu")
    with pytest.raises(ValueError):
        D.PairedBank.from_pkl(paths[3], paths[1], "cpu")
    with pytest.raises(OSError):
        D.PairedBank.from_pkl(str(tmp_path / "missing.pkl"), paths[1], "cpu")


@pytest.mark.parametrize("rule", ["augment", "pkl"])
def test_draws_deterministic_valid_and_covering(rule):
    b, _, _ = _bank()                                                                   # LQ 9 x 12, crop 6 x 6: top 0 .. 3, left 0 .. 6
    idx = [0] * 512
    t1 = D.draw_paired_crops(b, idx, 24, rule, generator=torch.Generator().manual_seed(5))
    t2 = D.draw_paired_crops(b, idx, 24, rule, generator=torch.Generator().manual_seed(5))
    t3 = D.draw_paired_crops(b, idx, 24, rule, generator=torch.Generator().manual_seed(6))
    assert t1.dtype == torch.int32 and tuple(t1.shape) == (512, 6) and t1.device.type == "cpu"
    assert torch.equal(t1, t2) and not torch.equal(t1, t3)
    assert set(t1[:, 1].tolist()) == set(range(4)) and set(t1[:, 2].tolist()) == set(range(7))     # inside, both ends hit
    assert set(t1[:, 0].tolist()) == {0}
    triples = {tuple(r[3:].tolist()) for r in t1}
    assert triples == (AUGMENT_TRIPLES if rule == "augment" else PKL_TRIPLES)


def test_pkl_draws_are_uniform_over_the_six():
    """60 000 draws: each triple's count is Binomial(n, 1/6), so within 5 standard deviations of n / 6 (5.7e-7 per triple)."""
    b, _, _ = _bank()
    n = 60000
    t = D.draw_paired_crops(b, [0] * n, 24, "pkl", generator=torch.Generator().manual_seed(7))
    code = (t[:, 3] + 2 * t[:, 4] + 4 * t[:, 5]).to(torch.int64)
    counts = torch.bincount(code, minlength=8).tolist()
    bound = 5 * math.sqrt(n * (1 / 6) * (5 / 6))
    for h, v, r in AUGMENT_TRIPLES:
        c = counts[h + 2 * v + 4 * r]
        if (h, v, r) in PKL_TRIPLES:
            assert abs(c - n / 6) <= bound, ((h, v, r), c)
        else:
            assert c == 0, (h, v, r)


def test_draw_gates():
    b, _, _ = _bank()
    g = torch.Generator().manual_seed(8)
    for rule in ("augment", "pkl"):
        assert int(D.draw_paired_crops(b, [0] * 64, 24, rule, use_flip=False, use_rot=False, generator=g)[:, 3:].abs().sum()) == 0
    t = D.draw_paired_crops(b, [0] * 64, 24, "augment", use_flip=True, use_rot=False, generator=g)
    assert int(t[:, 4:].sum()) == 0 and 0 < int(t[:, 3].sum()) < 64
    t = D.draw_paired_crops(b, [0] * 64, 24, "augment", use_flip=False, use_rot=True, generator=g)
    assert int(t[:, 3].sum()) == 0 and 0 < int(t[:, 4].sum()) < 64 and 0 < int(t[:, 5].sum()) < 64
    t = D.draw_paired_crops(b, [0] * 64, 24, "pkl", use_flip=True, use_rot=False, generator=g)            # f alone: k = 0
    assert {tuple(r[3:].tolist()) for r in t} == {(0, 0, 0), (1, 0, 0)}
    t = D.draw_paired_crops(b, [0] * 64, 24, "pkl", use_flip=False, use_rot=True, generator=g)            # k alone: f = 0
    assert {tuple(r[3:].tolist()) for r in t} == {O.PKL_FLAGS[(0, k)] for k in (0, 1, 3)}


def test_draws_reject_what_cannot_be_cropped():
    b, _, _ = _bank()
    with pytest.raises(ValueError):
        D.draw_paired_crops(b, [0], 40, "pkl")               # 10 LQ rows of 9: the reference would return a short patch
    with pytest.raises(ValueError):
        D.draw_paired_crops(b, [1], 24, "pkl")
    with pytest.raises(ValueError):
        D.draw_paired_crops(b, [0], 26, "pkl")               # not a multiple of the scale
    with pytest.raises(ValueError):
        D.draw_paired_crops(b, [0], 24, "rot")


def test_center_crops_rows_and_errors():
    b, _, _ = _bank(((10, 10), (8, 8), (9, 12), (9, 9)), scale=4)
    assert D.center_crops(b, [0, 1], 24).tolist() == [[0, 2, 2, 0, 0, 0], [1, 1, 1, 0, 0, 0]]
    assert D.center_crops(b, [1], 32).tolist() == [[1, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError, match="pair 2"):
        D.center_crops(b, [2], 24)                           # not square
    with pytest.raises(ValueError, match="pair 3"):
        D.center_crops(b, [3], 24)                           # border 3 is odd
    with pytest.raises(ValueError):
        D.center_crops(b, [0], 48)                           # larger than the image
    with pytest.raises(ValueError):
        D.center_crops(b, [0], 26)
    with pytest.raises(ValueError):
        D.center_crops(b, [4], 24)
    big, _, _ = _bank(((10, 10),), scale=4, extra=(2, 2))
    with pytest.raises(ValueError, match="pair 0"):
        D.center_crops(big, [0], 24)                         # HR is not exactly 4 x LQ: the borders are not one window


# ---- sharding ----
@pytest.mark.parametrize("world", [1, 2, 3])
def test_loader_shards(world):
    b, _, _ = _bank(tuple((6, 6) for _ in range(11)), scale=2)               # 11 is a multiple of neither 2 nor 3
    loaders = [D.PairedBankLoader(b, 1, 8, "pkl", True, True, rank=r, world=world, seed=4) for r in range(world)]
    shards = [l.shard().tolist() for l in loaders]
    assert all(len(s) == 11 // world for s in shards) and all(len(l) == 11 // world for l in loaders)
    flat = [i for s in shards for i in s]
    assert len(set(flat)) == len(flat) and set(flat) <= set(range(11))
    assert [l.shard().tolist() for l in loaders] == shards                   # the same on every call of one epoch
    for l in loaders:
        l.set_epoch(1)
    again = [l.shard().tolist() for l in loaders]
    assert again != shards
    flat = [i for s in again for i in s]
    assert len(set(flat)) == len(flat)
    other_seed = D.PairedBankLoader(b, 1, 8, "pkl", True, True, rank=0, world=world, seed=5)        # seed + epoch: 5 + 0 = 4 + 1
    assert other_seed.shard().tolist() == again[0]


def test_loader_rejects_bad_geometry():
    b, _, _ = _bank(tuple((6, 6) for _ in range(5)), scale=2)
    with pytest.raises(ValueError):
        D.PairedBankLoader(b, 3, 8, "pkl", True, True, world=2)              # 2 images per rank
    with pytest.raises(ValueError):
        D.PairedBankLoader(b, 1, 8, "pkl", True, True, rank=2, world=2)
    with pytest.raises(ValueError):
        D.PairedBankLoader(b, 1, 8, "gt", True, True)
    with pytest.raises(ValueError):
        D.PairedBankLoader(b, 1, 9, "pkl", True, True)


# ---- hcf_data_prepare_paired: every rejection happens on the host, before any HIP call (fake device pointers, no device) ----
GT_IMG, LQ_IMG = [[0, 37, 50]], [[0, 9, 12]]             # x4; the HR image exceeds 36 x 48: legal


def _call(gt_images=GT_IMG, lq_images=LQ_IMG, crops=((0, 0, 0, 0, 0, 0),), lr_h=6, lr_w=6, scale=4, gt_bytes=None, lq_bytes=None,
          gt=0x2000, lq=0x3000, gt_bank=0x1000, lq_bank=0x4000, n_images=None, null_table=None):
    lib = _lib.load()
    gi = np.ascontiguousarray(np.asarray(gt_images, dtype=np.int64).reshape(-1, 3))
    li = np.ascontiguousarray(np.asarray(lq_images, dtype=np.int64).reshape(-1, 3))
    crp = np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 6))
    size = lambda t: int((t[:, 0] + 3 * t[:, 1] * t[:, 2]).max())                       # noqa: E731
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731  (fake non-null device addresses: never dereferenced on a refusal)
    tab = lambda name, t: None if null_table == name else t.ctypes.data_as(C.c_void_p)  # noqa: E731
    return lib.hcf_data_prepare_paired(p(gt_bank), size(gi) if gt_bytes is None else gt_bytes, tab("gt", gi),
                                       p(lq_bank), size(li) if lq_bytes is None else lq_bytes, tab("lq", li),
                                       gi.shape[0] if n_images is None else n_images, tab("crops", crp), crp.shape[0], lr_h, lr_w,
                                       scale, 1, p(gt), p(lq), None)


def test_symbol_is_bound():
    assert "hcf_data_prepare_paired" in _lib.SYMBOLS and len(_lib.load().hcf_data_prepare_paired.argtypes) == 16


def test_accepts_an_empty_batch_without_a_device():
    assert _call(crops=np.zeros((0, 6))) == 0


def test_rejects_null_pointers():
    assert _call(gt=0, lq=0) == -1
    assert _call(gt_bank=0) == -1
    assert _call(lq_bank=0) == -1
    for name in ("gt", "lq", "crops"):
        assert _call(null_table=name) == -1


@pytest.mark.parametrize("scale", [1, 9, 0, -4])
def test_rejects_scale(scale):
    assert _call([[0, 128, 128]], [[0, 8, 8]], scale=scale) == -1


def test_rejects_no_images():
    assert _call(n_images=0) == -1
    assert _call(n_images=-1) == -1


def test_rejects_offset_or_image_outside_its_bank():
    assert _call(gt_bytes=3 * 37 * 50 - 1) == -1
    assert _call(lq_bytes=3 * 9 * 12 - 1) == -1
    assert _call(gt_images=[[16, 37, 50]], gt_bytes=3 * 37 * 50 + 15) == -1
    assert _call(lq_images=[[16, 9, 12]], lq_bytes=3 * 9 * 12 + 15) == -1
    assert _call(gt_images=[[-16, 37, 50]], gt_bytes=1 << 20) == -1
    assert _call(lq_images=[[1 << 40, 9, 12]], lq_bytes=1 << 20) == -1
    assert _call(lq_images=[[0, 0, 12]], lq_bytes=1 << 20) == -1


def test_rejects_image_index_or_crop_outside_its_image():
    assert _call(crops=[[1, 0, 0, 0, 0, 0]]) == -1
    assert _call(crops=[[-1, 0, 0, 0, 0, 0]]) == -1
    assert _call(crops=[[0, 4, 0, 0, 0, 0]]) == -1           # rows 4 .. 9 of 9
    assert _call(crops=[[0, 0, 7, 0, 0, 0]]) == -1           # columns 7 .. 12 of 12
    assert _call(crops=[[0, -1, 0, 0, 0, 0]]) == -1
    assert _call(crops=[[0, 0, -1, 0, 0, 0]]) == -1
    assert _call(lr_h=10, lr_w=5) == -1
    assert _call(lr_h=0) == -1 and _call(lr_w=0) == -1
    assert _call(crops=[[0, 3, 6, 0, 0, 0], [0, 3, 7, 0, 0, 0]]) == -1       # the second record of two


def test_rejects_flags_other_than_0_1():
    for f in (3, 4, 5):
        for bad in (2, -1):
            row = [0, 0, 0, 0, 0, 0]
            row[f] = bad
            assert _call(crops=[row]) == -1


def test_rejects_rot90_on_non_square_crop():
    assert _call(crops=[[0, 0, 0, 0, 0, 1]], lr_h=5, lr_w=7) == -1


def test_rejects_hr_smaller_than_scale_times_lq():
    assert _call(gt_images=[[0, 35, 50]]) == -5
    assert _call(gt_images=[[0, 37, 47]]) == -5
    assert _call(gt_images=[[0, 37, 50], [5552, 36, 47]], lq_images=[[0, 9, 12], [336, 9, 12]]) == -5     # any pair of the table


def test_no_cpu_path():
    b, _, _ = _bank(((8, 8),), scale=2)
    with pytest.raises(_lib.HcfError):
        D.whole_pair(b, 0, out={"GT": torch.empty(1, 3, 16, 16), "LQ": torch.empty(1, 3, 8, 8)})
    with pytest.raises(_lib.HcfError):
        D.prepare_paired_batch(b, [[0, 0, 0, 0, 0, 0]], 8)
