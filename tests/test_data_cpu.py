"""Device-side training batches, the parts that need no GPU: the float64 oracle (tests/data_oracle.py) against the reference
fixture (tests/golden/data_prep.npz, make_data_golden.py), the launcher's argument checks (they come before any HIP call), the
crop sampler and the image bank."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd import data as D
from tests import data_oracle as O
from tests.conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "data_prep.npz")
LQ_TOL = 5e-7          # 4 fp32 ulp of 1.0; the reference's own fp32 pipeline is 1.2e-7 .. 1.4e-7 from the float64 oracle


@pytest.fixture(scope="module")
def fixture_cases():
    return O.load_fixture_cases(FIXTURE)


def test_oracle_matches_reference_whole_images(fixture_cases):
    z, _ = fixture_cases
    for s in (2, 3, 4, 8):
        for i in range(3):
            ref = z["whole_s%d_img%d" % (s, i)]
            got = O.imresize_down(z["img%d" % i].astype(np.float32) / 255., s)
            assert got.shape == ref.shape
            assert np.abs(got - ref).max() <= LQ_TOL, (s, i)


def test_oracle_matches_reference_samples(fixture_cases):
    z, cases = fixture_cases
    assert len(cases) == 32
    for s in (2, 3, 4, 8):      # all 8 flag combinations per scale
        assert len({(c["hflip"], c["vflip"], c["rot90"]) for c in cases if c["scale"] == s}) == 8
    for n, c in enumerate(cases):
        gt, lq = O.sample(z["img%d" % c["image"]], c["scale"], c["top"], c["left"], c["h"], c["w"], c["hflip"], c["vflip"], c["rot90"])
        assert gt.dtype == np.float32 and np.array_equal(gt, c["gt"]), n
        assert lq.shape == c["lq"].shape and np.abs(lq - c["lq"]).max() <= LQ_TOL, n


def test_torch_pipeline_is_the_oracle_in_fp32(fixture_cases):
    """The CPU figure of tools/batch_prep_bench.py times this restatement: it must be the same function."""
    z, cases = fixture_cases
    imgs = [torch.from_numpy(z["img%d" % i]) for i in range(3)]
    for c in [c for c in cases if c["rot90"]]:
        got = O.torch_pipeline(imgs, [[c["image"], c["top"], c["left"], c["hflip"], c["vflip"], 1]], c["h"], c["scale"])
        assert np.array_equal(got["GT"][0].numpy(), c["gt"])
        assert np.abs(got["LQ"][0].numpy() - c["lq"]).max() <= LQ_TOL


# ---- hcf_data_prepare_batch: every rejection happens on the host, before any HIP call (this machine has no device) ----
def _call(images, crops, lr_h=6, lr_w=6, scale=4, bank_bytes=None, gt=0x2000, lq=0x3000, bank=0x1000):
    lib = _lib.load()
    img = np.ascontiguousarray(np.asarray(images, dtype=np.int64).reshape(-1, 3))
    crp = np.ascontiguousarray(np.asarray(crops, dtype=np.int32).reshape(-1, 6))
    if bank_bytes is None:
        bank_bytes = int((img[:, 0] + 3 * img[:, 1] * img[:, 2]).max())
    p = lambda v: C.c_void_p(v) if v else None      # noqa: E731  (fake non-null device addresses: never dereferenced on a refusal)
    return lib.hcf_data_prepare_batch(p(bank), bank_bytes, img.ctypes.data_as(C.c_void_p), img.shape[0],
                                      crp.ctypes.data_as(C.c_void_p), crp.shape[0], lr_h, lr_w, scale, 1, p(gt), p(lq), None)


IMG = [[0, 37, 50]]             # LR grid at x4: 9 x 12


def test_rejects_crop_one_pixel_outside():
    assert _call(IMG, [[0, 4, 0, 0, 0, 0]]) == -1            # rows 4 .. 9 of 9
    assert _call(IMG, [[0, 0, 7, 0, 0, 0]]) == -1            # columns 7 .. 12 of 12
    assert _call(IMG, [[0, -1, 0, 0, 0, 0]]) == -1
    assert _call(IMG, [[0, 0, -1, 0, 0, 0]]) == -1
    assert _call(IMG, [[0, 0, 0, 0, 0, 0]], lr_h=10, lr_w=5) == -1


def test_rejects_bad_image_index():
    assert _call(IMG, [[1, 0, 0, 0, 0, 0]]) == -1
    assert _call(IMG, [[-1, 0, 0, 0, 0, 0]]) == -1


def test_rejects_offset_past_bank():
    assert _call(IMG, [[0, 0, 0, 0, 0, 0]], bank_bytes=3 * 37 * 50 - 1) == -1
    assert _call([[16, 37, 50]], [[0, 0, 0, 0, 0, 0]], bank_bytes=3 * 37 * 50 + 15) == -1
    assert _call([[-16, 37, 50]], [[0, 0, 0, 0, 0, 0]], bank_bytes=1 << 20) == -1
    assert _call([[1 << 40, 37, 50]], [[0, 0, 0, 0, 0, 0]], bank_bytes=1 << 20) == -1


@pytest.mark.parametrize("scale", [1, 9, 0, -4])
def test_rejects_scale(scale):
    assert _call([[0, 128, 128]], [[0, 0, 0, 0, 0, 0]], scale=scale) == -1


def test_rejects_rot90_on_non_square_crop():
    assert _call(IMG, [[0, 0, 0, 0, 0, 1]], lr_h=5, lr_w=7) == -1


def test_rejects_flags_other_than_0_1():
    for f in (3, 4, 5):
        row = [0, 0, 0, 0, 0, 0]
        row[f] = 2
        assert _call(IMG, [row]) == -1


def test_rejects_image_smaller_than_4_scale():
    assert _call([[0, 15, 50]], [[0, 0, 0, 0, 0, 0]], lr_h=2, lr_w=2) == -5
    assert _call([[0, 50, 15]], [[0, 0, 0, 0, 0, 0]], lr_h=2, lr_w=2) == -5
    assert _call([[0, 37, 50], [5552, 31, 64]], [[0, 0, 0, 0, 0, 0]], lr_h=2, lr_w=2, scale=8) == -5     # any image of the table


def test_rejects_null_pointers():
    ok = [[0, 0, 0, 0, 0, 0]]
    assert _call(IMG, ok, gt=0, lq=0) == -1
    assert _call(IMG, ok, bank=0) == -1
    lib = _lib.load()
    crp = np.zeros((1, 6), dtype=np.int32)
    img = np.asarray(IMG, dtype=np.int64)
    v = C.c_void_p
    assert lib.hcf_data_prepare_batch(v(0x1000), 5550, None, 1, crp.ctypes.data_as(v), 1, 6, 6, 4, 1, v(0x2000), v(0x3000), None) == -1
    assert lib.hcf_data_prepare_batch(v(0x1000), 5550, img.ctypes.data_as(v), 1, None, 1, 6, 6, 4, 1, v(0x2000), v(0x3000), None) == -1


def test_rejects_empty_geometry():
    ok = [[0, 0, 0, 0, 0, 0]]
    assert _call(IMG, ok, lr_h=0) == -1
    assert _call(IMG, ok, lr_w=0) == -1


# ---- ImageBank / draw_crops ----
def _bank(sizes=((37, 50),), device="cpu"):
    rs = np.random.RandomState(3)
    return D.ImageBank([rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in sizes], device)


def test_image_bank_layout():
    rs = np.random.RandomState(4)
    imgs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((37, 50), (45, 61), (5, 3))]
    b = D.ImageBank(imgs, "cpu")
    assert len(b) == 3 and b.nbytes == b.data.numel() and b.data.dtype == torch.uint8
    assert b.table.dtype == torch.int64 and tuple(b.table.shape) == (3, 3)
    end = 0
    for i, im in enumerate(imgs):
        off, H, W = (int(v) for v in b.table[i])
        assert off % 16 == 0 and off >= end and (H, W) == im.shape[:2]
        assert np.array_equal(b.data[off:off + im.size].numpy().reshape(im.shape), im)
        end = off + im.size
    assert end <= b.nbytes


def test_image_bank_rejects_other_formats():
    with pytest.raises(ValueError):
        D.ImageBank([np.zeros((8, 8, 3), dtype=np.float32)], "cpu")
    with pytest.raises(ValueError):
        D.ImageBank([np.zeros((8, 8, 1), dtype=np.uint8)], "cpu")
    with pytest.raises(ValueError):
        D.ImageBank([np.zeros((8, 8), dtype=np.uint8)], "cpu")
    with pytest.raises(ValueError):
        D.ImageBank([np.zeros((8, 8, 3), dtype=np.uint16)], "cpu")
    with pytest.raises(ValueError):
        D.ImageBank([], "cpu")


def test_draw_crops_deterministic_valid_and_covering():
    b = _bank()
    idx = [0] * 256
    t1 = D.draw_crops(b, idx, 24, 4, generator=torch.Generator().manual_seed(5))
    t2 = D.draw_crops(b, idx, 24, 4, generator=torch.Generator().manual_seed(5))
    t3 = D.draw_crops(b, idx, 24, 4, generator=torch.Generator().manual_seed(6))
    assert t1.dtype == torch.int32 and tuple(t1.shape) == (256, 6) and t1.device.type == "cpu"
    assert torch.equal(t1, t2) and not torch.equal(t1, t3)
    assert len({tuple(r[3:].tolist()) for r in t1}) == 8
    # every crop valid on the 37 x 50 image: LR grid 9 x 12, crop 6 x 6 -> top in 0 .. 3, left in 0 .. 6, each value drawn
    assert set(t1[:, 1].tolist()) == set(range(4)) and set(t1[:, 2].tolist()) == set(range(7))
    assert set(t1[:, 0].tolist()) == {0}
    for r in t1.tolist():
        assert r[1] >= 0 and r[2] >= 0 and (r[1] + 6) * 4 <= 37 and (r[2] + 6) * 4 <= 50


def test_draw_crops_flag_gates():
    b = _bank()
    g = torch.Generator().manual_seed(7)
    assert int(D.draw_crops(b, [0] * 64, 24, 4, use_flip=False, use_rot=False, generator=g)[:, 3:].abs().sum()) == 0
    t = D.draw_crops(b, [0] * 64, 24, 4, use_flip=True, use_rot=False, generator=g)
    assert int(t[:, 4:].sum()) == 0 and 0 < int(t[:, 3].sum()) < 64
    t = D.draw_crops(b, [0] * 64, 24, 4, use_flip=False, use_rot=True, generator=g)
    assert int(t[:, 3].sum()) == 0 and 0 < int(t[:, 4].sum()) < 64 and 0 < int(t[:, 5].sum()) < 64


def test_draw_crops_rejects_what_cannot_be_cropped():
    b = _bank()
    with pytest.raises(ValueError):
        D.draw_crops(b, [0], 40, 4)          # 10 LR rows of 9
    with pytest.raises(ValueError):
        D.draw_crops(b, [1], 24, 4)
    with pytest.raises(ValueError):
        D.draw_crops(b, [0], 26, 4)          # not a multiple of the scale
    with pytest.raises(ValueError):
        D.draw_crops(b, [0], 24, 12)


def test_whole_image_needs_multiples_of_scale():
    b = _bank(((37, 50), (64, 96)))
    with pytest.raises(ValueError):
        D.whole_image(b, 0, 4)
    with pytest.raises(ValueError):
        D.whole_image(b, 2, 4)


def test_no_cpu_path():
    b = _bank(((64, 96),))
    with pytest.raises(_lib.HcfError):
        D.whole_image(b, 0, 4, out={"GT": torch.empty(1, 3, 64, 96), "LQ": torch.empty(1, 3, 16, 24)})
