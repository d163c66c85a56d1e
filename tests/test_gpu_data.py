"""Device-side training batches on the GPU (hcflow_amd.data, hcf_data_prepare_batch): parity with the reference fixture
(tests/golden/data_prep.npz), and the exact properties of the kernel -- a crop is the same window of the whole image bit for bit
(tile seams, border reflection), samples do not depend on their batch or launch, the augment is an index map.

LQ gate, per fixture case: max |gpu - oracle| <= 8 * e32, where the oracle is the float64 restatement tests/data_oracle.py and
e32 = max |reference - oracle| is the reference's own fp32 deviation on that case: both are fp32 evaluations of the same two
dot products (4 s live taps each) that differ in summation order and in the last bit of the weights. GT is bit-equal.
"""
import os

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd import data as D
from tests import data_oracle as O
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE_FACTOR = 8.0


@pytest.fixture(scope="module")
def fixture_cases():
    return O.load_fixture_cases(os.path.join(GOLDEN, "data_prep.npz"))


@pytest.fixture(scope="module")
def fixture_bank(fixture_cases):
    z, _ = fixture_cases
    return D.ImageBank([z["img%d" % i] for i in range(3)], DEV)


def _row(c):
    return [c["image"], c["top"], c["left"], c["hflip"], c["vflip"], c["rot90"]]


@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_parity_with_reference_fixture(fixture_cases, fixture_bank, scale):
    z, cases = fixture_cases
    mine = [c for c in cases if c["scale"] == scale]
    assert len(mine) == 8
    worst = 0.0
    for c in mine:
        got = D.prepare_crops(fixture_bank, [_row(c)], c["h"], c["w"], scale)
        gt, lq = got["GT"][0].cpu().numpy(), got["LQ"][0].cpu().numpy()
        _, lq64 = O.sample(z["img%d" % c["image"]], scale, c["top"], c["left"], c["h"], c["w"], c["hflip"], c["vflip"], c["rot90"])
        assert np.array_equal(gt, c["gt"]), _row(c)
        e32 = float(np.abs(c["lq"].astype(np.float64) - lq64).max())
        err = float(np.abs(lq.astype(np.float64) - lq64).max())
        worst = max(worst, err / (GATE_FACTOR * e32))
        print("data-parity x%d %s: e32 %.3e, gpu %.3e (%.3f of the gate)" % (scale, _row(c), e32, err, err / (GATE_FACTOR * e32)))
        assert err <= GATE_FACTOR * e32, _row(c)
    print("data-parity x%d: worst fraction of the gate %.3f" % (scale, worst))


@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_whole_image_against_reference(fixture_cases, scale):
    """The reference's whole-image imresize_np output of the 64 x 96 image. x3: 64 is no multiple, whole_image refuses it; the
    crop of all 21 x 32 LR pixels whose GT lies inside the image is the same window of the reference's 22 x 32 output."""
    z, _ = fixture_cases
    img = z["img2"]
    bank = D.ImageBank([img], DEV)
    ref = z["whole_s%d_img2" % scale][:64 // scale]
    if scale == 3:
        got = D.prepare_crops(bank, [[0, 0, 0, 0, 0, 0]], 21, 32, 3)
    else:
        got = D.whole_image(bank, 0, scale)
    f = img.astype(np.float32) / 255.
    lq64 = O.imresize_down(f, scale)[:ref.shape[0]]
    lq = got["LQ"][0].cpu().numpy()[::-1].transpose(1, 2, 0)            # CHW RGB -> HWC BGR
    gt = got["GT"][0].cpu().numpy()[::-1].transpose(1, 2, 0)
    assert np.array_equal(gt, f[:gt.shape[0]])
    e32 = float(np.abs(ref.astype(np.float64) - lq64).max())
    err = float(np.abs(lq.astype(np.float64) - lq64).max())
    print("data-whole x%d: e32 %.3e, gpu %.3e (%.3f of the gate)" % (scale, e32, err, err / (GATE_FACTOR * e32)))
    assert err <= GATE_FACTOR * e32


def _all_windows(h, w, ch, cw, image=0):
    return [[image, t, l, 0, 0, 0] for t in range(h - ch + 1) for l in range(w - cw + 1)]


@pytest.mark.parametrize("size,scale,crop_shapes", [
    ((64, 96), 2, [(6, 6), (5, 7), (10, 34)]),        # LR 32 x 48: 4 x 2 tiles of 8 x 32; 10 x 34 crops span tiles of their own
    ((57, 135), 3, [(6, 6), (11, 37)]),               # LR 19 x 45: 2 full + 1 partial tile row, 1 full + 1 partial tile column
    ((76, 140), 4, [(19, 35)]),                       # LR 19 x 35 (the whole image as a crop, through the batch entry)
])
def test_crop_is_the_window_of_the_whole_image(size, scale, crop_shapes):
    rs = np.random.RandomState(11)
    bank = D.ImageBank([rs.randint(0, 256, size=size + (3,)).astype(np.uint8)], DEV)
    whole = D.whole_image(bank, 0, scale)
    H, W = size[0] // scale, size[1] // scale
    for ch, cw in crop_shapes:
        rows = _all_windows(H, W, ch, cw)
        got = D.prepare_crops(bank, rows, ch, cw, scale)
        lq_ref = whole["LQ"][0].unfold(1, ch, 1).unfold(2, cw, 1)               # [3, H-ch+1, W-cw+1, ch, cw]
        lq_ref = lq_ref.permute(1, 2, 0, 3, 4).reshape(len(rows), 3, ch, cw)
        assert torch.equal(got["LQ"], lq_ref), (ch, cw)
        for n in (0, len(rows) // 2, len(rows) - 1):
            t, l = rows[n][1] * scale, rows[n][2] * scale
            assert torch.equal(got["GT"][n], whole["GT"][0, :, t:t + ch * scale, l:l + cw * scale])


def test_samples_do_not_depend_on_their_batch(fixture_bank):
    rows = [[0, 3, 6, 1, 0, 1], [1, 0, 0, 0, 1, 0], [2, 10, 18, 1, 1, 1], [0, 0, 2, 0, 0, 0], [2, 4, 4, 0, 1, 1]]
    got = D.prepare_batch(fixture_bank, rows, 24, 4)
    for i, r in enumerate(rows):
        one = D.prepare_batch(fixture_bank, [r], 24, 4)
        assert torch.equal(one["GT"][0], got["GT"][i]) and torch.equal(one["LQ"][0], got["LQ"][i]), i


def test_samples_do_not_depend_on_the_launch_split(fixture_bank):
    B = _lib.DATA_LAUNCH_BATCH + 1
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 3, (B,), generator=g)
    rows = D.draw_crops(fixture_bank, idx, 12, 2, generator=g)
    got = D.prepare_batch(fixture_bank, rows, 12, 2)
    for i in (0, 1, _lib.DATA_LAUNCH_BATCH - 1, _lib.DATA_LAUNCH_BATCH):
        one = D.prepare_batch(fixture_bank, rows[i:i + 1], 12, 2)
        assert torch.equal(one["GT"][0], got["GT"][i]) and torch.equal(one["LQ"][0], got["LQ"][i]), i
    head = D.prepare_batch(fixture_bank, rows[:_lib.DATA_LAUNCH_BATCH], 12, 2)
    assert torch.equal(head["GT"], got["GT"][:-1]) and torch.equal(head["LQ"], got["LQ"][:-1])


@pytest.mark.parametrize("lr_h,lr_w", [(6, 6), (5, 7), (9, 33)])
def test_flags_are_index_maps(lr_h, lr_w):
    rs = np.random.RandomState(12)
    bank = D.ImageBank([rs.randint(0, 256, size=(45, 140, 3)).astype(np.uint8)], DEV)
    plain = D.prepare_crops(bank, [[0, 1, 1, 0, 0, 0]], lr_h, lr_w, 4)
    combos = [(h, v, r) for r in ((0, 1) if lr_h == lr_w else (0,)) for v in (0, 1) for h in (0, 1)]
    got = D.prepare_crops(bank, [[0, 1, 1, h, v, r] for h, v, r in combos], lr_h, lr_w, 4)
    for i, (h, v, r) in enumerate(combos):
        for k in ("GT", "LQ"):
            t = plain[k][0]
            if h:
                t = t.flip(2)
            if v:
                t = t.flip(1)
            if r:
                t = t.transpose(1, 2)
            assert torch.equal(got[k][i], t), (k, h, v, r)


def test_rgb_bank_keeps_channel_order():
    rs = np.random.RandomState(13)
    img = rs.randint(0, 256, size=(32, 40, 3)).astype(np.uint8)
    a = D.prepare_crops(D.ImageBank([img], DEV, order="bgr"), [[0, 1, 2, 0, 0, 0]], 5, 7, 4)
    b = D.prepare_crops(D.ImageBank([np.ascontiguousarray(img[:, :, ::-1])], DEV, order="rgb"), [[0, 1, 2, 0, 0, 0]], 5, 7, 4)
    assert torch.equal(a["GT"], b["GT"]) and torch.equal(a["LQ"], b["LQ"])


def test_out_reuse_allocates_nothing(fixture_bank):
    g = torch.Generator().manual_seed(4)
    out = {"GT": torch.empty(5, 3, 24, 24, device=DEV), "LQ": torch.empty(5, 3, 6, 6, device=DEV)}
    rows = [D.draw_crops(fixture_bank, [0, 1, 2, 1, 0], 24, 4, generator=g) for _ in range(3)]
    fresh = D.prepare_batch(fixture_bank, rows[2], 24, 4)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for r in rows:
        o = D.prepare_batch(fixture_bank, r, 24, 4, out=out)
        assert o is out
        assert torch.cuda.memory_allocated() == before
    assert torch.equal(out["GT"], fresh["GT"]) and torch.equal(out["LQ"], fresh["LQ"])
    with pytest.raises(ValueError):
        D.prepare_batch(fixture_bank, rows[0][:4], 24, 4, out=out)


def test_bank_loader_feeds_the_tiny_sr_net():
    from hcflow_amd import HCFlowNet_SR, make_params, preset
    rs = np.random.RandomState(14)
    bank = D.ImageBank([rs.randint(0, 256, size=(64 + 4 * i, 96, 3)).astype(np.uint8) for i in range(9)], DEV,
                       paths=["img_%d.png" % i for i in range(9)])
    loader = D.BankLoader(bank, batch_size=4, gt_size=48, scale=4, generator=torch.Generator().manual_seed(5))
    batches = list(loader)
    assert len(loader) == 2 and len(batches) == 2
    seen = [p for b in batches for p in b["GT_path"]]
    assert len(set(seen)) == 8 and set(seen) <= set(bank.paths)
    b = batches[0]
    assert tuple(b["GT"].shape) == (4, 3, 48, 48) and tuple(b["LQ"].shape) == (4, 3, 12, 12) and b["LQ_path"] == b["GT_path"]
    assert float(b["GT"].min()) >= 0 and float(b["GT"].max()) <= 1
    again = list(D.BankLoader(bank, batch_size=4, gt_size=48, scale=4, generator=torch.Generator().manual_seed(5)))
    assert again[1]["GT_path"] == batches[1]["GT_path"] and torch.equal(again[1]["LQ"], batches[1]["LQ"])
    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(DEV).eval()
    with torch.no_grad():
        _, nll = net(hr=b["GT"], lr=b["LQ"], reverse=False, noise=torch.rand(4, 3, 48, 48, device=DEV))
    assert bool(torch.isfinite(nll).all())
