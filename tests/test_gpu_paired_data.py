"""Paired image banks on the GPU (hcflow_amd.data's paired path, hcf_data_prepare_paired): parity with the reference fixture
(tests/golden/data_paired.npz) and with the numpy oracle (tests/paired_data_oracle.py) on crops that cross the kernel's 8 x 32
tiles. Every output value is one byte of a stored image divided by 255.f, so every comparison is bit equality: no tolerance.
"""
import os

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from hcflow_amd import data as D
from tests import paired_data_oracle as O
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def fixture_cases():
    return O.load_fixture_cases(os.path.join(GOLDEN, "data_paired.npz"))


def _row(c):
    return [c["image"], c["top"], c["left"], c["hflip"], c["vflip"], c["rot90"]]


def _fixture_bank(z, kind, scale, swap=False):
    """swap: the same pairs stored in the other channel order, declared as such -- the batches must not change."""
    pairs = O.fixture_pairs(z, kind, scale)
    order = "rgb" if kind == "pkl" else "bgr"
    if swap:
        pairs = [(np.ascontiguousarray(g[:, :, ::-1]), np.ascontiguousarray(l[:, :, ::-1])) for g, l in pairs]
        order = "bgr" if order == "rgb" else "rgb"
    return D.PairedBank([p[0] for p in pairs], [p[1] for p in pairs], DEV, order=order)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("kind,scale", [("pkl", 2), ("pkl", 4), ("pkl", 8), ("gtlq", 2), ("gtlq", 3), ("gtlq", 4), ("gtlq", 8)])
def test_parity_with_reference_fixture(fixture_cases, kind, scale, swap):
    """order="rgb" for the PKL pairs and order="bgr" for the GTLQ pairs as the reference stores them, and each again with the
    bytes stored in the other order."""
    z, cases = fixture_cases
    bank = _fixture_bank(z, kind, scale, swap)
    assert bank.scale == scale
    mine = [c for c in cases if c["scale"] == scale and c["bgr"] == (kind == "gtlq")]
    assert len(mine) >= 3
    for c in mine:
        got = D.prepare_paired_crops(bank, [_row(c)], c["h"], c["w"])
        assert np.array_equal(got["GT"][0].cpu().numpy(), c["gt"]), (c["mode"], _row(c))
        assert np.array_equal(got["LQ"][0].cpu().numpy(), c["lq"]), (c["mode"], _row(c))


def _positions(H, W, h, w):
    return [(0, 0), (0, W - w), (H - h, 0), (H - h, W - w), ((H - h) // 2, (W - w) // 2)]


@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_tile_crossing_crops_against_the_oracle(scale):
    """Partial tiles in x (5 x 7: one; 9 x 33: 2 x 2 with a 1-wide and a 1-high rest), in y and in both (17 x 40: 3 x 2), at the
    four corners and the centre of the LQ image, every flag triple the shape allows; pair e has an HR image that exceeds
    scale times its LQ image by e rows and scale - e columns, e = 1 .. scale - 1 (never read: the corners touch the last legal
    row and column)."""
    rs = np.random.RandomState(30 + scale)
    H, W = 20, 44
    lqs = [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(1, scale)]
    gts = [rs.randint(0, 256, size=(H * scale + e, W * scale + scale - e, 3)).astype(np.uint8) for e in range(1, scale)]
    bank = D.PairedBank(gts, lqs, DEV)
    n = 0
    for h, w in ((6, 6), (5, 7), (9, 33), (17, 40)):
        rows = []
        for top, left in _positions(H, W, h, w):
            for rot in ((0, 1) if h == w else (0,)):
                for vf in (0, 1):
                    for hf in (0, 1):
                        rows.append([n % len(lqs), top, left, hf, vf, rot])
                        n += 1
        assert len(rows) == (40 if h == w else 20)
        got = D.prepare_paired_crops(bank, rows, h, w)
        gt, lq = got["GT"].cpu().numpy(), got["LQ"].cpu().numpy()
        for j, r in enumerate(rows):
            want_gt, want_lq = O.sample(gts[r[0]], lqs[r[0]], scale, r[1], r[2], h, w, r[3], r[4], r[5])
            assert np.array_equal(gt[j], want_gt), ("GT", h, w, r)
            assert np.array_equal(lq[j], want_lq), ("LQ", h, w, r)


@pytest.mark.parametrize("scale", [2, 3, 4, 8])
def test_both_entries_copy_the_same_window(scale):
    """The GT of hcf_data_prepare_batch and of hcf_data_prepare_paired is the same copy, stated in prepare_batch_kernel with 8 rows
    in flight and as copy_window with 16: on the same HR images and crop rows both are the same bytes / 255.f through the same
    index map, so torch.equal.
    Two pairs, LQ 10 x 35 and HR exactly scale times that, the HR images as an ImageBank too; every origin of a 9 x 33 crop (over
    the 8-row and the 32-column tile edge) with both flips on and off, the same rows as one batch of 65 (the second launch of the
    chunk loop), every origin of a 6 x 6 crop under each of the eight flag triples. The paired LQ is the oracle's window."""
    rs = np.random.RandomState(50 + scale)
    H, W = 10, 35
    order = "bgr" if scale in (2, 4) else "rgb"
    lqs = [rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8) for _ in range(2)]
    gts = [rs.randint(0, 256, size=(H * scale, W * scale, 3)).astype(np.uint8) for _ in range(2)]
    pairs, single = D.PairedBank(gts, lqs, DEV, order=order), D.ImageBank(gts, DEV, order=order)
    wide = [[(t + l) % 2, t, l, hf, vf, 0] for t in range(H - 9 + 1) for l in range(W - 33 + 1) for vf in (0, 1) for hf in (0, 1)]
    batches = [(9, 33, wide), (9, 33, (wide * 3)[:_lib.DATA_LAUNCH_BATCH + 1])]
    batches += [(6, 6, [[(t + l) % 2, t, l, hf, vf, rot] for t in range(H - 6 + 1) for l in range(W - 6 + 1)])
                for rot in (0, 1) for vf in (0, 1) for hf in (0, 1)]
    assert len(wide) == 24 and len(batches[1][2]) == 65 and len(batches) == 10 and len(batches[2][2]) == 150
    for h, w, rows in batches:
        one = D.prepare_crops(single, rows, h, w, scale)
        two = D.prepare_paired_crops(pairs, rows, h, w)
        assert tuple(two["GT"].shape) == (len(rows), 3, h * scale, w * scale)
        assert torch.equal(one["GT"], two["GT"]), (h, w, rows[0][3:])
        lq = two["LQ"].cpu().numpy()
        for j, r in enumerate(rows):
            assert np.array_equal(lq[j], O.window(lqs[r[0]], r[1], r[2], h, w, r[3], r[4], r[5], bgr=order == "bgr")), (h, w, r)


@pytest.fixture(scope="module")
def small_bank():
    rs = np.random.RandomState(41)
    lqs = [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((12, 12), (9, 14), (16, 10))]
    gts = [rs.randint(0, 256, size=(l.shape[0] * 2 + i, l.shape[1] * 2 + 1, 3)).astype(np.uint8) for i, l in enumerate(lqs)]
    return D.PairedBank(gts, lqs, DEV), gts, lqs


def test_samples_do_not_depend_on_their_batch(small_bank):
    bank, _, _ = small_bank
    rows = [[0, 3, 6, 1, 0, 1], [1, 0, 0, 0, 1, 0], [2, 10, 4, 1, 1, 1], [0, 0, 2, 0, 0, 0], [2, 4, 4, 0, 1, 1]]
    got = D.prepare_paired_batch(bank, rows, 12)
    for i, r in enumerate(rows):
        one = D.prepare_paired_batch(bank, [r], 12)
        assert torch.equal(one["GT"][0], got["GT"][i]) and torch.equal(one["LQ"][0], got["LQ"][i]), i


def test_samples_do_not_depend_on_the_launch_split(small_bank):
    bank, _, _ = small_bank
    B = _lib.DATA_LAUNCH_BATCH + 1
    assert B == 65
    g = torch.Generator().manual_seed(3)
    rows = D.draw_paired_crops(bank, torch.randint(0, 3, (B,), generator=g), 12, "augment", generator=g)
    got = D.prepare_paired_batch(bank, rows, 12)
    for i in range(B):
        one = D.prepare_paired_batch(bank, rows[i:i + 1], 12)
        assert torch.equal(one["GT"][0], got["GT"][i]) and torch.equal(one["LQ"][0], got["LQ"][i]), i


def test_an_output_does_not_depend_on_the_other_being_made(small_bank):
    bank, _, _ = small_bank
    g = torch.Generator().manual_seed(4)
    rows = D.draw_paired_crops(bank, [0, 1, 2, 1, 0], 12, "pkl", generator=g)
    both = D.prepare_paired_batch(bank, rows, 12)
    only_gt = D.prepare_paired_batch(bank, rows, 12, out={"GT": torch.zeros(5, 3, 12, 12, device=DEV), "LQ": None})
    only_lq = D.prepare_paired_batch(bank, rows, 12, out={"GT": None, "LQ": torch.zeros(5, 3, 6, 6, device=DEV)})
    assert only_gt["LQ"] is None and only_lq["GT"] is None
    assert torch.equal(only_gt["GT"], both["GT"]) and torch.equal(only_lq["LQ"], both["LQ"])
    with pytest.raises(ValueError):
        D.prepare_paired_batch(bank, rows, 12, out={"GT": None, "LQ": None})


def test_whole_pair_is_the_oracle_and_crops_are_its_windows(small_bank):
    bank, gts, lqs = small_bank
    for i in range(3):
        whole = D.whole_pair(bank, i)
        want_gt, want_lq = O.whole(gts[i], lqs[i], 2)                       # mod-crop: HR is i rows and 1 column larger
        assert tuple(whole["GT"].shape) == (1,) + want_gt.shape
        assert np.array_equal(whole["GT"][0].cpu().numpy(), want_gt) and np.array_equal(whole["LQ"][0].cpu().numpy(), want_lq)
        H, W = bank.shape(i)
        rows = [[i, t, l, 0, 0, 0] for t in range(H - 5 + 1) for l in range(W - 7 + 1)]
        got = D.prepare_paired_crops(bank, rows, 5, 7)
        for k, s in (("LQ", 1), ("GT", 2)):
            ref = whole[k][0].unfold(1, 5 * s, s).unfold(2, 7 * s, s)       # [3, H-4, W-6, 5 s, 7 s]
            ref = ref.permute(1, 2, 0, 3, 4).reshape(len(rows), 3, 5 * s, 7 * s)
            assert torch.equal(got[k], ref), (i, k)
    with pytest.raises(ValueError):
        D.whole_pair(bank, 3)


def test_center_crops_are_the_fixture_validation_cases(fixture_cases):
    z, cases = fixture_cases
    mine = [c for c in cases if c["mode"] == O.MODE_PKL_CENTER]
    assert {c["scale"] for c in mine} == {2, 4, 8}
    for c in mine:
        bank = _fixture_bank(z, "pkl", c["scale"])
        rows = D.center_crops(bank, [c["image"]], c["h"] * c["scale"])
        assert rows.tolist() == [_row(c)]
        got = D.prepare_paired_batch(bank, rows, c["h"] * c["scale"])
        assert np.array_equal(got["GT"][0].cpu().numpy(), c["gt"]) and np.array_equal(got["LQ"][0].cpu().numpy(), c["lq"])


def test_out_reuse_allocates_nothing(small_bank):
    bank, _, _ = small_bank
    g = torch.Generator().manual_seed(5)
    out = {"GT": torch.empty(5, 3, 12, 12, device=DEV), "LQ": torch.empty(5, 3, 6, 6, device=DEV)}
    rows = [D.draw_paired_crops(bank, [0, 1, 2, 1, 0], 12, "pkl", generator=g) for _ in range(3)]
    fresh = D.prepare_paired_batch(bank, rows[2], 12)
    whole = {"GT": torch.empty(1, 3, 18, 28, device=DEV), "LQ": torch.empty(1, 3, 9, 14, device=DEV)}
    fresh_whole = D.whole_pair(bank, 1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for r in rows:
        o = D.prepare_paired_batch(bank, r, 12, out=out)
        assert o is out
        assert torch.cuda.memory_allocated() == before
    assert D.whole_pair(bank, 1, out=whole) is whole and torch.cuda.memory_allocated() == before
    assert torch.equal(out["GT"], fresh["GT"]) and torch.equal(out["LQ"], fresh["LQ"])
    assert torch.equal(whole["GT"], fresh_whole["GT"]) and torch.equal(whole["LQ"], fresh_whole["LQ"])
    with pytest.raises(ValueError):
        D.prepare_paired_batch(bank, rows[0][:4], 12, out=out)


def test_paired_loader_feeds_one_nll_step_of_the_tiny_sr_net():
    from hcflow_amd import HCFlowNet_SR, make_params, preset
    rs = np.random.RandomState(14)
    lqs = [rs.randint(0, 256, size=(16 + i, 24, 3)).astype(np.uint8) for i in range(9)]
    gts = [rs.randint(0, 256, size=(l.shape[0] * 4, 96, 3)).astype(np.uint8) for l in lqs]
    bank = D.PairedBank(gts, lqs, DEV, order="rgb", paths=[("gt_%d.npy" % i, "lq_%d.npy" % i) for i in range(9)])

    def loader(rank=0, world=1):
        return D.PairedBankLoader(bank, 4 // world, 48, "pkl", True, True, generator=torch.Generator().manual_seed(5),
                                  rank=rank, world=world, seed=2)
    batches = list(loader())
    assert len(loader()) == 2 and len(batches) == 2
    seen = [p for b in batches for p in b["GT_path"]]
    assert len(set(seen)) == 8 and set(seen) <= set(bank.paths)
    b = batches[0]
    assert tuple(b["GT"].shape) == (4, 3, 48, 48) and tuple(b["LQ"].shape) == (4, 3, 12, 12)
    assert b["LQ_path"] == [p.replace("gt_", "lq_") for p in b["GT_path"]]
    again = list(loader())
    assert again[1]["GT_path"] == batches[1]["GT_path"] and torch.equal(again[1]["LQ"], batches[1]["LQ"])
    halves = [next(iter(loader(r, 2))) for r in (0, 1)]                     # two ranks: disjoint images of the same epoch
    assert not set(halves[0]["GT_path"]) & set(halves[1]["GT_path"])
    # the LQ batch is the stored LQ data, not a resize of GT: sample 0 is a window of its LQ image
    i = int(b["LQ_path"][0][3:-4])
    win = torch.from_numpy(lqs[i]).permute(2, 0, 1).float().div(255.).to(DEV).unfold(1, 12, 1).unfold(2, 12, 1)      # divided on the host
    cand = win.permute(1, 2, 0, 3, 4).reshape(-1, 3, 12, 12)
    aug = [torch.rot90(c, k, (2, 3)) for c in (cand, cand.flip(3)) for k in (0, 1, 3)]      # np.flip(axis=2), then np.rot90(k)
    assert any(bool((t == b["LQ"][0]).flatten(1).all(1).any()) for t in aug)

    cfg = preset("SR_4X_tiny")
    net = HCFlowNet_SR(opt=cfg.to_opt(), step=0)
    net.load_state_dict(make_params(cfg, 11), strict=True)
    for m in net.modules():
        if "ActNorm" in type(m).__name__:
            m.inited = True
    net = net.to(DEV).train()
    _, nll = net(hr=b["GT"], lr=b["LQ"], reverse=False, noise=torch.rand(4, 3, 48, 48, device=DEV))
    assert bool(torch.isfinite(nll).all())
    nll.mean().backward()
    grads = [p.grad for p in net.parameters() if p.requires_grad]
    assert grads and all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
