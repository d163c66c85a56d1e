"""CPU checks of hcflow_amd.lpips (no GPU): the lpips.LPIPS(net='alex') state-dict table, loading the two offline weight files
(torchvision's AlexNet, lpips' alex.pth) into the right places, the loud failure off-GPU, and the exactness of conv1's
11x11 / stride-4 -> space-to-depth + 5x5 re-indexing that the HIP path relies on."""
import pytest
import torch
import torch.nn.functional as F

from hcflow_amd import _lib
from hcflow_amd.lpips import LPIPS, alex_conv1_as_s2d

# lpips.LPIPS(net='alex', version='0.1').state_dict() minus the `lins.K.` ModuleList aliases
LPIPS_ALEX_TABLE = [
    ("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1)),
    ("net.slice1.0.weight", (64, 3, 11, 11)), ("net.slice1.0.bias", (64,)),
    ("net.slice2.3.weight", (192, 64, 5, 5)), ("net.slice2.3.bias", (192,)),
    ("net.slice3.6.weight", (384, 192, 3, 3)), ("net.slice3.6.bias", (384,)),
    ("net.slice4.8.weight", (256, 384, 3, 3)), ("net.slice4.8.bias", (256,)),
    ("net.slice5.10.weight", (256, 256, 3, 3)), ("net.slice5.10.bias", (256,)),
    ("lin0.model.1.weight", (1, 64, 1, 1)), ("lin1.model.1.weight", (1, 192, 1, 1)), ("lin2.model.1.weight", (1, 384, 1, 1)),
    ("lin3.model.1.weight", (1, 256, 1, 1)), ("lin4.model.1.weight", (1, 256, 1, 1)),
]


def test_state_dict_table_matches_lpips_alex():
    m = LPIPS()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == LPIPS_ALEX_TABLE
    assert torch.allclose(m.scaling_layer.shift.flatten(), torch.tensor([-.030, -.088, -.188]))
    assert torch.allclose(m.scaling_layer.scale.flatten(), torch.tensor([.458, .448, .450]))
    assert not any(p.requires_grad for p in m.parameters())
    # seeded: two constructions agree, another seed differs
    a, b, c = LPIPS().state_dict(), LPIPS().state_dict(), LPIPS(seed=1).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["net.slice1.0.weight"], c["net.slice1.0.weight"])


def test_unsupported_variants_raise():
    for kw in ({"net": "vgg"}, {"version": "0.0"}, {"spatial": True}, {"lpips": False}):
        with pytest.raises(_lib.HcfError):
            LPIPS(**kw)


def _fake_files(seed=5):
    g = torch.Generator().manual_seed(seed)
    feats = {0: (64, 3, 11, 11), 3: (192, 64, 5, 5), 6: (384, 192, 3, 3), 8: (256, 384, 3, 3), 10: (256, 256, 3, 3)}
    tv = {}
    for i, s in feats.items():
        tv["features.%d.weight" % i] = torch.randn(*s, generator=g)
        tv["features.%d.bias" % i] = torch.randn(s[0], generator=g)
    tv["classifier.1.weight"] = torch.randn(8, 4, generator=g)       # ignored
    lin = {"lin%d.model.1.weight" % l: torch.rand(1, c, 1, 1, generator=g) for l, c in enumerate((64, 192, 384, 256, 256))}
    return tv, lin


def test_load_torchvision_alexnet_and_lpips_heads(tmp_path):
    tv, lin = _fake_files()
    m = LPIPS().load_pretrained(tv, lin)
    sd = m.state_dict()
    for s, i in enumerate((0, 3, 6, 8, 10), start=1):
        assert torch.equal(sd["net.slice%d.%d.weight" % (s, i)], tv["features.%d.weight" % i])
        assert torch.equal(sd["net.slice%d.%d.bias" % (s, i)], tv["features.%d.bias" % i])
    for k, v in lin.items():
        assert torch.equal(sd[k], v)
    # from local files, through the constructor
    torch.save(tv, tmp_path / "alexnet-owt-7be5be79.pth")
    torch.save(lin, tmp_path / "alex.pth")
    m2 = LPIPS(pnet_path=str(tmp_path / "alexnet-owt-7be5be79.pth"), model_path=str(tmp_path / "alex.pth"))
    assert all(torch.equal(sd[k], v) for k, v in m2.state_dict().items())


def test_lins_aliases_load():
    _, lin = _fake_files(7)
    src = LPIPS(seed=3).state_dict()
    for l in range(5):                      # an lpips.LPIPS state dict carries both spellings
        src["lins.%d.model.1.weight" % l] = src["lin%d.model.1.weight" % l]
    m = LPIPS()
    m.load_state_dict(src, strict=True)
    assert all(torch.equal(v, src[k]) for k, v in m.state_dict().items())
    only = {k.replace("lin%d." % l, "lins.%d." % l): v for l, (k, v) in enumerate(lin.items())}
    m = LPIPS().load_pretrained(None, only)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in lin.items())
    with pytest.raises(_lib.HcfError):
        LPIPS().load_pretrained(None, {"lin%d.model.1.weight" % l: torch.zeros(1, 3, 1, 1) for l in range(5)})


def test_forward_off_gpu_raises():
    m = LPIPS()
    x = torch.rand(1, 3, 64, 64)
    with pytest.raises(_lib.HcfError):
        m(x, x)


def _s2d_nchw(x):
    """[B, C, H, W] -> zero padded to multiples of 4 -> [B, 16 C, H/4, W/4], channel c * 16 + a * 4 + b."""
    B, Cc, H, W = x.shape
    x = F.pad(x, (0, (-W) % 4, 0, (-H) % 4))
    Hs, Ws = x.shape[2] // 4, x.shape[3] // 4
    return x.view(B, Cc, Hs, 4, Ws, 4).permute(0, 1, 3, 5, 2, 4).reshape(B, Cc * 16, Hs, Ws)


@pytest.mark.parametrize("H", [31, 32, 33, 34, 64, 100, 160])
def test_conv1_s2d_reindexing_is_exact(H):
    g = torch.Generator().manual_seed(H)
    for W in sorted({H, 31, 100}):
        x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(64, 3, 11, 11, generator=g, dtype=torch.float64)
        ref = F.conv2d(x, w, stride=4, padding=2)
        got = F.conv2d(_s2d_nchw(x), alex_conv1_as_s2d(w), padding=2)
        h1, w1 = ref.shape[2:]
        assert (h1, w1) == ((H - 7) // 4 + 1, (W - 7) // 4 + 1)
        assert got.shape[2] >= h1 and got.shape[3] >= w1
        assert float((got[:, :, :h1, :w1] - ref).abs().max()) <= 1e-12
