"""CPU checks of the training criteria (hcflow_amd/losses.py, hcf_loss.hip): the float64 oracle the GPU tests use agrees with the
reference-generated fixture, every native entry refuses bad arguments before it touches a device, and the module surface fails
loudly off the GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from hcflow_amd import _lib
from tests import criteria_oracle as O
from tests.util import load_golden, t

GAN_TYPES = ["gan", "ragan", "lsgan", "wgan-gp"]
NEW = ["hcf_loss_pair_workspace", "hcf_loss_pair", "hcf_loss_pair_backward", "hcf_loss_sumsq_workspace", "hcf_loss_sumsq",
       "hcf_loss_sumsq_backward", "hcf_loss_gan", "hcf_loss_gan_backward"]


def close(have, want, rtol=1e-12):
    have = np.asarray(have.detach().numpy() if torch.is_tensor(have) else have, np.float64)
    want = np.asarray(want, np.float64)
    assert have.shape == want.shape, (have.shape, want.shape)
    assert np.abs(have - want).max() <= rtol * np.abs(want).max(), (np.abs(have - want).max(), np.abs(want).max())


def leaf(a):
    return t(a).double().requires_grad_(True)


def test_oracle_pair_criteria_match_the_reference_fixture():
    g = load_golden("criteria_ref")
    cases = {"l1": lambda a, b: O.pixel(a, b, "l1"), "mse": lambda a, b: O.pixel(a, b, "l2"),
             "rec_l2": lambda a, b: O.reconstruction(a, b, "l2"), "rec_l1": lambda a, b: O.reconstruction(a, b, "l1"),
             "rec_l1_eps": lambda a, b: O.reconstruction(a, b, "l1", eps=1e-3), "charb": lambda a, b: O.charbonnier(a, b)}
    for name, fn in cases.items():
        a, b = leaf(g["x"]), leaf(g["y"])
        v = fn(a, b)
        ga, gb = O.grads(v, a, b)
        close(v, g[name + "_val"])
        close(ga, g[name + "_gx"])
        close(gb, g[name + "_gy"])
    # the other reductions are the same sums, regrouped
    a, b = t(g["x"]), t(g["y"])
    close(O.pixel(a, b, "l1", "none").mean(), g["l1_val"])
    close(O.pixel(a, b, "l2", "sum") / a.numel(), g["mse_val"])
    close(O.reconstruction(a, b, "l1", reduction="none").mean(), g["rec_l1_val"])
    close(O.reconstruction(a, b, "l1", reduction="none").sum(), g["charb_val"])


def test_oracle_latent_term_matches_the_reference_fixture():
    g = load_golden("criteria_ref")
    zs = [leaf(g["z1"]), leaf(g["z2"]), leaf(g["z3"])]
    v = O.latent_l2(*zs[:2])
    close(v, g["lat2_val"])
    for have, k in zip(O.grads(v, *zs[:2]), ("lat2_g1", "lat2_g2")):
        close(have, g[k])
    v = O.latent_l2(*zs)
    close(v, g["lat3_val"])
    for have, k in zip(O.grads(v, *zs), ("lat3_g1", "lat3_g2", "lat3_g3")):
        close(have, g[k])


@pytest.mark.parametrize("gan_type", GAN_TYPES)
@pytest.mark.parametrize("s", ["v", "p"])
def test_oracle_gan_sequences_match_the_reference_fixture(s, gan_type):
    g = load_golden("criteria_ref")
    key = "%s_%s" % (s, gan_type.replace("-", ""))
    for tag, (rl, fl) in (("", (1.0, 0.0)), ("_smooth", (0.9, 0.1))):
        for real in (True, False):
            a = leaf(g[s + "_pr"])
            v = O.gan_term(a, real, gan_type, rl, fl)
            close(v, g["%s%s_fwd%d_val" % (key, tag, real)])
            close(O.grads(v, a)[0], g["%s%s_fwd%d_g" % (key, tag, real)])
    pf, pr = leaf(g[s + "_pf"]), leaf(g[s + "_pr"])
    v = O.gan_generator(pf, pr, gan_type)
    close(v, g[key + "_g_val"])
    close(O.grads(v, pf)[0], g[key + "_g_gpf"])
    pr, pf = leaf(g[s + "_pr"]), leaf(g[s + "_pf"])
    tot, logs = O.gan_discriminator(pr, pf, gan_type)
    close(logs, g[key + "_d_logs"])
    gpr, gpf = O.grads(tot, pr, pf)
    close(gpr, g[key + "_d_gpr"])
    close(gpf, g[key + "_d_gpf"])


def test_new_entries_are_bound():
    lib = _lib.load()
    for s in NEW:
        assert s in _lib.SYMBOLS and hasattr(lib, s)
    assert lib.hcf_loss_pair_workspace.restype is C.c_size_t and lib.hcf_loss_sumsq_workspace.restype is C.c_size_t


def _host():
    buf = (C.c_float * 64)()                          # never dereferenced: every call below is refused first
    return buf, C.cast(buf, C.c_void_p).value


def test_pair_entries_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    n = None
    buf, p = _host()

    def fwd(x=p, y=p, B=2, nn=8, kind=0, eps=0.0, out=p, rows=n, work=p, wb=1 << 16):
        return lib.hcf_loss_pair(x, y, B, nn, kind, eps, 1.0, 1.0, out, rows, work, wb, n)

    def bwd(x=p, y=p, B=2, nn=8, kind=0, eps=0.0, g=p, gs=0, gx=p, gy=n):
        return lib.hcf_loss_pair_backward(x, y, B, nn, kind, eps, 1.0, g, gs, gx, gy, n)
    assert fwd(x=n) == -1 and bwd(x=n) == -1                            # NULL tensors (a NULL y is zeros)
    assert fwd(out=n) == -1 and fwd(work=n) == -1 and bwd(g=n) == -1 and bwd(gx=n) == -1
    assert fwd(kind=-1) == -1 and fwd(kind=3) == -1 and bwd(kind=3) == -1
    assert fwd(B=0) == -1 and fwd(nn=0) == -1 and bwd(B=0) == -1 and bwd(nn=0) == -1
    assert fwd(eps=-1.0) == -1 and fwd(eps=float("nan")) == -1 and bwd(gs=2) == -1
    assert fwd(x=p + 2) == -1 and bwd(gx=p + 1) == -1 and fwd(work=p + 4) == -1      # 4-byte tensors, 8-byte workspace
    assert fwd(B=1 << 30, nn=1 << 30) == -5                            # > 2^40 elements
    assert fwd(B=(1 << 23) + 1, nn=4) == -5                            # > 2^23 blocks
    assert fwd(wb=8) == -7 and fwd(B=1, nn=1 << 22, wb=1024) == -7     # short workspace: HCF_ERR_NOMEM
    assert lib.hcf_loss_pair_workspace(0, 8) == 0 and lib.hcf_loss_pair_workspace(2, 0) == 0
    assert lib.hcf_loss_pair_workspace(2, 105) >= 4 * 8
    # the grid is capped: past 1024 blocks per sample the workspace stops growing
    assert lib.hcf_loss_pair_workspace(1, 1 << 22) == lib.hcf_loss_pair_workspace(1, 1 << 30) <= 1 << 14


def test_sumsq_entries_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    n = None
    buf, p = _host()
    tab = lambda k, v=p: (C.c_void_p * 9)(*([v] * k))
    lens = lambda k, v=16: (C.c_int64 * 9)(*([v] * k))

    def fwd(z=tab(2), ln=lens(2), k=2, out=p, work=p, wb=1 << 16):
        return lib.hcf_loss_sumsq(z, ln, k, out, work, wb, n)

    def bwd(z=tab(2), ln=lens(2), k=2, g=p, gz=tab(2)):
        return lib.hcf_loss_sumsq_backward(z, ln, k, g, gz, n)
    assert fwd(z=n) == -1 and fwd(ln=n) == -1 and fwd(out=n) == -1 and fwd(work=n) == -1
    assert fwd(z=tab(1)) == -1                                          # a NULL tensor in the table
    assert fwd(k=0) == -1 and fwd(z=tab(9), ln=lens(9), k=9) == -1 and bwd(z=tab(9), ln=lens(9), k=9, gz=tab(9)) == -1   # > 8 tensors
    assert fwd(ln=lens(2, 0)) == -1 and bwd(ln=lens(2, 0)) == -1
    assert fwd(ln=lens(2, 1 << 40)) == -5
    assert fwd(wb=8) == -7
    assert bwd(g=n) == -1 and bwd(gz=n) == -1 and bwd(gz=tab(0)) == -1 and bwd(z=n) == -1
    assert lib.hcf_loss_sumsq_workspace(lens(2), 2) >= 3 * 8 and lib.hcf_loss_sumsq_workspace(lens(2), 9) == 0
    assert lib.hcf_loss_sumsq_workspace(n, 2) == 0


def test_gan_entries_reject_bad_arguments_without_a_device():
    lib = _lib.load()
    n = None
    buf, p = _host()

    def fwd(a=p, na=4, b=p, nb=4, typ=0, rel=0, halve=0, out=p, ta=1.0):
        return lib.hcf_loss_gan(a, na, ta, b, nb, 0.0, typ, rel, halve, out, n)

    def bwd(a=p, na=4, b=p, nb=4, typ=0, rel=0, halve=0, g=p, ga=p, gb=n):
        return lib.hcf_loss_gan_backward(a, na, 1.0, b, nb, 0.0, typ, rel, halve, g, ga, gb, n)
    assert fwd(a=n) == -1 and fwd(out=n) == -1 and bwd(a=n) == -1 and bwd(g=n) == -1 and bwd(ga=n) == -1
    assert fwd(typ=-1) == -1 and fwd(typ=3) == -1 and bwd(typ=3) == -1
    assert fwd(na=0) == -1 and fwd(nb=-1) == -1 and fwd(b=n) == -1 and fwd(nb=0) == -1        # b and nb go together
    assert fwd(b=n, nb=0, rel=1) == -1 and fwd(rel=2) == -1 and fwd(halve=2) == -1 and fwd(ta=float("inf")) == -1
    assert bwd(b=n, nb=0, ga=n, gb=p) == -1                            # a gradient for a tensor that is not there
    assert fwd(na=(1 << 20) + 1) == -5 and fwd(nb=(1 << 20) + 1) == -5 and bwd(na=(1 << 20) + 1) == -5     # > 2^20 logits


def test_module_surface_fails_loudly_off_the_gpu():
    import hcflow_amd
    from hcflow_amd import losses
    for name in losses.__all__:
        assert getattr(hcflow_amd, name) is getattr(losses, name)
    a, b = torch.rand(2, 3, 4, 4), torch.rand(2, 3, 4, 4)
    for cri in (losses.PixelLoss("l1"), losses.PixelLoss("l2", "none"), losses.ReconstructionLoss("l1"), losses.CharbonnierLoss()):
        with pytest.raises(_lib.HcfError):
            cri(a, b)                                                   # a CPU tensor: no fallback
    with pytest.raises(_lib.HcfError, match="input is .* target is"):   # a shape mismatch, named before the device
        losses.PixelLoss()(a, b[:, :2])
    with pytest.raises(_lib.HcfError, match="float32 only"):
        losses.ReconstructionLoss()(a, b.double())
    with pytest.raises(_lib.HcfError, match="float32 only"):
        losses.GANLoss("lsgan")(torch.rand(2, 1).half(), True)
    with pytest.raises(_lib.HcfError):
        losses.latent_l2(a, b)
    with pytest.raises(_lib.HcfError):
        losses.latent_l2()
    with pytest.raises(_lib.HcfError):
        losses.latent_l2(*([a] * 9))
    with pytest.raises(_lib.HcfError):
        losses.GANLoss("gan")(torch.rand(2, 1), True)
    with pytest.raises(_lib.HcfError):
        losses.GANLoss("ragan").discriminator_loss(torch.rand(2, 1), torch.rand(2, 1))
    with pytest.raises(_lib.HcfError):
        losses.Quantization()(a)
    with pytest.raises(_lib.HcfError):
        losses.PixelLoss()(a, "b")
    with pytest.raises(_lib.HcfError):
        losses.finite_sum()
    with pytest.raises(_lib.HcfError):
        losses.finite_sum(torch.rand(2))
    with pytest.raises(NotImplementedError, match=r"GAN type \[hinge\] is not found"):
        losses.GANLoss("hinge")
    assert losses.GANLoss("RaGAN").gan_type == "ragan"                  # lower-cased, as the reference does
    for bad in (lambda: losses.PixelLoss("l1", "batch"), lambda: losses.ReconstructionLoss("l2", reduction="sum"),
                lambda: losses.ReconstructionLoss("huber")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(NotImplementedError):
        losses.PixelLoss("huber")
