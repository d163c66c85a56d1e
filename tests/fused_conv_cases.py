"""The cases of tests/test_gpu_fused_convs.py, shared with tests/test_fused_convs_cpu.py: geometry, the launch each case must
select, its inputs and the float64 / float32 CPU evaluation of the composition the launch computes. No GPU, no shared library.

A row is what ``info`` reports: ("fcn12", pre) for the persistent kernel's two instantiations, or the nine template arguments
(NTB, VEC, UP, FUSE2, TAILC, TH, SCALED, K1, N16) of a ``kVariants`` row of hcf_conv_f16x3.hip.
"""
import zlib

import torch
import torch.nn.functional as F

AFFINE, SHIFT3 = 0, 1
CAP = 1e-5            # the gate 4 * max(e32, ec, FLOOR) must stay within this for every case
FLOOR = 1e-6
ABL_NO_WINO, ABL_NO_N16 = 256, 2048


def fuse2_row(th, up=0):
    return (2, 1, up, 1, 0, th, 0, 0, 0)


def tail_row(tailc, th, n16):
    return (1, 1, 0, 0, tailc, th, 0, 0, n16)


# every fused row of kVariants, and both instantiations of fcn12_kernel
ALL_ROWS = ({fuse2_row(8, 1), fuse2_row(4), fuse2_row(8)} |
            {tail_row(c, th, 1) for c in (8, 12) for th in (4, 8)} | {tail_row(c, th, 0) for c in (8, 12, 24) for th in (4, 8)} |
            {("fcn12", 0), ("fcn12", 1)})
assert len(ALL_ROWS) == 15


def _fcn(name, B, H, W, srcs, row, ups=None, pre=False, form=0):
    return dict(kind="fcn", name=name, B=B, H=H, W=W, srcs=list(srcs), ups=list(ups or [0] * len(srcs)), pre=pre, form=form,
                row=row, env={}, ablation=0)


FCN_CASES = [
    _fcn("one_tile", 1, 4, 32, [6], ("fcn12", 0)),                                   # exactly one fcn12 tile
    _fcn("ragged_pre", 2, 9, 33, [12], ("fcn12", 1), pre=True),                      # ragged in both directions
    _fcn("small", 1, 3, 5, [3], ("fcn12", 0)),                                       # smaller than a tile, channel stride 4
    _fcn("persistent_pre", 3, 131, 161, [16], ("fcn12", 1), pre=True),               # 594 tiles: more tiles than blocks
    _fcn("one_tile_direct", 1, 4, 32, [6], fuse2_row(4), form=1),
    _fcn("ragged_direct", 2, 9, 33, [12], fuse2_row(4), form=1),
    _fcn("small_direct", 1, 3, 5, [3], fuse2_row(4), form=1),
    _fcn("th8_direct", 3, 87, 97, [12], fuse2_row(8), form=1),                       # 8-row tiles chosen by the grid, ragged
    _fcn("two_sources", 2, 10, 12, [10, 128], fuse2_row(4)),                         # cat(z1, u): the persistent form declines
    _fcn("upsampled", 1, 16, 24, [6, 128], fuse2_row(8, 1), ups=[0, 1]),             # the UP row
]


def _tail(name, C, ns, mode, f_out, th, n16, B=2, H=9, W=33, mat=True, zpad=False, env=None, ablation=0):
    cm = 8 if C <= 8 else 12 if C <= 12 else 24
    return dict(kind="tail", name=name, B=B, H=H, W=W, C=C, ns=ns, mode=mode, f_out=f_out, hid=64, mat=mat, zpad=zpad,
                row=tail_row(cm, th, n16), env=dict(env or {}), ablation=ablation)


_TAIL_SHAPES = [   # (C, ns, mode, f_out, n16, mat)
    (6, 3, AFFINE, 6, 1, True),
    (12, 6, AFFINE, 12, 1, True),
    (12, 3, AFFINE, 18, 0, True),          # the natural non-N16 TAILC 12 row
    (24, 12, AFFINE, 24, 0, True),
    (21, 10, AFFINE, 22, 0, True),         # channel tails
    (12, 3, SHIFT3, 3, 1, False),          # Affine3shift's other half, no permutation
]
NO_TH4 = {"HCF_NO_TH4": "1"}
TAIL_CASES = []
for _th, _env in ((4, None), (8, NO_TH4)):
    for _i, (_C, _ns, _m, _f, _n16, _mat) in enumerate(_TAIL_SHAPES):
        TAIL_CASES.append(_tail("c%d_ns%d_m%d_th%d" % (_C, _ns, _m, _th), _C, _ns, _m, _f, _th, _n16, mat=_mat, env=_env,
                                zpad=(_th == 4 and _i < 2)))
    # the non-N16 rows of TAILC 8 and 12 (the ablation bit only changes the row chosen)
    for _C, _ns, _m, _f, _n16, _mat in _TAIL_SHAPES[:2]:
        TAIL_CASES.append(_tail("c%d_ns%d_no_n16_th%d" % (_C, _ns, _th), _C, _ns, _m, _f, _th, 0, env=_env, ablation=ABL_NO_N16))
TAIL_CASES += [
    _tail("c12_ns6_th8_by_grid", 12, 6, AFFINE, 12, 8, 1, B=3, H=87, W=97),
    _tail("c12_ns6_one_tile", 12, 6, AFFINE, 12, 4, 1, B=1, H=4, W=32),
    _tail("c6_ns3_small", 6, 3, AFFINE, 6, 4, 1, B=1, H=3, W=5),
]
CASES = FCN_CASES + TAIL_CASES
assert len({c["kind"] + c["name"] for c in CASES}) == len(CASES)


def case_id(c):
    return "%s-%s" % (c["kind"], c["name"])


def ru4(n):
    return (n + 3) & ~3


def plan_input(c):
    """The case as hcf_debug_conv_plan's in[40] (include/hcflow.h), with tC, w2 and the views as the per-op entry sets them:
    dense NHWC tensors of roundup4 channels, every window at channel 0."""
    v = [0] * 40
    fcn = c["kind"] == "fcn"
    srcs = list(zip(c["srcs"], c["ups"])) if fcn else [(c["hid"], 0)]
    v[0:6] = [0, 9, c["B"], c["H"], c["W"], len(srcs)]
    for i, (n, up) in enumerate(srcs):
        v[6 + 5 * i: 11 + 5 * i] = [n, ru4(n), 0, up, 1]
    cout = 64 if fcn else c["f_out"]
    v[21:25] = [cout, ru4(cout), 0, 1]
    v[31] = 0 if fcn else c["C"]
    v[32] = 7 if fcn else 0
    v[34] = 1 if fcn else 0
    return v


def takes_fcn12(c):
    """launch_fcn12's own conditions on a form-0 call of the per-op entry (one source of <= 16 channels, not upsampled)."""
    return c["kind"] == "fcn" and c["form"] == 0 and len(c["srcs"]) == 1 and c["srcs"][0] <= 16 and c["ups"][0] == 0


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(c):
    """float32 CPU tensors of the case (deterministic per case name)."""
    g = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) % (2 ** 31))
    B, H, W = c["B"], c["H"], c["W"]

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    if c["kind"] == "fcn":
        cin = sum(c["srcs"])
        d = dict(srcs=[rn(B, n, H >> u, W >> u) for n, u in zip(c["srcs"], c["ups"])],
                 w1=rn(64, cin, 3, 3) / (cin * 9) ** 0.5, bias1=rn(64) * 0.1, scale1=torch.exp(rn(64) * 0.1),
                 w2=rn(64, 64, 1, 1) / 4.0, bias2=rn(64) * 0.1, scale2=torch.exp(rn(64) * 0.1))
        d["pre"] = rn(B, 64, H, W) * 0.5 if c["pre"] else None
        return d
    C, hid, f_out = c["C"], c["hid"], c["f_out"]
    scale3 = torch.exp(rn(f_out) * 0.3)                       # non-trivial, different per channel
    d = dict(z=rn(B, C, H, W), h2=rn(B, hid, H, W).abs(),     # h2 follows a ReLU
             scale3=scale3,
             # h = (conv + bias3) * scale3 ~ 0.5 N(0, 1): hid * 9 terms of E[h2^2] = 1
             w3=rn(f_out, hid, 3, 3) * (0.5 / (hid * 9) ** 0.5) / scale3.view(-1, 1, 1, 1),
             bias3=rn(f_out) * 0.05 / scale3,
             mat=(torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64))[0] * 1.1).float() if c["mat"] else None,
             an_bias=rn(1, C, 1, 1) * 0.1, an_logs=rn(1, C, 1, 1) * 0.1)
    return d


# ------------------------------------------------------------------------------------------------------------ references
def _f16(x):
    return x.to(torch.float16).to(x.dtype)


def fcn_eval(c, d, dtype=torch.float64, drop=None):
    """out = relu(((W2 . relu(((conv3x3(cat(up(src_i)), w1) + pre) + bias1) * scale1)) + bias2) * scale2) in ``dtype``.
    drop: "w1" / "w2" / "x" / "h1" rounds that operand to float16 first (the f16 split with its lo term dropped)."""
    t = lambda v: v.to(dtype)
    x = torch.cat([F.interpolate(t(s), scale_factor=2 ** u, mode="nearest") if u else t(s) for s, u in zip(d["srcs"], c["ups"])], 1)
    w1, w2 = t(d["w1"]), t(d["w2"])
    x = _f16(x) if drop == "x" else x
    w1 = _f16(w1) if drop == "w1" else w1
    w2 = _f16(w2) if drop == "w2" else w2
    a = F.conv2d(x, w1, None, 1, 1)
    if d["pre"] is not None:
        a = a + t(d["pre"])
    h1 = F.relu((a + t(d["bias1"]).view(1, -1, 1, 1)) * t(d["scale1"]).view(1, -1, 1, 1))
    h1 = _f16(h1) if drop == "h1" else h1
    return F.relu((F.conv2d(h1, w2) + t(d["bias2"]).view(1, -1, 1, 1)) * t(d["scale2"]).view(1, -1, 1, 1))


FCN_DROPS = ("w1", "w2", "x", "h1")


def tail_eval(c, d, dtype=torch.float64, drop=None):
    """h = (conv3x3(h2, w3) + bias3) * scale3, then the inverse flow step on z (the expressions of test_step_affine /
    test_step_shift3_and_no_perm) in ``dtype``: (out_z, h). drop: "w3" / "h2" as fcn_eval."""
    t = lambda v: v.to(dtype)
    h2, w3 = t(d["h2"]), t(d["w3"])
    h2 = _f16(h2) if drop == "h2" else h2
    w3 = _f16(w3) if drop == "w3" else w3
    h = (F.conv2d(h2, w3, None, 1, 1) + t(d["bias3"]).view(1, -1, 1, 1)) * t(d["scale3"]).view(1, -1, 1, 1)
    z, ns = t(d["z"]), c["ns"]
    if c["mode"] == AFFINE:
        shift, scale = h[:, 0::2], h[:, 1::2]
        zc = torch.cat((z[:, :ns], z[:, ns:] * torch.exp(-(0.318 * torch.atan(2 * scale))) - shift), 1)
    else:
        zc = torch.cat((z[:, :3] - h, z[:, 3:]), 1)
    if d["mat"] is not None:
        winv = torch.inverse(d["mat"].double()).to(dtype)
        zc = F.conv2d(zc, winv.view(c["C"], c["C"], 1, 1))
    return zc * torch.exp(-t(d["an_logs"])) - t(d["an_bias"]), h


TAIL_DROPS = ("w3", "h2")


def err(got, ref64):
    """max |got - ref64| / max(1, max |ref64|)"""
    return float((got.double() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))


def zpad_of(out, n):
    """the first n channels of ``out`` zero-padded to 16"""
    p = torch.zeros(out.shape[0], 16, out.shape[2], out.shape[3], dtype=out.dtype)
    p[:, :n] = out[:, :n]
    return p
