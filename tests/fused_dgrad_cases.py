"""The cases of tests/test_gpu_fused_dgrad.py, shared with tests/test_fused_dgrad_cpu.py: ONE launch of the fused data-gradient
form (ConvArgs::fb_y; hcf_op_conv2d_dgrad_fused_views) on channel windows of shared buffers, and its float64 reference. The arena,
the fills, the window helpers, err, FLOOR and CAP are those of tests/view_conv_cases.py (imported, not copied). No GPU, no shared
library.

A case: sources (windows of dL/dpre of the later convs), the weight [n, cin, k, k], ``y`` (a window of the producer's forward
output), the producer's activation, optionally its scale and the wish for the sum of dz * y, and the out window. Reference:

    d = conv2d(cat(srcs), w);  dz = d | where(y > 0, d, 0) | where(y >= 0, d, 0.2 d)   (tests/train_glue_ref.py::epi_closed)
    out = dpre = dz * scale;   sum_pre[c] = sum dpre;   sum_zy[c] = zy_mult * sum dz * y

Plants: in every relu / lrelu case 16 values of ``y`` are exactly 0.0 and 16 exactly -0.0, at places where |d| >= 1e-2 max |d|
(the CPU test asks for >= 1e-3): they separate ``>=`` from ``>``.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

from tests import view_conv_cases as VC

CAP, FLOOR, ABL_NO_WINO = VC.CAP, VC.FLOOR, VC.ABL_NO_WINO
SWITCHES = ("HCF_NO_DG_TH4", "HCF_NO_DG_STRIP", "HCF_NO_K1", "HCF_WINO_REV")
NPLANT = 16
PRESETS = {"small": 0.0, "big": 1.0e6}       # fb_max2 before the launch: below everything, above every |dpre| and |source|
NCU = 256                                    # persistent blocks of a Winograd launch on an MI355X


def wino_units(B, H, W):
    """units of 16 x 32 pixels the 32-channel Winograd kernel walks (wino_units(B, H, W, 1) of hcf_conv_wino.hip)"""
    return B * ((W + 31) // 32) * ((H + 15) // 16)


def scaled_rows(B, H, W, env):
    """(rows of partial sums = grid, tile height, strip_w) of the scaled f16x3 kernel: conv_f16x3_scaled_blocks"""
    sw = 0 if "HCF_NO_DG_STRIP" in env else VC.strip_width(B, W)
    row_tiles = (B * (W + 1) + 31) // 32 if sw else B * ((W + 31) // 32)
    th = 4 if "HCF_NO_DG_TH4" not in env and row_tiles * ((H + 3) // 4) <= 256 else 8
    return row_tiles * ((H + th - 1) // th), th, sw


XIN, GROW = VC.XIN, VC.GROW
_GB = {"xin": (64, 0, 0), "grow": (128, 0, 0), "Y": (64, 0, 0)}      # a dense block's input, its growth buffer, the producer's output


def _case(name, kernel, bufs=_GB, srcs=(XIN, GROW), out=("grow", 64, 32, 0), y=("Y", 16, 32, 0), act="lrelu", scale=False, zy=False,
          zy_mult=1.0, k=3, env=None, B=2, H=9, W=33, zero_src=False, rev0=True):
    """kernel: "f16x3" (Winograd ablated, bit 256, unless ``abl`` is cleared below) or "wino"; rev0: run under HCF_WINO_REV=0"""
    env = dict(env or {})
    if kernel == "wino" and rev0:
        env["HCF_WINO_REV"] = "0"
    n = out[2]
    c = dict(kind="fdg", name=name, kernel=kernel, B=B, H=H, W=W, k=k, bufs=dict(bufs), srcs=list(srcs), out=out, y=y, act=act,
             scale=scale, zy=zy, zy_mult=zy_mult, env=env, abl=ABL_NO_WINO if kernel == "f16x3" else 0, zero_src=zero_src)
    if kernel == "f16x3":
        rows, th, sw = scaled_rows(B, H, W, env)
        c.update(row=VC.f16_row((n + 31) // 32, 1, 0, th, scaled=1, k1=int(k == 1)), vec_epi=1, strip_w=sw, rows=rows, units=0)
    else:
        u = wino_units(B, H, W)
        c.update(row=None, vec_epi=0, strip_w=0, rows=min(u, NCU), units=u)
    return c


CASES = [
    _case("direct_n32_th4", "f16x3"),
    _case("direct_n32_th8", "f16x3", env=VC.NO_DG_TH4),
    # 64 output channels: the fused Winograd form refuses (ntile_n != 1) without any ablation
    dict(_case("direct_n64", "f16x3", out=("grow", 64, 64, 0), y=("Y", 16, 64, 0), bufs=dict(_GB, Y=(96, 0, 0)), act="relu"), abl=0),
    _case("direct_scale_zy", "f16x3", act="none", scale=True, zy=True, zy_mult=3.0),
    _case("direct_scale_zy_relu", "f16x3", act="relu", scale=True, zy=True, zy_mult=3.0),
    # the FCN conv2 form: a 1x1 data gradient completes dL/dy of conv1 (relu, learned scale)
    _case("direct_scale_zy_k1", "f16x3", srcs=(GROW,), act="relu", scale=True, zy=True, zy_mult=3.0, k=1),
    # whole quads, no whole tile, live channels behind the window: ``c4 < n4`` of the fused branch, ``tid < n`` of the row store
    _case("direct_n24", "f16x3", bufs=dict(_GB, o=(64, 0, 0)), out=("o", 8, 24, 0), y=("Y", 16, 24, 0)),
    _case("direct_strip", "f16x3", B=3, W=20),
    _case("direct_nostrip", "f16x3", B=1),
    _case("direct_zero_src", "f16x3", zero_src=True),
    _case("wino_ragged", "wino"),
    _case("wino_ragged_17x65", "wino", H=17, W=65),
    # (no engine launch: the gather convs' producers are leaky; the kernel's relu branch all the same)
    _case("wino_ragged_relu", "wino", act="relu"),
    _case("wino_zero_src", "wino", zero_src=True),
    # 384 units on 256 persistent blocks: the only case in which a block adds a second unit's sums to its slot; narrow buffers
    # with live channels on one side of every window keep the arena at 72 MB
    _case("wino_multi_unit", "wino", bufs={"g": (20, 0, 0), "o": (36, 0, 0), "Y": (36, 0, 0)}, srcs=(("g", 4, 16, 0),), out=("o", 4, 32, 0),
          y=("Y", 0, 32, 0), B=8, H=48, W=512),
]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the same launches in the default ALTERNATING walk direction (two consecutive launches: one forward, one backward)
ALTERNATING = [dict(BY_NAME[n], name=n + "_alt", env={}) for n in ("wino_ragged_17x65", "wino_multi_unit")]

# what the table above must come to (tests/test_fused_dgrad_cpu.py)
TABLE = {  # name: (strip_w, tile height, rows, Winograd units)
    "direct_n32_th4": (34, 4, 9, 0), "direct_n32_th8": (34, 8, 6, 0), "direct_n64": (34, 4, 9, 0), "direct_scale_zy": (34, 4, 9, 0),
    "direct_scale_zy_relu": (34, 4, 9, 0), "direct_scale_zy_k1": (34, 4, 9, 0), "direct_n24": (34, 4, 9, 0),
    "direct_strip": (21, 4, 6, 0), "direct_nostrip": (0, 4, 6, 0), "direct_zero_src": (34, 4, 9, 0),
    "wino_ragged": (0, 0, 4, 4), "wino_ragged_17x65": (0, 0, 12, 12), "wino_zero_src": (0, 0, 4, 4), "wino_ragged_relu": (0, 0, 4, 4),
    "wino_multi_unit": (0, 0, 256, 384),
}


def base_name(c):
    """an ALTERNATING case shares the inputs and the reference of the case it repeats"""
    return c["name"][:-4] if c["name"].endswith("_alt") else c["name"]


def expected(c):
    """what ``info`` must report, in the form of VC.expected()"""
    return ("wino", 32) if c["kernel"] == "wino" else ("f16x3",) + tuple(c["row"]) + (c["vec_epi"], c["strip_w"])


def reported(info):
    if info["launcher"] >= 2:
        return ("wino", 32 * (info["launcher"] - 1))
    return ("f16x3",) + tuple(info[k] for k in ("ntb", "vec", "up", "fuse2", "tailc", "th", "scaled", "k1", "n16", "vec_epi", "strip_w"))


def coverage(rows):
    """what a set of (reported row, rows, units) leaves uncovered: the fused f16x3 kernel with NTB 1 / 2, TH 4 / 8, with and without
    strips; the fused Winograd kernel with one unit per block and with several"""
    f16 = [r for r, _, _ in rows if r[0] == "f16x3" and r[7] == 1]
    missing = [("NTB", v) for v in (1, 2) if not any(r[1] == v for r in f16)]
    missing += [("TH", v) for v in (4, 8) if not any(r[6] == v for r in f16)]
    missing += [("strips", v) for v in (0, 1) if not any(bool(r[11]) == bool(v) for r in f16)]
    missing += [("K1", 1)] if not any(r[8] == 1 for r in f16) else []
    wino = [(n, u) for r, n, u in rows if r[0] == "wino"]
    missing += [("wino", "one unit per block")] if not any(u == n for n, u in wino) else []
    missing += [("wino", "several units per block")] if not any(u > n for n, u in wino) else []
    return missing


def plan_input(c):
    """The f16x3 launch of the case as hcf_debug_conv_plan's in[40] (include/hcflow.h): the scaled form with fb_y and fb_part"""
    v = [0] * 40
    v[0:6] = [0, c["k"] * c["k"], c["B"], c["H"], c["W"], len(c["srcs"])]
    for i, w in enumerate(c["srcs"]):
        v[6 + 5 * i: 11 + 5 * i] = [w[2], c["bufs"][w[0]][0], w[1], w[3], VC.aligned(c, w)]
    o, y = c["out"], c["y"]
    v[21:25] = [o[2], c["bufs"][o[0]][0], o[1], VC.aligned(c, o)]
    v[33], v[34] = 1, 0
    v[35:38] = [1 if VC.aligned(c, y) else 2, c["bufs"][y[0]][0], y[1]]
    v[38] = 1 | (2 if c["scale"] else 0)
    return v


def windows(c):
    """(read windows, written windows)"""
    return list(dict.fromkeys(c["srcs"] + [c["y"]])), [c["out"]]


# ---------------------------------------------------------------------------------------------------------------- inputs
def conv_d(c, d, dtype=torch.float64):
    x = torch.cat([d["win"][w].to(dtype) for w in c["srcs"]], 1)
    return F.conv2d(x, d["w"].to(dtype), None, 1, c["k"] // 2)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) % (2 ** 31))
    B, H, W, k, n = c["B"], c["H"], c["W"], c["k"], c["out"][2]

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    win = {}
    for w in c["srcs"]:
        win[w] = rn(B, w[2], H, W)                                     # gradients: randn
        if c["zero_src"]:
            win[w] = torch.zeros_like(win[w])
    cin = sum(w[2] for w in c["srcs"])
    d = dict(w=rn(n, cin, k, k) / (cin * k * k) ** 0.5, scale=torch.exp(rn(n) * 0.2) if c["scale"] else None)
    pre = rn(B, n, H, W)
    y = pre if c["act"] == "none" else F.relu(pre) if c["act"] == "relu" else F.leaky_relu(pre, 0.2)
    win[c["out"]] = rn(B, n, H, W)                                     # what the window held before: all of it must be overwritten
    d["win"] = win
    d["plants"] = None
    if c["act"] != "none" and not c["zero_src"]:
        dd = conv_d(c, d).abs().flatten()
        ok = (dd >= 1e-2 * dd.max()).nonzero().flatten()
        idx = ok[torch.randperm(ok.numel(), generator=g)[: 2 * NPLANT]]
        assert idx.numel() == 2 * NPLANT
        y = y.clone()
        y.view(-1)[idx[:NPLANT]] = 0.0
        y.view(-1)[idx[NPLANT:]] = -0.0
        d["plants"] = idx
    win[c["y"]] = y
    return d


def make_inputs(c):
    """float32 CPU tensors of the case (deterministic per case name; shared, never modified): d["win"][window] = NCHW data, d["w"],
    d["scale"] (or None), d["plants"] (flat indices into y: the first 16 hold 0.0, the next 16 -0.0; or None)"""
    return _inputs(base_name(c))


# ------------------------------------------------------------------------------------------------------------ references
def evaluate(c, d, dtype=torch.float64):
    dz = conv_d(c, d, dtype)
    y = d["win"][c["y"]].to(dtype)
    if c["act"] == "relu":
        dz = torch.where(y > 0, dz, torch.zeros_like(dz))
    elif c["act"] == "lrelu":
        dz = torch.where(y >= 0, dz, dz * 0.2)
    dpre = dz * d["scale"].to(dtype).view(1, -1, 1, 1) if c["scale"] else dz
    r = {"out": dpre, "sum_pre": dpre.sum((0, 2, 3))}
    if c["zy"]:
        r["sum_zy"] = c["zy_mult"] * (dz * y).sum((0, 2, 3))
    return r


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = BY_NAME[name]
    d = make_inputs(c)
    ref = evaluate(c, d)
    r32 = evaluate(c, d, torch.float32)
    e32 = {k: VC.err(r32[k], ref[k]) for k in ref}
    return ref, e32, {k: 4 * max(v, FLOOR) for k, v in e32.items()}


def reference(c):
    """(float64 outputs, e32 per output = the error of the float32 CPU evaluation, gate per output = 4 max(e32, FLOOR)); computed
    once per case and shared"""
    return _reference(base_name(c))
