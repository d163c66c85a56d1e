"""The cases of tests/test_gpu_view_convs.py, shared with tests/test_view_convs_cpu.py: the conv, weight-gradient and
epilogue-backward kernels on channel WINDOWS of shared buffers, as the engine uses them. Geometry, the launch each case must
report, its inputs, the float64 / float32 CPU evaluation and the arena its buffers are cut from. No GPU, no shared library.

A window is a tuple (buffer name, c0, n, up). A buffer is (cs, misaligned, up): ``cs`` floats per pixel, its base off by 4
bytes when ``misaligned``, held at half resolution when ``up`` = 1. Every buffer of a case lies in ONE flat float32 tensor as

    [64-float guard][0 or 1 float of pad][B * H * W * cs floats][64-float guard]     (each segment starts 16-byte aligned)

pre-filled with a FILL before the windows are written: "nan" (every float a NaN), "loud" (finite, distinct per element,
magnitudes in [1e3, 6e4], inside the f16 range: a leak shows as wrong numbers, not as a range refusal) or "zero" (the dense
twin of a case only). Kernels may READ a few floats past a buffer (the engine allocates 64 bytes of slack; the guards stand for
it) and must never WRITE outside the out window.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

CAP = 1e-5            # the gate 4 * max(e32, FLOOR) must stay within this for every case
FLOOR = 1e-6
ABL_NO_WINO = 256
GUARD = 64
NO_TH4 = {"HCF_NO_TH4": "1"}
NO_DG_TH4 = {"HCF_NO_DG_TH4": "1"}
SWITCHES = ("HCF_NO_TH4", "HCF_NO_DG_TH4", "HCF_NO_DG_STRIP", "HCF_NO_WG_STRIP", "HCF_WG_SINGLE_BUF", "HCF_WG_DB_BLOCK", "HCF_NO_K1")


def ru4(n):
    return (n + 3) & ~3


def case_id(c):
    return "%s-%s" % (c["kind"], c["name"])


# ------------------------------------------------------------------------------------------------------------ the tables
def f16_row(ntb, vec, up, th, scaled=0, k1=0):
    """a kVariants row of hcf_conv_f16x3.hip without FUSE2 / TAILC / N16: (NTB, VEC, UP, FUSE2, TAILC, TH, SCALED, K1, N16)"""
    return (ntb, vec, up, 0, 0, th, scaled, k1, 0)


def strip_width(B, W):
    """The launchers' strip rule (conv_f16x3_scaled_blocks, plan_conv_wgrad): the B images of a tile row side by side, one zero
    column between them, where that saves >= 10 % of the 32-wide tiles; W + 1, or 0 without strips. At these sizes every scaled
    and every f16x3 weight-gradient launch walks strips: (2, 33) 3 against 4, (2, 34) 3 against 4, (3, 20) 2 against 3."""
    strips, tiles = (B * (W + 1) + 31) // 32, B * ((W + 31) // 32)
    return W + 1 if B >= 2 and strips * 10 <= tiles * 9 else 0


def _conv(name, bufs, srcs, out, row, vec_epi, exact, k=3, act="lrelu", wino=0, res1=None, res2=None, scaled=False, env=None,
          B=2, H=9, W=33, k1_exact=False):
    """row / vec_epi / strip_w: what the f16x3 kernel's plan reports (with Winograd ablated where ``wino`` = 32 / 64, the kernel
    the f16x3 run takes otherwise); exact: (VEC, vec_epi, NT) of conv_mfma_kernel; k1_exact: the f16x3 plan refuses this 1x1 conv
    and the f16x3 run IS the exact kernel."""
    return dict(kind="conv", name=name, B=B, H=H, W=W, k=k, bufs=dict(bufs), srcs=list(srcs), out=out, res1=res1, res2=res2,
                rs1=0.2, rs2=0.2, act=act, scaled=scaled, env=dict(env or {}), row=row, vec_epi=vec_epi,
                strip_w=strip_width(B, W) if scaled else 0, exact=exact,
                wino=wino, k1_exact=k1_exact)


XIN, GROW = ("xin", 0, 64, 0), ("grow", 0, 64, 0)
_GB = {"xin": (64, 0, 0), "grow": (128, 0, 0)}              # a dense block's input and its growth buffer
_ZH = ("h", 64, 64, 0)                                      # a coupling net's second source: 64 channels at 64 of 128

CONV_CASES = [
    # dense-block growth: conv i writes grow[64:96] of the buffer conv i + 1 reads as grow[0:96]
    _conv("growth", _GB, [XIN, GROW], ("grow", 64, 32, 0), f16_row(1, 1, 0, 4), 1, (1, 1, 1), wino=32),
    # the block's last conv: both residuals are windows, out sits at channel 32 of a wider buffer
    _conv("rdb_last", dict(_GB, r2=(128, 0, 0), o=(128, 0, 0)), [XIN, GROW], ("o", 32, 64, 0), f16_row(2, 1, 0, 4), 1, (1, 1, 2),
          act=None, wino=64, res1=XIN, res2=("r2", 64, 64, 0)),
    # z1 = z[:3] beside live z2 (channels 3 .. 5 of the same records)
    _conv("z1_tail", {"z": (8, 0, 0), "h": (128, 0, 0), "o": (64, 0, 0)}, [("z", 0, 3, 0), _ZH], ("o", 0, 64, 0), f16_row(2, 1, 0, 4), 1,
          (1, 1, 2), act="relu"),
    # Affine3shift: z[3:12], c0 & 3 != 0, the last unit of every pixel reads 3 floats past its record
    _conv("shift3", {"z": (12, 0, 0), "h": (128, 0, 0), "o": (64, 0, 0)}, [("z", 3, 9, 0), _ZH], ("o", 0, 64, 0), f16_row(2, 0, 1, 8), 1,
          (0, 1, 2), act="relu"),
    _conv("shift3_n32", {"z": (12, 0, 0), "h": (128, 0, 0), "o": (32, 0, 0)}, [("z", 3, 9, 0), _ZH], ("o", 0, 32, 0), f16_row(1, 0, 1, 8), 1,
          (0, 1, 1), act="relu"),
    _conv("misaligned_src", {"x": (64, 1, 0), "o": (32, 0, 0)}, [("x", 0, 64, 0)], ("o", 0, 32, 0), f16_row(1, 0, 1, 8), 1, (0, 1, 1)),
    _conv("misaligned_out", {"x": (64, 0, 0), "o": (64, 1, 0)}, [("x", 0, 64, 0)], ("o", 0, 64, 0), f16_row(2, 1, 0, 8), 0, (1, 0, 2)),
    _conv("out_c0_2", {"x": (64, 0, 0), "o": (36, 0, 0)}, [("x", 0, 64, 0)], ("o", 2, 32, 0), f16_row(1, 1, 0, 8), 0, (1, 0, 1)),
    # whole quads but not a whole 32-channel tile, live channels behind the window: the vector epilogues' c4 < n4
    _conv("out_n24", {"x": (64, 0, 0), "o": (64, 0, 0)}, [("x", 0, 64, 0)], ("o", 8, 24, 0), f16_row(1, 1, 0, 4), 1, (1, 1, 1)),
    # a Conv2dZeros-like head: input and output channel tails, live channels on both sides of both windows
    _conv("head_tails", {"x": (32, 0, 0), "o": (32, 0, 0)}, [("x", 8, 21, 0)], ("o", 4, 22, 0), f16_row(1, 1, 0, 8), 0, (1, 0, 1), act=None),
    _conv("up_window", {"a": (12, 0, 0), "cf": (96, 0, 1), "o": (64, 0, 0)}, [("a", 0, 12, 0), ("cf", 32, 64, 1)], ("o", 0, 64, 0),
          f16_row(2, 1, 1, 8), 1, (1, 1, 2), act="relu", H=10, W=34),
    _conv("up_window_n32", {"a": (12, 0, 0), "cf": (96, 0, 1), "o": (32, 0, 0)}, [("a", 0, 12, 0), ("cf", 32, 64, 1)], ("o", 0, 32, 0),
          f16_row(1, 1, 1, 8), 1, (1, 1, 1), act="relu", H=10, W=34),
]
_KB = {"grow": (128, 0, 0), "o": (128, 0, 0)}
for _n, _ntb in ((64, 2), (32, 1)):
    for _th, _env in ((4, None), (8, NO_TH4)):
        CONV_CASES.append(_conv("k1_n%d_th%d" % (_n, _th), _KB, [GROW], ("o", 32, _n, 0), f16_row(_ntb, 1, 0, _th, k1=1), 1,
                                (1, 1, _ntb), k=1, act="relu", env=_env))
CONV_CASES.append(_conv("k1_unaligned", {"x": (68, 0, 0), "o": (128, 0, 0)}, [("x", 2, 64, 0)], ("o", 32, 64, 0), None, 1, (0, 1, 2), k=1,
                        act="relu", k1_exact=True))
# the training data-gradient form (ConvArgs::in_max): windows as in `growth`; *_acc accumulates into out through res1, as bwd_conv does
for _n, _ntb in ((32, 1), (64, 2)):
    for _th, _env in ((4, None), (8, NO_DG_TH4)):
        _o = ("grow", 64, _n, 0)
        CONV_CASES.append(_conv("scaled_n%d_th%d" % (_n, _th), _GB, [XIN, GROW], _o, f16_row(_ntb, 1, 0, _th, scaled=1), 1, (1, 1, _ntb),
                                act=None, wino=_n, scaled=True, env=_env, res1=_o if _th == 4 else None))
        CONV_CASES.append(_conv("scaled_k1_n%d_th%d" % (_n, _th), _GB, [GROW], _o, f16_row(_ntb, 1, 0, _th, scaled=1, k1=1), 1,
                                (1, 1, _ntb), k=1, act=None, scaled=True, env=_env))
# strips: B (W + 1) = 63 columns are 2 strips of 32 against 3 per-image tiles (>= 10 % saved)
CONV_CASES.append(_conv("scaled_strip", _GB, [XIN, GROW], ("grow", 64, 32, 0), f16_row(1, 1, 0, 4, scaled=1), 1, (1, 1, 1), act=None, wino=32,
                        scaled=True, res1=("grow", 64, 32, 0), B=3, W=20))
assert CONV_CASES[-1]["strip_w"] == 21


def _wg(name, bufs, srcs, g, vec, k=3, B=2, H=9, W=33):
    """vec: the VEC argument of both weight-gradient kernels; strip_w: of the f16x3 kernel's plan"""
    return dict(kind="wgrad", name=name, B=B, H=H, W=W, k=k, bufs=dict(bufs), srcs=list(srcs), g=g, vec=vec, strip_w=strip_width(B, W),
                env={})


_GG = dict(_GB, gg=(128, 0, 0))
WGRAD_CASES = [
    _wg("growth", _GG, [XIN, GROW], ("gg", 64, 32, 0), 1),
    _wg("shift3", {"z": (12, 0, 0), "h": (128, 0, 0), "g": (64, 0, 0)}, [("z", 3, 9, 0), _ZH], ("g", 0, 64, 0), 0),
    _wg("head_tails", {"x": (32, 0, 0), "g": (32, 0, 0)}, [("x", 8, 21, 0)], ("g", 4, 22, 0), 1),
    _wg("misaligned", {"x": (64, 1, 0), "g": (32, 0, 0)}, [("x", 0, 64, 0)], ("g", 0, 32, 0), 0),
    _wg("up_window", {"a": (12, 0, 0), "cf": (96, 0, 1), "g": (64, 0, 0)}, [("a", 0, 12, 0), ("cf", 32, 64, 1)], ("g", 0, 64, 0), 1, H=10, W=34),
    _wg("taps1", {"grow": (128, 0, 0), "g": (128, 0, 0)}, [GROW], ("g", 32, 64, 0), 1, k=1),
    _wg("taps1_unaligned", {"x": (68, 0, 0), "g": (128, 0, 0)}, [("x", 2, 64, 0)], ("g", 32, 64, 0), 0, k=1),
    _wg("strip", _GG, [XIN, GROW], ("gg", 64, 32, 0), 1, B=3, W=20),
]
assert WGRAD_CASES[-1]["strip_w"] == 21


def _epi(name, act, n, gy, y, g1, g2, bufs, vec):
    """in place on ``gy``; vec: conv_epilogue_bwd_vec_kernel runs"""
    return dict(kind="epi", name=name, B=2, H=9, W=33, act=act, n=n, bufs=dict(bufs), gy=gy, y=y, g1=g1, g2=g2, rs1=0.2, rs2=0.3,
                zy_mult=3.0 if act == "none" else 1.0, vec=vec, env={})


EPI_CASES = []
for _act in ("none", "relu", "lrelu"):
    EPI_CASES.append(_epi("vec_" + _act, _act, 32, ("G", 32, 32, 0), ("Y", 16, 32, 0), ("G1", 64, 32, 0), ("G2", 0, 32, 0),
                          {"G": (128, 0, 0), "Y": (64, 0, 0), "G1": (96, 0, 0), "G2": (32, 0, 0)}, 1))
    EPI_CASES.append(_epi("scalar_" + _act, _act, 22, ("G", 3, 22, 0), ("Y", 2, 22, 0), ("G1", 0, 22, 0), ("G2", 5, 22, 0),
                          {"G": (28, 0, 0), "Y": (25, 0, 0), "G1": (22, 0, 0), "G2": (30, 0, 0)}, 0))

CASES = CONV_CASES + WGRAD_CASES + EPI_CASES
assert len({case_id(c) for c in CASES}) == len(CASES)


def modes(c):
    """the runs of a case: op precision, and once more without Winograd where the f16x3 run takes it"""
    if c["kind"] == "epi":
        return ["exact"]
    return ["exact", "f16x3"] + (["f16x3_nowino"] if c["kind"] == "conv" and c["wino"] else [])


def precision(mode):
    return "exact" if mode == "exact" else "f16x3"


def ablation(mode):
    return ABL_NO_WINO if mode == "f16x3_nowino" else 0


def expected(c, mode):
    """what ``info`` must report for the run, as a tuple that starts with the kernel family"""
    if c["kind"] == "epi":
        return ("epi", c["vec"])
    if c["kind"] == "wgrad":
        f16 = int(mode != "exact")
        return ("wgrad", f16, c["k"] * c["k"], c["vec"], 2 if f16 else 0, c["strip_w"] if f16 else 0)
    if mode == "exact" or c["k1_exact"]:
        return ("exact",) + tuple(c["exact"])
    if mode == "f16x3" and c["wino"]:
        return ("wino", c["wino"])
    return ("f16x3",) + tuple(c["row"]) + (c["vec_epi"], c["strip_w"])


def reported(c, info):
    """``info`` of the entry (hcflow_amd.ops) in the form of expected()"""
    if c["kind"] == "epi":
        return ("epi", info["vec"])
    if c["kind"] == "wgrad":
        return ("wgrad",) + tuple(info[k] for k in ("f16", "taps", "vec", "db", "strip_w"))
    if info["launcher"] == 0:
        return ("exact", info["ntb"], info["vec"], info["up"])           # VEC, vec_epi, NT travel in the first three row fields
    if info["launcher"] >= 2:
        return ("wino", 32 * (info["launcher"] - 1))
    return ("f16x3",) + tuple(info[k] for k in ("ntb", "vec", "up", "fuse2", "tailc", "th", "scaled", "k1", "n16", "vec_epi", "strip_w"))


# every row the cases must reach between them (tests/test_view_convs_cpu.py, and the rows SEEN on the GPU)
SCALED_K1_ROWS = ({f16_row(n, 1, 0, th, scaled=1) for n in (1, 2) for th in (4, 8)} |
                  {f16_row(n, 1, 0, th, scaled=s, k1=1) for n in (1, 2) for th in (4, 8) for s in (0, 1)})
UP_ROWS = {f16_row(n, v, 1, 8) for n in (1, 2) for v in (0, 1)}
WGRAD_ROWS = {(f16, taps, vec) for f16 in (0, 1) for taps in (9, 1) for vec in (0, 1)}
assert len(SCALED_K1_ROWS) == 12 and len(UP_ROWS) == 4 and len(WGRAD_ROWS) == 8


def coverage(rows):
    """what a set of expected() / reported() tuples leaves uncovered of the list above (empty: all covered)"""
    f16 = {r[1:10] for r in rows if r[0] == "f16x3"}
    wg = {r[1:4] for r in rows if r[0] == "wgrad"}
    missing = [("f16x3",) + r for r in sorted((SCALED_K1_ROWS | UP_ROWS) - f16)] + [("wgrad",) + r for r in sorted(WGRAD_ROWS - wg)]
    missing += [("epi", v) for v in (0, 1) if ("epi", v) not in rows]
    missing += [("wino", n) for n in (32, 64) if ("wino", n) not in rows]
    missing += [("exact VEC", v) for v in (0, 1) if not any(r[0] == "exact" and r[1] == v for r in rows)]
    missing += [("exact vec_epi", v) for v in (0, 1) if not any(r[0] == "exact" and r[2] == v for r in rows)]
    return missing


def aligned(c, w):
    """view_vec16 of hcf_launch.h"""
    cs, mis, _ = c["bufs"][w[0]]
    return int(not mis and (cs & 3) == 0 and (w[1] & 3) == 0)


def plan_input(c, mode):
    """The run as hcf_debug_conv_plan's in[40] (include/hcflow.h), or None where no plan decides it (exact kernel, Winograd,
    epilogue backward)."""
    if c["kind"] == "epi" or expected(c, mode)[0] in ("exact", "wino"):
        return None
    v = [0] * 40
    wg = c["kind"] == "wgrad"
    v[0:6] = [int(wg), c["k"] * c["k"], c["B"], c["H"], c["W"], len(c["srcs"])]
    for i, w in enumerate(c["srcs"]):
        v[6 + 5 * i: 11 + 5 * i] = [w[2], c["bufs"][w[0]][0], w[1], w[3], aligned(c, w)]
    o = c["g"] if wg else c["out"]
    v[21:25] = [o[2], c["bufs"][o[0]][0], o[1], aligned(c, o)]
    if wg:
        v[33] = int(mode != "exact")            # g_max: the f16x3 kernel
        return v
    for j, r in ((25, c["res1"]), (28, c["res2"])):
        if r is not None:
            v[j:j + 3] = [1 if aligned(c, r) else 2, c["bufs"][r[0]][0], r[1]]
    v[33] = int(c["scaled"])
    v[34] = {None: 0, "none": 0, "relu": 1, "lrelu": 2}[c["act"]]
    return v


# ------------------------------------------------------------------------------------------------------------- the arena
def buf_shape(c, name):
    cs, _, up = c["bufs"][name]
    return c["B"], c["H"] >> up, c["W"] >> up, cs


def layout(c):
    """({buffer: offset of its first float in the arena}, floats of the arena)"""
    off, pos = {}, 0
    for name in c["bufs"]:
        B, H, W, cs = buf_shape(c, name)
        off[name] = pos + GUARD + c["bufs"][name][1]
        pos = (off[name] + B * H * W * cs + GUARD + 3) & ~3
    return off, pos


def windows(c):
    """(read windows, written windows) of the case, each once"""
    if c["kind"] == "conv":
        rd, wr = c["srcs"] + [r for r in (c["res1"], c["res2"]) if r is not None], [c["out"]]
    elif c["kind"] == "wgrad":
        rd, wr = c["srcs"] + [c["g"]], []
    else:
        rd, wr = [c["gy"], c["y"], c["g1"], c["g2"]], [c["gy"], c["g1"], c["g2"]]
    return list(dict.fromkeys(rd)), list(dict.fromkeys(wr))


def fill_tensor(n, fill):
    if fill == "zero":
        return torch.zeros(n)
    if fill == "nan":
        return torch.full((n,), float("nan"))
    assert fill == "loud"
    g = torch.Generator().manual_seed(n)
    mag = 1.0e3 + 5.9e4 * (torch.randperm(n, generator=g).double() + 0.5) / n
    return (mag * (1.0 - 2.0 * (torch.arange(n) & 1))).float()


def buf_view(c, arena, name):
    """the buffer as an [B, H, W, cs] view of the arena"""
    B, H, W, cs = buf_shape(c, name)
    o = layout(c)[0][name]
    return arena[o: o + B * H * W * cs].view(B, H, W, cs)


def put(c, arena, w, t):
    """write the NCHW tensor ``t`` into window ``w``"""
    buf_view(c, arena, w[0])[..., w[1]: w[1] + w[2]] = t.permute(0, 2, 3, 1)


def get(c, arena, w):
    """window ``w`` as an NCHW tensor (a copy)"""
    return buf_view(c, arena, w[0])[..., w[1]: w[1] + w[2]].permute(0, 3, 1, 2).contiguous()


def outside_mask(c, wins):
    """bool over the arena: True for every float outside the listed windows (guards, pads, other channels, other buffers)"""
    m = torch.ones(layout(c)[1], dtype=torch.bool)
    for w in wins:
        buf_view(c, m, w[0])[..., w[1]: w[1] + w[2]] = False
    return m


def outside_count(c, wins):
    """the element count of outside_mask that the geometry predicts (distinct windows)"""
    n = layout(c)[1]
    for w in dict.fromkeys(wins):
        B, H, W, _ = buf_shape(c, w[0])
        n -= B * H * W * w[2]
    return n


def build_arena(c, d, fill):
    """the arena of the case: ``fill`` everywhere, then every window's data (d["win"])"""
    a = fill_tensor(layout(c)[1], fill)
    for w, t in d["win"].items():
        put(c, a, w, t)
    return a


def dense_twin(c):
    """The same case on dense zero-padded views at channel 0, as the older per-op entries build them: every distinct window in a
    buffer of its own with roundup4(n) channels, 16-byte aligned. Returns (case, {window of c: window of the twin})."""
    rd, wr = windows(c)
    m, bufs = {}, {}
    for i, w in enumerate(dict.fromkeys(rd + wr)):
        bufs["d%d" % i] = (ru4(w[2]), 0, w[3])
        m[w] = ("d%d" % i, 0, w[2], w[3])
    t = dict(c, bufs=bufs, name=c["name"] + "_dense")
    for k in ("out", "res1", "res2", "g", "gy", "y", "g1", "g2"):
        if t.get(k) is not None:
            t[k] = m[t[k]]
    if "srcs" in t:
        t["srcs"] = [m[w] for w in c["srcs"]]
    return t, m


def twin_inputs(d, m):
    """the inputs of a case for its dense twin"""
    return dict(d, win={m[w]: t for w, t in d["win"].items()})


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _inputs(cid):
    c = next(x for x in CASES if case_id(x) == cid)
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()) % (2 ** 31))
    B, H, W = c["B"], c["H"], c["W"]

    def rn(*shape):
        return torch.randn(*shape, generator=g)
    win = {}
    if c["kind"] == "epi":
        n = c["n"]
        scale = torch.exp(rn(n) * 0.3)
        pre = rn(B, n, H, W)
        y = pre if c["act"] == "none" else F.relu(pre) if c["act"] == "relu" else F.leaky_relu(pre, 0.2)
        win = {c["gy"]: rn(B, n, H, W), c["y"]: y, c["g1"]: rn(B, n, H, W), c["g2"]: rn(B, n, H, W)}
        return dict(win=win, scale=scale, sp0=rn(n), sz0=rn(n))
    for w in c["srcs"]:
        win[w] = rn(B, w[2], H >> w[3], W >> w[3])
    cin, k = sum(w[2] for w in c["srcs"]), c["k"]
    if c["kind"] == "wgrad":
        win[c["g"]] = rn(B, c["g"][2], H, W)
        return dict(win=win)
    cout = c["out"][2]
    d = dict(w=rn(cout, cin, k, k) / (cin * k * k) ** 0.5, bias=rn(cout) * 0.2, scale=torch.exp(rn(cout) * 0.2))
    for r in (c["res1"], c["res2"]):
        if r is not None and r not in win:
            win[r] = rn(B, cout, H, W)
    if c["out"] not in win:
        win[c["out"]] = rn(B, cout, H, W)              # what the window held before: all of it must be overwritten
    d["win"] = win
    return d


def make_inputs(c):
    """float32 CPU tensors of the case (deterministic per case name; shared, never modified): d["win"][window] = NCHW data"""
    return _inputs(case_id(c))


# ------------------------------------------------------------------------------------------------------------ references
def evaluate(c, d, dtype=torch.float64):
    """{output name: tensor} in ``dtype``. conv: the expressions of tests/test_gpu_fuzz.py::test_conv2d_fuzz; wgrad:
    torch.nn.grad.conv2d_weight; epi: the closed form of tests/train_glue_ref.py::epi_closed."""
    t = lambda v: v.to(dtype)
    if c["kind"] == "epi":
        gy, y, sc = t(d["win"][c["gy"]]), t(d["win"][c["y"]]), t(d["scale"]).view(1, -1, 1, 1)
        dz = gy * (c["rs2"] * c["rs1"])
        if c["act"] == "relu":
            dz = torch.where(y > 0, dz, torch.zeros_like(dz))
        elif c["act"] == "lrelu":
            dz = torch.where(y >= 0, dz, dz * 0.2)
        gpre = dz * sc
        return {"gpre": gpre, "g1": t(d["win"][c["g1"]]) + gy * c["rs2"], "g2": t(d["win"][c["g2"]]) + gy,
                "sum_pre": t(d["sp0"]) + gpre.sum((0, 2, 3)), "sum_zy": t(d["sz0"]) + c["zy_mult"] * (dz * y).sum((0, 2, 3)),
                "absmax": gpre.abs().max().view(1)}
    x = torch.cat([F.interpolate(t(d["win"][w]), scale_factor=2 ** w[3], mode="nearest") if w[3] else t(d["win"][w]) for w in c["srcs"]], 1)
    k = c["k"]
    if c["kind"] == "wgrad":
        g = t(d["win"][c["g"]])
        return {"dw": torch.nn.grad.conv2d_weight(x, (g.shape[1], x.shape[1], k, k), g, padding=k // 2)}
    ref = (F.conv2d(x, t(d["w"]), None, 1, k // 2) + t(d["bias"]).view(1, -1, 1, 1)) * t(d["scale"]).view(1, -1, 1, 1)
    if c["act"] == "relu":
        ref = F.relu(ref)
    elif c["act"] == "lrelu":
        ref = F.leaky_relu(ref, 0.2)
    if c["res1"] is not None:
        ref = ref * c["rs1"] + t(d["win"][c["res1"]])
    if c["res2"] is not None:
        ref = ref * c["rs2"] + t(d["win"][c["res2"]])
    return {"out": ref}


def err(got, ref64):
    """max |got - ref64| / max(1, max |ref64|)"""
    return float((got.double() - ref64).abs().max()) / max(1.0, float(ref64.abs().max()))


@functools.lru_cache(maxsize=None)
def _reference(cid):
    c = next(x for x in CASES if case_id(x) == cid)
    d = make_inputs(c)
    ref = evaluate(c, d)
    r32 = evaluate(c, d, torch.float32)
    e32 = {k: err(r32[k], ref[k]) for k in ref}
    return ref, e32, {k: 4 * max(v, FLOOR) for k, v in e32.items()}


def reference(c):
    """(float64 outputs, e32 per output = the error of the float32 CPU evaluation, gate per output = 4 max(e32, FLOOR)); computed
    once per case and shared"""
    return _reference(case_id(c))
