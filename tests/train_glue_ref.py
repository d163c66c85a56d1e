"""References for the backward kernels of the training path (hcflow_amd/csrc/hcf_train.hip), one kernel at a time.

Every case builds float32 inputs, evaluates the FORWARD formula in float64 on their float32 images and takes ``torch.autograd``
of the scalar ``sum(g_out * out) + gobj * sum_b(objective_b)`` with a random ``g_out``. The tensors the engine would have taped
(zout, za, x, zc, a, y) are computed in float64 and rounded to float32 before they go to the kernel. Beside the autograd reference
each family has the closed form documented in hcf_common.h (EpiBwdArgs, StepBwdArgs, StepInvBwdArgs, PriorBwdArgs, LuChainArgs),
written over a dtype: tests/test_train_glue_ref_cpu.py holds it to the autograd reference in float64 and, evaluated in float32, to
half of the gate that tests/test_gpu_train_glue.py applies to the kernel, so a failure there is never the inputs' conditioning.

A reference is a dict ``name -> ("v", ref)`` (elementwise: |got - ref| <= 2e-6 * max(1, |ref|max)) or ``("s", ref, absterms)``
(per-channel sum: |got - ref| <= 1e-5 * sum |terms| of that channel): the gates of tests/test_gpu_flow_glue.py.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import hcflow_oracle as O
from tests.test_gpu_flow_glue import GAUSS_CASES, STEP_CASES as _FLOW_STEP_CASES

B = 3
AFFINE, SHIFT3 = 0, 1

# (C, ns, H, W, mode, has_mat). Register buckets 8 / 12 / 24 / 48 of the step kernels each see two or more 256-pixel blocks per
# sample with fewer than 64 pixels in the last one (waves 1..3 of that block own no pixel):
#   8: (6, 3, 33, 8) 264 px;  12: (10, 5, 17, 16) 272 px and the shift case, 300 px;  24: (24, 12, 17, 31) 527 px, (21, 10, 19, 14)
#   266 px;  48: (48, 24, 17, 16) 272 px, (45, 22, 19, 14) 266 px.  (45, 22, 13, 10): 130 px, an empty fourth wave;
#   (12, 6, 16, 16): exactly one full block;  (12, 3, 15, 20) SHIFT3 without a matrix: 300 px.
STEP_CASES = [c + (AFFINE, True) for c in _FLOW_STEP_CASES] + [
    (48, 24, 17, 16, AFFINE, True), (45, 22, 19, 14, AFFINE, True), (10, 5, 17, 16, AFFINE, True), (12, 6, 16, 16, AFFINE, True),
    (12, 3, 15, 20, SHIFT3, False)]

QUANT_CASES = [(2, 17, 31), (3, 8, 8)]

# (B, H, W, n, cs, c0): 3 x 9 x 11 = 297 px is one full 192-pixel block and a ragged one; 2 x 5 x 7 = 70 px a single partial block.
# n = 64 / 32 / 12 in a 4-float aligned window take the vector kernel (n = 12: three channel quads, thread 255 idle), n = 22 / 6
# and the window at c0 = 2 the scalar kernel.
EPI_LAYOUTS = [(3, 9, 11, 64, 64, 0), (3, 9, 11, 32, 32, 0), (3, 9, 11, 12, 12, 0), (3, 9, 11, 22, 24, 0), (3, 9, 11, 6, 8, 0),
               (3, 9, 11, 32, 96, 4), (3, 9, 11, 32, 36, 2), (2, 5, 7, 32, 32, 0), (2, 5, 7, 22, 24, 0)]
EPI_ACTS = ["none", "relu", "lrelu"]
EPI_RES = ["none", "res1", "both"]
EPI_CASES = [(lay, act, res) for lay in EPI_LAYOUTS for act in EPI_ACTS for res in EPI_RES]
RS1, RS2 = 0.2, 0.7

LU_CASES = [3, 12, 24, 45, 48]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _interleave(a, b):
    """(a, b) -> the "cross" layout h[:, 0::2] = a, h[:, 1::2] = b."""
    return torch.stack((a, b), 2).reshape(a.shape[0], 2 * a.shape[1], a.shape[2], a.shape[3])


def _chan(x):
    return x.sum(dim=(0, 2, 3))


def _t(k, name, dt):
    """Input ``name`` of a kernel in dtype ``dt``: the float32 tensor the kernel gets, or -- float64, for a tensor the engine would
    have taped -- its unrounded float64 value (k["exact"]), which is what the autograd reference differentiates through."""
    if dt == torch.float64 and name in k.get("exact", {}):
        return k["exact"][name]
    return k[name].to(dt)


def _mat(Wm, x):
    """y[b, i] = sum_j Wm[i, j] x[b, j] per pixel."""
    return torch.einsum("ij,bjhw->bihw", Wm, x)


# ---------------------------------------------------------------- gates
def vgate(ref):
    return 2e-6 * max(1.0, float(ref.abs().max()))


def worst_ratio(got, entry):
    """max over the elements of |got - ref| / gate, with the error and the gate of the worst element."""
    got = got.detach().cpu().double()
    if entry[0] == "v":
        ref = entry[1]
        err = float((got - ref).abs().max()) if ref.numel() else 0.0
        g = vgate(ref) if ref.numel() else 2e-6
        return err / g, err, g
    ref, absterms = entry[1], entry[2]
    gate = 1e-5 * absterms
    err = (got.reshape(ref.shape) - ref).abs()
    ratio = err / gate.clamp_min(1e-300)
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), float(err.flatten()[i]), float(gate.flatten()[i])


def check(got, ref, what, frac=1.0):
    """Every output of ``got`` against the reference dict; prints measured error and gate, then asserts."""
    bad = []
    for name, entry in ref.items():
        r, err, g = worst_ratio(got[name], entry)
        print("%s %s: error %.3e, gate %.3e (%.3f of the gate)" % (what, name, err, frac * g, r / frac))
        if not r <= frac:
            bad.append((name, err, frac * g))
    assert not bad, (what, bad)


# ---------------------------------------------------------------- flow step, forward direction
@functools.lru_cache(maxsize=None)
def step_inputs(C, ns, H, W, mode, has_mat):
    """z, h, W, bias, logs as test_gpu_flow_glue.py::test_step_affine_multi_block draws them; then the gradients."""
    g = _gen(1000 * C + H)
    z = torch.randn(B, C, H, W, generator=g)
    if mode == AFFINE:
        h = torch.randn(B, 2 * (C - ns), H, W, generator=g) * 0.5
    else:
        h = torch.randn(B, 3, H, W, generator=g)
    Wm = torch.linalg.qr(torch.randn(C, C, generator=g, dtype=torch.float64))[0].float() * 1.1
    bias = torch.randn(1, C, 1, 1, generator=g) * 0.1
    logs = torch.randn(1, C, 1, 1, generator=g) * 0.1
    gout = torch.randn(B, C, H, W, generator=g)
    gb0 = torch.randn(C, generator=g)
    gl0 = torch.randn(C, generator=g)
    return dict(z=z, h=h, W=Wm if has_mat else None, bias=bias, logs=logs, gout=gout, gb0=gb0, gl0=gl0, gobj=-0.7, ns=ns, mode=mode)


def _couple_fwd(zb, h, ns, mode):
    if mode == AFFINE:
        shift, scale = O.split_cross(h)
        ls = O.logscale_of(scale)
        return torch.cat((zb[:, :ns], (zb[:, ns:] + shift) * torch.exp(ls)), 1), ls
    return torch.cat((zb[:, :3] + h, zb[:, 3:]), 1), None


@functools.lru_cache(maxsize=None)
def step_forward_case(*case):
    """(kernel inputs, reference) of za = (zin + b) e^s, zb = W za, zout = coupling(zb, h); objective_b = sum ls."""
    inp = step_inputs(*case)
    ns, mode, gobj = inp["ns"], inp["mode"], inp["gobj"]
    zin, h, b, s = [inp[k].double().requires_grad_(True) for k in ("z", "h", "bias", "logs")]
    Wd = inp["W"].double() if inp["W"] is not None else None
    za = (zin + b) * torch.exp(s)
    zb = _mat(Wd, za) if Wd is not None else za
    zout, ls = _couple_fwd(zb, h, ns, mode)
    gout = inp["gout"].double()
    loss = (gout * zout).sum()
    if ls is not None:
        loss = loss + gobj * ls.sum()
    gzin, gh, gb, gs = torch.autograd.grad(loss, [zin, h, b, s])
    # the terms of the two per-channel sums: d bias = sum gzin, d logs = sum gzin (zin + b)
    t_logs = (gzin * (zin + b)).detach()
    ref = {"gzin": ("v", gzin), "gh": ("v", gh),
           "g_bias": ("s", inp["gb0"].double() + gb.flatten(), _chan(gzin.abs()) + inp["gb0"].double().abs()),
           "g_logs": ("s", inp["gl0"].double() + gs.flatten(), _chan(t_logs.abs()) + inp["gl0"].double().abs())}
    kin = dict(gzout=inp["gout"], zout=zout.detach().float(), h=inp["h"], za=za.detach().float(), W=inp["W"], logs=inp["logs"],
               gobj=gobj, ns=ns, mode=mode, gb0=inp["gb0"], gl0=inp["gl0"], exact=dict(zout=zout.detach(), za=za.detach()))
    return kin, ref


def step_forward_closed(k, dt):
    """StepBwdArgs: coupling backward (gzout, zout, h) -> gzb, gh; head backward (gzb, za) -> gzin and the two sums."""
    gzout, zout, h, za, s = [_t(k, n, dt) for n in ("gzout", "zout", "h", "za", "logs")]
    ns = k["ns"]
    if k["mode"] == AFFINE:
        scale = h[:, 1::2]
        e = torch.exp(0.318 * torch.atan(2 * scale))
        g2 = gzout[:, ns:]
        gzb = torch.cat((gzout[:, :ns], g2 * e), 1)
        dls = g2 * zout[:, ns:] + k["gobj"]
        gh = _interleave(g2 * e, dls * (0.636 / (1 + 4 * scale * scale)))
    else:
        gzb, gh = gzout, gzout[:, :3]
    gza = _mat(k["W"].to(dt).t(), gzb) if k["W"] is not None else gzb
    gzin = gza * torch.exp(s)
    return {"gzin": gzin, "gh": gh, "g_bias": k["gb0"].to(dt) + _chan(gzin), "g_logs": k["gl0"].to(dt) + _chan(gza * za)}


# ---------------------------------------------------------------- flow step, inverse direction
@functools.lru_cache(maxsize=None)
def step_inverse_case(*case):
    """zc = coupling^-1(z, h), y = W^-1 zc, x = y e^-s - b; no objective term."""
    inp = step_inputs(*case)
    ns, mode = inp["ns"], inp["mode"]
    z, h, b, s = [inp[k].double().requires_grad_(True) for k in ("z", "h", "bias", "logs")]
    if mode == AFFINE:
        shift, scale = O.split_cross(h)
        zc = torch.cat((z[:, :ns], z[:, ns:] * torch.exp(-O.logscale_of(scale)) - shift), 1)
    else:
        zc = torch.cat((z[:, :3] - h, z[:, 3:]), 1)
    y = _mat(torch.inverse(inp["W"].double()), zc) if inp["W"] is not None else zc
    x = y * torch.exp(-s) - b
    gx = inp["gout"].double()
    gz, gh, gb, gs, gzc = torch.autograd.grad((gx * x).sum(), [z, h, b, s, zc])
    ref = {"gz": ("v", gz), "gh": ("v", gh), "gzc": ("v", gzc), "y": ("v", y.detach()),
           "g_bias": ("s", inp["gb0"].double() + gb.flatten(), _chan(gx.abs()) + inp["gb0"].double().abs()),
           "g_logs": ("s", inp["gl0"].double() + gs.flatten(), _chan((gx * (x + b)).detach().abs()) + inp["gl0"].double().abs())}
    kin = dict(gx=inp["gout"], x=x.detach().float(), zc=zc.detach().float(), h=inp["h"], W=inp["W"], bias=inp["bias"],
               logs=inp["logs"], ns=ns, mode=mode, gb0=inp["gb0"], gl0=inp["gl0"], exact=dict(x=x.detach(), zc=zc.detach()))
    return kin, ref


def step_inverse_closed(k, dt):
    """StepInvBwdArgs: gy = gx e^-s, gzc = W^-T gy, coupling^-1 backward; y = (x + b) e^s; sums -gx and -gx (x + b)."""
    gx, x, zc, h, b, s = [_t(k, n, dt) for n in ("gx", "x", "zc", "h", "bias", "logs")]
    ns = k["ns"]
    xb = x + b
    y = xb * torch.exp(s)
    gy = gx * torch.exp(-s)
    gzc = _mat(torch.inverse(k["W"].double()).to(dt).t(), gy) if k["W"] is not None else gy
    if k["mode"] == AFFINE:
        shift, scale = h[:, 0::2], h[:, 1::2]
        e = torch.exp(-0.318 * torch.atan(2 * scale))
        gz = torch.cat((gzc[:, :ns], gzc[:, ns:] * e), 1)
        gls = -gzc[:, ns:] * (zc[:, ns:] + shift)
        gh = _interleave(-gzc[:, ns:], gls * (0.636 / (1 + 4 * scale * scale)))
    else:
        gz, gh = gzc, -gzc[:, :3]
    return {"gz": gz, "gh": gh, "gzc": gzc, "y": y, "g_bias": k["gb0"].to(dt) - _chan(gx), "g_logs": k["gl0"].to(dt) - _chan(gx * xb)}


# ---------------------------------------------------------------- Gaussian priors
PRIOR_CASES = [("logp", 0, True)] + [(kind, r, True) for kind in ("sample", "encode") for r in (0, 1)] + [("encode", 0, False),
                                                                                                          ("encode", 1, False)]


@functools.lru_cache(maxsize=None)
def prior_case(shape, kind, rescale, with_gz=True):
    """(mean, s) = h[:, 0::2], h[:, 1::2] drawn as test_gpu_flow_glue.py::_gauss_inputs does. logp: objective = log N(a; mean, e^s);
    sample: a = mean + e^logs eps with dL/da random; encode: z = (a - mean) e^-logs with dL/dz random (or absent: zero)."""
    b, C, H, W = shape
    g = _gen(7 + C + 100 * rescale + 1000 * ("logp", "sample", "encode").index(kind))
    mean = torch.randn(b, C, H, W, generator=g)
    s = torch.rand(b, C, H, W, generator=g) * 2 - 1
    x = torch.randn(b, C, H, W, generator=g)
    gout = torch.randn(b, C, H, W, generator=g)
    h32 = _interleave(mean, s)
    gobj = 0.6
    h = h32.double().requires_grad_(True)
    md, sd = O.split_cross(h)
    logs = O.logscale_of(sd) if rescale else sd
    if kind == "logp":
        a = x.double().requires_grad_(True)
        ga, gh = torch.autograd.grad(gobj * O.gaussian_logp(md, logs, a).sum(), [a, h])
        return dict(a=x, h=h32, ga=None, gz=None, gobj=gobj, rescale=rescale, kind=kind), {"ga": ("v", ga), "gh": ("v", gh)}
    if kind == "sample":
        a = O.gaussian_sample(md, logs, 0.8, (x * 0.8).double())
        gh, = torch.autograd.grad((gout.double() * a).sum(), [h])
        return (dict(a=a.detach().float(), h=h32, ga=gout, gz=None, gobj=gobj, rescale=rescale, kind=kind, exact=dict(a=a.detach())),
                {"gh": ("v", gh)})
    a = x.double().requires_grad_(True)
    z = (a - md) * torch.exp(-logs)
    if with_gz:
        ga, gh = torch.autograd.grad((gout.double() * z).sum(), [a, h])
    else:
        ga, gh = torch.zeros_like(a), torch.zeros_like(h)
    return dict(a=x, h=h32, ga=None, gz=gout if with_gz else None, gobj=gobj, rescale=rescale, kind=kind), {"ga": ("v", ga), "gh": ("v", gh)}


def prior_closed(k, dt):
    """PriorBwdArgs and the formulas beside its three launchers."""
    a, h = _t(k, "a", dt), _t(k, "h", dt)
    mean, s = h[:, 0::2], h[:, 1::2]
    dlogs = 0.636 / (1 + 4 * s * s) if k["rescale"] else 1.0
    if k["kind"] == "logp":                       # logp = -1/2 (2 logs + d^2 e^-2logs + ln 2pi), logs = s
        d, iv = a - mean, torch.exp(-2 * s)
        return {"ga": -k["gobj"] * d * iv, "gh": _interleave(k["gobj"] * d * iv, k["gobj"] * (d * d * iv - 1))}
    if k["kind"] == "sample":                     # d a / d logs = e^logs eps = a - mean
        ga = k["ga"].to(dt)
        return {"gh": _interleave(ga, ga * (a - mean) * dlogs)}
    gz = k["gz"].to(dt) if k["gz"] is not None else torch.zeros_like(a)
    logs = 0.318 * torch.atan(2 * s) if k["rescale"] else s
    e = torch.exp(-logs)
    return {"ga": gz * e, "gh": _interleave(-gz * e, -gz * ((a - mean) * e) * dlogs)}


# ---------------------------------------------------------------- Dirac-LR term with the straight-through Quant
@functools.lru_cache(maxsize=None)
def quant_case(b, H, W):
    """z = (k + u) / 255, integer k in [-20, 275], u uniform in +-0.4: no input near a rounding tie, both clamp sides hit."""
    g = _gen(b * 100 + H)
    kk = torch.randint(-20, 276, (b, 3, H, W), generator=g).double()
    u = (torch.rand(b, 3, H, W, generator=g).double() * 2 - 1) * 0.4
    z32 = ((kk + u) / 255).float()
    lr = torch.rand(b, 3, H, W, generator=g)
    gz0 = torch.randn(b, 3, H, W, generator=g) * 100
    gobj = -0.45
    assert float(z32.min()) < 0 and float(z32.max()) > 1
    z = z32.double().requires_grad_(True)
    q = z + ((torch.clamp(z, 0, 1) * 255.).round() / 255. - z).detach()           # Basic.Quant: backward the identity
    logp = O.gaussian_logp(q, torch.full_like(q, -6.0), lr.double())
    gz, = torch.autograd.grad(gobj * logp.sum(), [z])
    return dict(z=z32, lr=lr, gz0=gz0, gobj=gobj), {"gz": ("v", gz0.double() + gz)}


def quant_closed(k, dt):
    z, lr = k["z"].to(dt), k["lr"].to(dt)
    q = torch.round(torch.clamp(z, 0, 1) * 255) / 255
    e12 = torch.exp(torch.tensor(12.0, dtype=dt))
    return {"gz": k["gz0"].to(dt) + k["gobj"] * (lr - q) * e12}


# ---------------------------------------------------------------- output-gradient masks (bit-exact)
@functools.lru_cache(maxsize=None)
def mask_case():
    """z holds exact 0.0 and 1.0, the floats next to them on both sides and a NaN; (z, g, gz0, pass mask)."""
    b, C, H, W = 2, 3, 18, 15                    # 270 px: two blocks of the one-thread-per-pixel kernel
    g = _gen(5)
    z = torch.rand(b, C, H, W, generator=g) * 1.6 - 0.3
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    inf = torch.tensor(float("inf"))
    special = [0.0, 1.0, float(torch.nextafter(zero, -inf)), float(torch.nextafter(zero, inf)), float(torch.nextafter(one, zero)),
               float(torch.nextafter(one, inf)), float("nan"), -0.0]
    flat = z.view(-1)
    for i, v in enumerate(special * 3):         # spread over both samples, all channels, both blocks
        flat[(i * 67 + 11) % flat.numel()] = v
    grad = torch.randn(b, C, H, W, generator=g)
    gz0 = torch.randn(b, C, H, W, generator=g)
    keep = (z >= 0) & (z <= 1)
    assert bool(keep[z == 0].all()) and bool(keep[z == 1].all()) and not bool(keep[z != z].any())
    return z, grad, gz0, keep


# ---------------------------------------------------------------- conv epilogue
def epi_zy_mult(lay, act):
    """1 (ActNorm logs) or 3 (Conv2dZeros logs): both against every kernel form."""
    return 3.0 if (EPI_LAYOUTS.index(lay) + EPI_ACTS.index(act)) % 2 == 0 else 1.0


@functools.lru_cache(maxsize=None)
def epi_case(lay, act, res):
    """y = res2 + rs2 (res1 + rs1 act((acc + bias) scale)), scale = exp(m logs). The kernel's ``y`` is the activation's output
    (the conv's own output when it has no residual). sum_zy is defined without a residual and with act in {none, relu}."""
    b, H, W, n, cs, c0 = lay
    g = _gen(EPI_LAYOUTS.index(lay) * 9 + EPI_ACTS.index(act) * 3 + EPI_RES.index(res))
    acc32 = torch.randn(b, n, H, W, generator=g)
    bias32 = torch.randn(1, n, 1, 1, generator=g) * 0.1
    logs32 = torch.randn(1, n, 1, 1, generator=g) * 0.1
    if act == "relu":                            # exact zeros in y = relu(pre): pre = (acc + bias) scale = 0 exactly
        m0 = torch.rand(b, n, H, W, generator=g) < 0.1
        acc32 = torch.where(m0, -bias32.expand_as(acc32), acc32)
    gy = torch.randn(b, n, H, W, generator=g)
    r1 = torch.randn(b, n, H, W, generator=g)
    r2 = torch.randn(b, n, H, W, generator=g)
    g10 = torch.randn(b, n, H, W, generator=g)
    g20 = torch.randn(b, n, H, W, generator=g)
    sp0 = torch.randn(n, generator=g)
    sz0 = torch.randn(n, generator=g)
    m = epi_zy_mult(lay, act)
    want_zy = res == "none" and act in ("none", "relu")
    acc, bias, logs, res1, res2 = [t.double().requires_grad_(True) for t in (acc32, bias32, logs32, r1, r2)]
    scale = torch.exp(m * logs)
    pre = (acc + bias) * scale
    a = pre if act == "none" else F.relu(pre) if act == "relu" else F.leaky_relu(pre, 0.2)
    if act == "relu":
        assert int((a == 0).sum()) > int((pre < 0).sum())          # exact zeros beyond the clipped negatives
    if act == "lrelu":
        assert not bool((a == 0).any())
    y = a
    if res != "none":
        y = res1 + RS1 * y
    if res == "both":
        y = res2 + RS2 * y
    grads = torch.autograd.grad((gy.double() * y).sum(), [acc, bias, logs] + ([res1] if res != "none" else []) +
                                ([res2] if res == "both" else []))
    gpre = grads[0]
    ref = {"gpre": ("v", gpre), "sum_pre": ("s", sp0.double() + grads[1].flatten(), _chan(gpre.abs()) + sp0.double().abs())}
    if want_zy:                                  # dL/dlogs = m sum dz pre = m sum dz y (relu: dz != 0 only where y = pre)
        dz = gpre / scale
        ref["sum_zy"] = ("s", sz0.double() + grads[2].flatten(), m * _chan((dz * a).detach().abs()) + sz0.double().abs())
    if res != "none":
        ref["g1"] = ("v", g10.double() + grads[3])
    if res == "both":
        ref["g2"] = ("v", g20.double() + grads[4])
    kin = dict(gy=gy, y=a.detach().float(), scale=scale.detach().float().flatten(), act=act, res=res, g10=g10, g20=g20, sp0=sp0, sz0=sz0,
               m=m, want_zy=want_zy, cs=cs, c0=c0, exact=dict(y=a.detach(), scale=scale.detach().flatten()))
    return kin, ref


def epi_closed(k, dt):
    """EpiBwdArgs: g2 += gy; g1 += gy rs2; dz = gy rs2 rs1 act'(y); gpre = dz scale; the two sums."""
    gy, y = _t(k, "gy", dt), _t(k, "y", dt)
    sc = _t(k, "scale", dt).view(1, -1, 1, 1)
    k1 = RS2 if k["res"] == "both" else 1.0
    k2 = k1 * (RS1 if k["res"] != "none" else 1.0)
    dz = gy * k2
    if k["act"] == "relu":
        dz = torch.where(y > 0, dz, torch.zeros_like(dz))
    elif k["act"] == "lrelu":
        dz = torch.where(y >= 0, dz, dz * 0.2)
    gpre = dz * sc
    out = {"gpre": gpre, "sum_pre": k["sp0"].to(dt) + _chan(gpre)}
    if k["want_zy"]:
        out["sum_zy"] = k["sz0"].to(dt) + k["m"] * _chan(dz * y)
    if k["res"] != "none":
        out["g1"] = k["g10"].to(dt) + gy * k1
    if k["res"] == "both":
        out["g2"] = k["g20"].to(dt) + gy
    return out


# ---------------------------------------------------------------- LU chain
@functools.lru_cache(maxsize=None)
def lu_case(C):
    """W = P (l o mask + I)(u o mask^T + diag(sign_s exp(log_s))) (Permutations.py:78-86), loss = sum(dW o W)."""
    g = _gen(40 + C)
    l32 = torch.randn(C, C, generator=g) * 0.3
    u32 = torch.randn(C, C, generator=g) * 0.3
    log_s32 = torch.randn(C, generator=g) * 0.3
    sign = torch.where(torch.arange(C) % 3 == 1, -torch.ones(C), torch.ones(C)).double()
    P = torch.eye(C, dtype=torch.float64)[torch.randperm(C, generator=g)]
    dW = torch.randn(C, C, generator=g)
    dl0, du0, ds0 = torch.randn(C, C, generator=g), torch.randn(C, C, generator=g), torch.randn(C, generator=g)
    mask = torch.tril(torch.ones(C, C, dtype=torch.float64), -1)
    l, u, log_s = [t.double().requires_grad_(True) for t in (l32, u32, log_s32)]
    L = l * mask + torch.eye(C, dtype=torch.float64)
    U = u * mask.t() + torch.diag(sign * torch.exp(log_s))
    Wm = P @ L @ U
    gl, gu, gs = torch.autograd.grad((dW.double() * Wm).sum(), [l, u, log_s])
    ref = {"dl": ("v", dl0.double() + gl), "du": ("v", du0.double() + gu), "dlog_s": ("v", ds0.double() + gs)}
    kin = dict(dW=dW, P=P.float(), L=L.detach().float(), U=U.detach().float(), dl0=dl0, du0=du0, ds0=ds0,
               exact=dict(L=L.detach(), U=U.detach()))
    return kin, ref


def lu_closed(k, dt):
    """LuChainArgs: A = P^T dW; dl += strict_lower(A U'^T); du += strict_upper(L^T A); dlog_s[i] += (L^T A)[i][i] U'[i][i]."""
    dW, P, L, U = [_t(k, n, dt) for n in ("dW", "P", "L", "U")]
    A = P.t() @ dW
    M = L.t() @ A
    return {"dl": k["dl0"].to(dt) + torch.tril(A @ U.t(), -1), "du": k["du0"].to(dt) + torch.triu(M, 1),
            "dlog_s": k["ds0"].to(dt) + torch.diagonal(M) * torch.diagonal(U)}
