"""Oracle of the MATLAB-bicubic resize (hcflow_amd/resize.py): the rule as dense float64 matrices in numpy, written from the
rule's statement (utils/imresize.py: contributions, cubic), independently of the library's table builder.

Per axis ``A`` [out_len, in_len]: output o (0-based) sits at u = (o + 1) / scale + 0.5 (1 - 1 / scale) (1-based source
coordinate), reads P = ceil(4 max(1, 1 / scale)) + 2 taps from left = floor(u - kw / 2) on, weights scale * cubic(scale * t) when
down-scaling and cubic(t) when up-scaling, each row normalised to sum 1, indices mirrored through aux = [0..n-1, n-1..0] modulo
2n. ``forward`` = A_h x A_w^T, ``backward`` = A_h^T g A_w. ``forward32`` / ``backward32`` restate the device arithmetic in fp32
on the CPU (fp32 weights, one accumulator per element, taps in order; numpy has no fma, so each step rounds twice): their
deviation from the float64 oracle is the ``e32`` of the GPU gates.
"""
import math

import numpy as np

# (H, W, s, up): the fixture's cases (tests/golden/make_resize_golden.py)
CASES = [(3, 5, 4, 0), (13, 18, 4, 0), (16, 24, 2, 0), (17, 9, 3, 0), (40, 33, 8, 0),
         (5, 7, 4, 1), (3, 2, 8, 1), (9, 6, 2, 1), (4, 5, 3, 1)]


def case_name(H, W, s, up):
    return "%dx%d_%s%d" % (H, W, "up" if up else "down", s)


def scale_of(s, up):
    return float(s) if up else 1.0 / s


def out_len(n, s, up):
    return n * s if up else -(-n // s)


def cubic(x):
    ax = np.abs(np.asarray(x, dtype=np.float64))
    ax2, ax3 = ax * ax, ax * ax * ax
    return (1.5 * ax3 - 2.5 * ax2 + 1) * (ax <= 1) + (-0.5 * ax3 + 2.5 * ax2 - 4 * ax + 2) * ((1 < ax) & (ax <= 2))


def taps(n, s, up):
    """(weights [out, P] float64, indices [out, P] int): every tap kept, in tap order, mirrored."""
    scale = scale_of(s, up)
    m = out_len(n, s, up)
    kw = 4.0 / scale if scale < 1 else 4.0
    P = int(math.ceil(kw)) + 2
    u = np.arange(1, m + 1, dtype=np.float64) / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kw / 2)
    ind = (left[:, None] + np.arange(P) - 1).astype(np.int64)
    t = u[:, None] - ind - 1
    w = scale * cubic(scale * t) if scale < 1 else cubic(t)
    w = w / w.sum(axis=1, keepdims=True)
    aux = np.concatenate([np.arange(n), np.arange(n - 1, -1, -1)])
    return w, aux[np.mod(ind, 2 * n)]


def matrix(n, s, up):
    """A [out_len, in_len] float64 (mirrored taps on one index add up)."""
    w, idx = taps(n, s, up)
    A = np.zeros((w.shape[0], n), dtype=np.float64)
    for o in range(w.shape[0]):
        np.add.at(A[o], idx[o], w[o])
    return A


def forward(x, s, up):
    """x [..., H, W] float64 -> [..., Ho, Wo] float64."""
    x = np.asarray(x, dtype=np.float64)
    Ah, Aw = matrix(x.shape[-2], s, up), matrix(x.shape[-1], s, up)
    return Ah @ x @ Aw.T


def backward(g, H, W, s, up):
    """g [..., Ho, Wo] float64 -> [..., H, W]: the transpose of ``forward`` at input size (H, W)."""
    g = np.asarray(g, dtype=np.float64)
    return matrix(H, s, up).T @ g @ matrix(W, s, up)


def _chain32(src, w, idx, axis):
    """One pass of the device arithmetic along ``axis`` (-2 or -1) in fp32: acc = acc + w_k * src[idx_k], k ascending."""
    w32 = w.astype(np.float32)
    src = np.moveaxis(np.asarray(src, dtype=np.float32), axis, -1)
    acc = np.zeros(src.shape[:-1] + (w.shape[0],), dtype=np.float32)
    for k in range(w.shape[1]):
        acc = (acc + w32[:, k] * src[..., idx[:, k]]).astype(np.float32)
    return np.moveaxis(acc, -1, axis)


def forward32(x, s, up):
    wh, ih = taps(x.shape[-2], s, up)
    ww, iw = taps(x.shape[-1], s, up)
    return _chain32(_chain32(x, wh, ih, -2), ww, iw, -1)


def transposed_lists(n, s, up):
    """Per input index the [(output, weight)] entries in ascending (output, tap) order."""
    w, idx = taps(n, s, up)
    rows = [[] for _ in range(n)]
    for o in range(w.shape[0]):
        for k in range(w.shape[1]):
            rows[idx[o, k]].append((o, w[o, k]))
    return rows


def _chain32_t(src, rows, axis):
    src = np.moveaxis(np.asarray(src, dtype=np.float32), axis, -1)
    out = np.zeros(src.shape[:-1] + (len(rows),), dtype=np.float32)
    for i, ent in enumerate(rows):
        acc = np.zeros(src.shape[:-1], dtype=np.float32)
        for o, wv in ent:
            acc = (acc + np.float32(wv) * src[..., o]).astype(np.float32)
        out[..., i] = acc
    return np.moveaxis(out, -1, axis)


def backward32(g, H, W, s, up):
    """Columns first, as the device does."""
    return _chain32_t(_chain32_t(g, transposed_lists(W, s, up), -1), transposed_lists(H, s, up), -2)


def gate(ref64, restated32):
    """The GPU tests' bound for a case: max(8 e32, 2^-23 max|ref|), e32 = max|fp32 CPU restatement - float64 oracle|."""
    e32 = float(np.abs(np.asarray(restated32, dtype=np.float64) - ref64).max())
    return max(8.0 * e32, 2.0 ** -23 * float(np.abs(ref64).max())), e32
