"""Host reference of the device sampler (hcflow_amd/csrc/hcf_flow.hip: philox_normal, gauss_sample_kernel), numpy only.

``philox4x32_10`` is the textbook Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11);
``normal`` restates the kernel's arithmetic after the generator in float32; ``level_eps`` lists the draws of one inverse pass.
"""
import numpy as np

_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = np.uint64(0x9E3779B9)
_W1 = np.uint64(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _u32(x):
    """A 32-bit word (or an array of them) held in uint64, so that a 32 x 32 product stays exact."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64) & _LO
    return np.uint64(int(x) & 0xFFFFFFFF)


def philox4x32_10(counter4, key2):
    """Ten rounds on the counter (c0, c1, c2, c3) under the key (k0, k1): four 32-bit output words (uint64 holders).
    The words may be scalars or arrays that broadcast against each other."""
    c0, c1, c2, c3 = [_u32(c) for c in counter4]
    k0, k1 = [_u32(k) for k in key2]
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0 = (k0 + _W0) & _LO
        k1 = (k1 + _W1) & _LO
    return c0, c1, c2, c3


def _split64(x):
    """(low word, high word) of a 64-bit value: a python int or a uint64 array."""
    if isinstance(x, np.ndarray):
        x = x.astype(np.uint64)
        return x & _LO, x >> _S32
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x & 0xFFFFFFFF, x >> 32


def normal(seed, offset, idx):
    """The standard-normal draw of element ``idx`` of stream ``offset`` under ``seed``, as float32 (Box-Muller on the first
    two output words): counter = (idx lo, idx hi, offset lo, offset hi), key = (seed lo, seed hi),
    u = (float32(word >> 8) + 0.5) * 2^-24, draw = sqrt(-2 ln u1) * cos(float32(2 pi) * u2).

    u1 can round to exactly 1.0 (word >> 8 = 2^24 - 1: the sum 2^24 - 0.5 is not a float32), which gives ln u1 = 0 and a draw
    of 0: harmless, one value in 2^24 lands on the mode. The smallest u1 is 2^-25, so |draw| <= sqrt(50 ln 2) < 5.9."""
    i_lo, i_hi = _split64(idx)
    o_lo, o_hi = _split64(offset)
    s_lo, s_hi = _split64(seed)
    w0, w1, _, _ = philox4x32_10((i_lo, i_hi, o_lo, o_hi), (s_lo, s_hi))
    f = np.float32
    scale = f(1.0 / 16777216.0)
    u1 = (np.asarray(w0 >> np.uint64(8)).astype(f) + f(0.5)) * scale
    u2 = (np.asarray(w1 >> np.uint64(8)).astype(f) + f(0.5)) * scale
    r = np.sqrt(f(-2.0) * np.log(u1))
    out = r * np.cos(f(6.28318530717958647692) * u2)
    assert out.dtype == np.float32
    return out


def sample_eps(shape, tau, seed, offset=0, first_sample=0):
    """tau * normal for every element of an NCHW tensor of ``shape``: idx = NCHW flat index + first_sample * C * H * W."""
    B, C, H, W = [int(v) for v in shape]
    n = C * H * W
    idx = np.arange(B * n, dtype=np.uint64) + np.uint64(int(first_sample) * n)
    return (np.float32(tau) * normal(seed, offset, idx)).reshape(B, C, H, W)


def level_eps(cfg, B, h, w, tau, seed, first_sample=0):
    """The draws of one inverse pass on a B x 3 x h x w LR batch, as hcf_inverse makes them on the device: shapes from
    config.eps_shapes (deepest level first), draw d from stream ``offset = d``, the rows of global samples
    [first_sample, first_sample + B)."""
    from hcflow_amd.config import eps_shapes
    return [sample_eps(s, tau, seed, d, first_sample) for d, s in enumerate(eps_shapes(cfg, B, h, w))]
