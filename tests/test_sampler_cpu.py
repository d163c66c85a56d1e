"""The host reference of the device sampler (tests/philox_ref.py) against published Philox4x32-10 vectors, and the statistics
of its normal draws. No GPU: tests/test_gpu_sampler.py holds the kernel against this reference."""
import functools

import numpy as np
import pytest

from tests import philox_ref as R

# counter, key -> output (the Random123 known-answer vectors of philox4x32-10: zeros, all ones, digits of pi)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

N = 1 << 18          # 2.6e5 draws: 1 / sqrt(N) = 0.002, the gates below are 5 sigma (kurtosis: sqrt(96 / N) = 0.019, 2.6 sigma)
SEED = 123


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = tuple(int(v) for v in R.philox4x32_10(counter, key))
    assert got == want, [hex(v) for v in got]


def test_philox_vectorised_equals_scalar():
    """Array counters / keys give the per-element scalar results (the GPU tests evaluate whole tensors at once)."""
    cs = np.array([k[0] for k in KAT], dtype=np.uint64).T
    ks = np.array([k[1] for k in KAT], dtype=np.uint64).T
    got = np.stack(R.philox4x32_10(tuple(cs), tuple(ks)), 1)
    assert got.tolist() == [list(k[2]) for k in KAT]


@functools.lru_cache(maxsize=None)
def _draws(seed, offset, start=0):
    x = R.normal(seed, offset, np.arange(start, start + N, dtype=np.uint64))
    x.setflags(write=False)
    return x


def _corr(a, b):
    a = a.astype(np.float64) - a.mean(dtype=np.float64)
    b = b.astype(np.float64) - b.mean(dtype=np.float64)
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_normal_moments():
    x = _draws(SEED, 0).astype(np.float64)
    assert x.shape == (N,) and np.isfinite(x).all()
    assert float(np.abs(x).max()) <= 5.9
    mean, std = float(x.mean()), float(x.std())
    kurt = float(((x - mean) ** 4).mean() / std ** 4)
    print("normal: mean %.5f std %.5f kurtosis %.4f" % (mean, std, kurt))
    assert abs(mean) < 0.01 and abs(std - 1.0) < 0.01 and abs(kurt - 3.0) < 0.05


def test_normal_streams_are_uncorrelated():
    x = _draws(SEED, 0)
    c = {"offsets 0 / 1": _corr(x, _draws(SEED, 1)),
         "seeds s / s + 1": _corr(x, _draws(SEED + 1, 0)),
         "seeds s / s + 2^32": _corr(x, _draws(SEED + (1 << 32), 0)),
         "lag 1": _corr(x[:-1], x[1:])}
    print("normal: correlations", c)
    for k, v in c.items():
        assert abs(v) < 0.01, (k, v)


def test_every_counter_and_key_word_changes_the_draw():
    """idx and offset high words, seed high word: each enters the generator (the values differ from the low-word-only draw)."""
    idx = np.arange(64, dtype=np.uint64)
    base = R.normal(5, 0, idx)
    assert not np.array_equal(base, R.normal(5 + (1 << 32), 0, idx))
    assert not np.array_equal(base, R.normal(5, 1 << 32, idx))
    assert not np.array_equal(base, R.normal(5, 0, idx + np.uint64(1 << 32)))
    assert not np.array_equal(base, R.normal(5, 1, idx))
    assert np.array_equal(base, R.normal(5 + (1 << 64), 0, idx))          # the seed is a 64-bit value


def test_normal_float32_restatement_is_close_to_float64():
    """The float32 Box-Muller against float64 on the same uniforms: rounding the cosine's argument 2 pi u2 to float32 moves
    it by at most ulp(6.28) / 2 = 2.4e-7, times the radius (<= 5.9) = 1.4e-6; log, sqrt and cos add a few float32 ulp of the
    draw (ulp(5.9) = 4.8e-7). 3e-6 bounds the sum; the GPU gate (1e-5) leaves room for the device's own libm on top."""
    idx = np.arange(N, dtype=np.uint64)
    w0, w1, _, _ = R.philox4x32_10((idx, 0, 0, 0), (SEED, 0))
    u1 = ((w0 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u2 = ((w1 >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    ref = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
    d = float(np.abs(_draws(SEED, 0).astype(np.float64) - ref).max())
    print("normal: float32 vs float64 max deviation %.3e" % d)
    assert d <= 3e-6


def test_level_eps_protocol():
    """level_eps: shapes of config.eps_shapes, stream d for draw d, NCHW element index, shards continue the full batch's rows."""
    from hcflow_amd.config import preset, eps_shapes
    cfg = preset("SR_8X_tiny")
    full = R.level_eps(cfg, 3, 4, 6, 0.8, 77)
    shapes = eps_shapes(cfg, 3, 4, 6)
    assert [e.shape for e in full] == [tuple(s) for s in shapes] and all(e.dtype == np.float32 for e in full)
    part = R.level_eps(cfg, 2, 4, 6, 0.8, 77, first_sample=1)
    for d, (f, p) in enumerate(zip(full, part)):
        assert np.array_equal(f[1:], p)
        B, C, H, W = f.shape
        b, c, y, x = 2, C - 1, H - 1, W - 2
        want = np.float32(0.8) * R.normal(77, d, ((b * C + c) * H + y) * W + x)
        assert f[b, c, y, x] == want
    assert not np.array_equal(full[0], R.sample_eps(full[0].shape, 0.8, 77, offset=1))
