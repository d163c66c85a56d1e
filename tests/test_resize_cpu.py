"""CPU checks of the bicubic resize (include/hcflow.h: hcf_resize_*; hcflow_amd/resize.py): the oracle against the reference's
recorded outputs, the library's host tables against the oracle, the argument checks that run before anything touches a device,
and the Python surface. No compute calls."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from hcflow_amd import _lib, latent, resize
from tests import resize_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hcf_resize_workspace", "hcf_resize_bicubic", "hcf_resize_bicubic_backward", "hcf_resize_tables"]
ERR_ARG, ERR_SHAPE = -1, -5
# every (in_len, s, up) of the cases' axes, and the lengths 1, 2 and 2040 at each case's factor
AXES = sorted({(n, s, up) for H, W, s, up in O.CASES for n in (H, W, 1, 2, 2040)})


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "imresize_float.npz"))


def lib_table(n, s, up, transposed):
    """(L, w [rows, L] float64, idx [rows, L], cnt [rows]) of hcf_resize_tables."""
    lib = _lib.load()
    L = lib.hcf_resize_tables(n, s, up, transposed, None, None, None, 0)
    assert L > 0, (n, s, up, transposed, L)
    rows = n if transposed else O.out_len(n, s, up)
    w = np.zeros((rows, L), dtype=np.float64)
    idx = np.zeros((rows, L), dtype=np.int32)
    cnt = np.zeros(rows, dtype=np.int32)
    got = lib.hcf_resize_tables(n, s, up, transposed, w.ctypes.data, idx.ctypes.data, cnt.ctypes.data, rows * L)
    assert got == L
    return L, w, idx, cnt


def dense(w, idx, n):
    """Lists [rows, L] scattered into [rows, n], taps added in order (mirrored taps on one index add up)."""
    A = np.zeros((w.shape[0], n))
    for o in range(w.shape[0]):
        np.add.at(A[o], idx[o], w[o])
    return A


def test_symbols_declared_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "hcflow.h")).read()
    declared = set(re.findall(r"\b(hcf_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert "utils/imresize.py" in hdr[hdr.index("hcf_resize.hip"):]


@pytest.mark.parametrize("case", O.CASES, ids=lambda c: O.case_name(*c))
def test_oracle_matches_the_reference(golden, case):
    H, W, s, up = case
    x, y = golden["x_" + O.case_name(*case)], golden["y_" + O.case_name(*case)]
    assert x.shape == (3, H, W) and x.dtype == np.float64 and x.min() >= 0 and x.max() < 1
    assert y.shape == (3, O.out_len(H, s, up), O.out_len(W, s, up)) and y.dtype == np.float64
    assert np.abs(O.forward(x, s, up) - y).max() <= 1e-12


def test_oracle_backward_is_the_transpose():
    rng = np.random.RandomState(3)
    for H, W, s, up in O.CASES:
        x = rng.random_sample((2, H, W))
        g = rng.standard_normal((2, O.out_len(H, s, up), O.out_len(W, s, up)))
        lhs, rhs = (O.forward(x, s, up) * g).sum(), (x * O.backward(g, H, W, s, up)).sum()
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_fp32_restatement_is_close_to_the_oracle(golden):
    for case in O.CASES:
        H, W, s, up = case
        x = golden["x_" + O.case_name(*case)]
        ref = O.forward(x.astype(np.float32), s, up)
        bound, e32 = O.gate(ref, O.forward32(x, s, up))
        assert 0 < e32 < 1e-6 and bound < 1e-5, (case, e32)
        g = np.random.RandomState(5).standard_normal(ref.shape).astype(np.float32)
        refb = O.backward(g, H, W, s, up)
        _, e32b = O.gate(refb, O.backward32(g, H, W, s, up))
        assert 0 < e32b < 1e-5, (case, e32b)


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "n%d_s%d_%s" % (a[0], a[1], "up" if a[2] else "down"))
def test_forward_tables_match_the_oracle(axis):
    n, s, up = axis
    L, w, idx, cnt = lib_table(n, s, up, 0)
    ow, oi = O.taps(n, s, up)
    assert L == ow.shape[1] == int(np.ceil(4 * max(1.0, 1.0 / O.scale_of(s, up)))) + 2
    assert (cnt == L).all() and (idx == oi).all()
    assert np.abs(w - ow).max() <= 1e-15
    for lo in range(0, w.shape[0], 512):                           # dense, 512 output rows at a time (2040 x8 is 16320 x 2040)
        assert np.abs(dense(w[lo:lo + 512], idx[lo:lo + 512], n) - dense(ow[lo:lo + 512], oi[lo:lo + 512], n)).max() <= 1e-15
    if n <= 64:
        assert np.abs(dense(w, idx, n) - O.matrix(n, s, up)).max() <= 1e-15
    assert np.abs(w.sum(axis=1) - 1).max() <= 1e-15


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "n%d_s%d_%s" % (a[0], a[1], "up" if a[2] else "down"))
def test_transposed_tables_are_the_forward_tables_permuted(axis):
    n, s, up = axis
    P, w, idx, _ = lib_table(n, s, up, 0)
    L, wt, it, ct = lib_table(n, s, up, 1)
    assert wt.shape[0] == n and L == ct.max() and ct.sum() == w.size
    # row i = the entries (o, k) with idx[o, k] == i in ascending (o, k) order, the SAME float64 values
    for i in range(n):
        o_, k_ = np.nonzero(idx == i)                               # row-major: ascending (o, k)
        c = int(ct[i])
        assert c == len(o_)
        assert (it[i, :c] == o_).all() and (wt[i, :c] == w[o_, k_]).all()
        assert (it[i, c:] == -1).all() and (wt[i, c:] == 0).all()
    # scattered into a dense matrix they are A^T exactly (per element the same additions in the same order as the forward scatter)
    if n <= 64:
        A = np.zeros((w.shape[0], n))
        for o in range(w.shape[0]):
            for k in range(P):
                A[o, idx[o, k]] += w[o, k]
        At = np.zeros((n, w.shape[0]))
        for i in range(n):
            for e in range(int(ct[i])):
                At[i, it[i, e]] += wt[i, e]
        assert (At == A.T).all() and (A == dense(w, idx, n)).all()


def test_tables_entry_checks_its_arguments():
    fn = _lib.load().hcf_resize_tables
    n = None
    for bad in [(0, 4, 0, 0), (-3, 4, 0, 0), (8, 1, 0, 0), (8, 9, 1, 0), (8, 4, 2, 0), (8, 4, 0, 2), (8, 4, -1, 0)]:
        assert fn(*bad, n, n, n, 0) == ERR_ARG, bad
    w = (C.c_double * 64)()
    i = (C.c_int32 * 64)()
    assert fn(8, 4, 0, 0, w, n, n, 64) == ERR_ARG and fn(8, 4, 0, 0, n, i, i, 64) == ERR_ARG       # all three or none
    assert fn(8, 4, 0, 0, w, i, i, 2 * 18 - 1) == ERR_SHAPE                                         # 2 rows x 18 taps
    assert fn(8, 4, 0, 0, w, i, i, 2 * 18) == 18
    assert fn(2 ** 31 - 1, 8, 1, 0, n, n, n, 0) == ERR_SHAPE


def test_workspace_query():
    fn = _lib.load().hcf_resize_workspace
    for bad in [(0, 3, 8, 8, 4, 0), (1, 0, 8, 8, 4, 0), (1, 3, 0, 8, 4, 0), (1, 3, 8, 0, 4, 0), (1, 3, 8, 8, 1, 0),
                (1, 3, 8, 8, 9, 1), (1, 3, 8, 8, 4, 2), (1, 3, 8, 8, 4, -1), (-1, 3, 8, 8, 4, 0)]:
        assert fn(*bad) == 0, bad
    assert fn(2, 3, 13, 18, 4, 0) == 2 * 3 * 4 * 18 * 4            # the [B, C, Ho, W] fp32 intermediate
    assert fn(2, 3, 5, 7, 4, 1) == 2 * 3 * 20 * 7 * 4
    assert fn(5, 3, 40, 33, 8, 0) == 5 * fn(1, 3, 40, 33, 8, 0)
    big = 2 ** 31 - 1
    assert fn(big, big, big, big, 2, 0) == 0 and fn(1, 1, big, 8, 2, 1) == 0 and fn(big, big, 64, 64, 4, 1) == 0


@pytest.mark.parametrize("name", NAMES[1:3])
def test_launching_entries_check_their_arguments_before_any_device_call(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    B, Cc, H, W, s = 2, 3, 13, 18, 4
    p = C.c_void_p(4096)                       # never dereferenced: every call below is refused first
    n = None
    wb = lib.hcf_resize_workspace(B, Cc, H, W, s, 0)

    def call(x=p, B=B, Cc=Cc, H=H, W=W, s=s, up=0, y=p, work=p, nbytes=wb):
        return fn(x, B, Cc, H, W, s, up, y, work, nbytes, n)
    assert call(x=n) == ERR_ARG and call(y=n) == ERR_ARG and call(work=n) == ERR_ARG
    assert call(B=0) == ERR_ARG and call(Cc=0) == ERR_ARG and call(H=0) == ERR_ARG and call(W=-1) == ERR_ARG
    assert call(s=1) == ERR_ARG and call(s=9) == ERR_ARG and call(s=0) == ERR_ARG and call(up=2) == ERR_ARG
    assert call(nbytes=wb - 1) == ERR_SHAPE and call(nbytes=0) == ERR_SHAPE
    assert call(up=1, nbytes=wb) == ERR_SHAPE                      # the up-scaling intermediate is larger
    big = 2 ** 31 - 1
    assert call(B=big, Cc=big, H=big, W=big, nbytes=2 ** 63) == ERR_SHAPE        # element counts leave int64
    assert call(H=big, up=1, nbytes=2 ** 63) == ERR_SHAPE                        # output side beyond int32


def test_scale_parsing():
    assert resize.parse_scale(4) == (4, 1) and resize.parse_scale(2) == (2, 1) and resize.parse_scale(8) == (8, 1)
    assert resize.parse_scale(0.25) == (4, 0) and resize.parse_scale(1 / 3) == (3, 0) and resize.parse_scale(Fraction(1, 8)) == (8, 0)
    assert resize.parse_scale(0.5 + 1e-11) == (2, 0)
    for bad in [1, 9, 0, -4, 4.0, 1.0, 0.3, 0.25 + 1e-6, 1 / 9, Fraction(2, 3), Fraction(1, 9), "4", None, True, float("nan"), 0.0,
                float("inf")]:
        with pytest.raises(ValueError):
            resize.parse_scale(bad)
    assert [resize.out_size(n, 4, 0) for n in (1, 4, 5, 13, 18)] == [1, 1, 2, 4, 5] and resize.out_size(5, 3, 1) == 15


def test_python_surface_refuses_without_a_fallback(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine call was made")
    x = torch.rand(1, 3, 8, 8)
    monkeypatch.setattr(_lib, "launch", no_engine)
    for bad in (3.0, 0.3, 9, "x"):
        with pytest.raises(ValueError):
            resize.imresize(x, bad)
        with pytest.raises(ValueError):
            latent.lr_consistency(x, bad)
    with pytest.raises(ValueError):
        latent.lr_consistency(x, 4, kind="huber")
    with pytest.raises(ValueError):
        resize.lr_psnr(x, x, 0.25)
    with pytest.raises(_lib.HcfError):
        resize.imresize(x, 0.25)                                   # a CPU tensor
    with pytest.raises(_lib.HcfError):
        resize.imresize(x.numpy(), 0.25)
    with pytest.raises(_lib.HcfError):
        latent.lr_consistency(x, 4)                                # a CPU lq
    with pytest.raises(_lib.HcfError):
        resize.lr_psnr(x, x, 4)
    import hcflow_amd
    assert hcflow_amd.imresize is resize.imresize and hcflow_amd.lr_psnr is resize.lr_psnr
