"""The order in which a conv call tries the kernel families, pinned without a GPU: hcf_debug_conv_route lists what route_conv
(hcflow_amd/csrc/hcf_conv_route.hip) would try for the packs a caller has and the forms it admits, and launches nothing. The engine's
forward and data-gradient convs, the per-op entries and the auxiliary nets all launch through that one function; the expected lists
below are the order written out by hand:
  1. Winograd: a Winograd pack, no fused tail, no fused second layer unless its Winograd fragment is there, ablation 256 off;
  2. with an f16x3 pack and 3x3 taps (or a 1x1 that fuses nothing): fcn12 when a second layer is fused and no tail, then f16x3, then
     -- the 1x1 only -- exact;
  3. otherwise exact.
A form whose pack is missing is never tried, the exact form included."""
import ctypes as C

import pytest

from hcflow_amd import _lib

WINO, FCN12, F16X3, EXACT = 0, 1, 2, 3
P_EXACT, P_F16, P_WINO, P_F16_2, P_FRAG2 = 1, 2, 4, 8, 16
ALL = 15
NO_WINO = 256      # hcf_debug_set_ablation: no Winograd kernels


def only(*forms):
    return sum(1 << f for f in forms)


# name, taps, packs, tail, allow, ablation, expected forms
CASES = [
    ("plain 3x3, all packs", 9, P_EXACT | P_F16 | P_WINO, 0, ALL, 0, [WINO, F16X3]),
    ("plain 3x3, all packs, no Winograd", 9, P_EXACT | P_F16 | P_WINO, 0, ALL, NO_WINO, [F16X3]),
    ("1x1, f16 and exact packs", 1, P_EXACT | P_F16, 0, ALL, 0, [F16X3, EXACT]),
    ("fused second layer with its fragment", 9, P_EXACT | P_F16 | P_WINO | P_F16_2 | P_FRAG2, 0, ALL, 0, [WINO, FCN12, F16X3]),
    ("fused second layer without the fragment", 9, P_EXACT | P_F16 | P_WINO | P_F16_2, 0, ALL, 0, [FCN12, F16X3]),
    ("fused tail", 9, P_EXACT | P_F16 | P_WINO, 1, ALL, 0, [F16X3]),
    ("fat call: the Winograd pack only, Winograd only", 9, P_WINO, 0, only(WINO), 0, [WINO]),
    ("fat call with the fused second layer", 9, P_WINO | P_F16_2 | P_FRAG2, 0, only(WINO), 0, [WINO]),
    ("fat call, no Winograd: nothing to launch", 9, P_WINO, 0, only(WINO), NO_WINO, []),
    ("pre-activation call: fcn12 or nothing", 9, P_EXACT | P_F16 | P_F16_2, 0, only(FCN12), 0, [FCN12]),
    ("no f16 pack at all", 9, P_EXACT, 0, ALL, 0, [EXACT]),
    ("no f16 pack at all, 1x1", 1, P_EXACT, 0, ALL, 0, [EXACT]),
    ("data gradient: the scaled forms only", 9, P_F16 | P_WINO, 0, only(WINO, F16X3), 0, [WINO, F16X3]),
    ("data gradient of a 1x1: no exact launch inside the router", 1, P_F16, 0, only(WINO, F16X3), 0, [F16X3]),
    ("the Winograd pack only, every form admitted: no exact launch without an exact pack", 9, P_WINO, 0, ALL, 0, [WINO]),
    ("1x1, the f16 pack only: no exact launch without an exact pack", 1, P_F16, 0, ALL, 0, [F16X3]),
    ("no pack at all: nothing to launch", 9, 0, 0, ALL, 0, []),
    ("1x1 with a fused tail falls to exact", 1, P_EXACT | P_F16, 1, ALL, 0, [EXACT]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_forms_in_order(case):
    _, taps, packs, tail, allow, ablation, want = case
    lib = _lib.load()
    forms = (C.c_int32 * 4)()
    assert lib.hcf_debug_set_ablation(ablation) == 0
    try:
        n = lib.hcf_debug_conv_route(taps, packs, tail, allow, forms, 4)
    finally:
        assert lib.hcf_debug_set_ablation(0) == 0
    assert n == len(want)
    assert list(forms) == want + [-1] * (4 - len(want))


def test_debug_entry_rejects_bad_calls():
    lib = _lib.load()
    forms = (C.c_int32 * 4)()
    assert lib.hcf_debug_conv_route(9, P_EXACT, 0, ALL, None, 4) == -1
    assert lib.hcf_debug_conv_route(9, P_EXACT, 0, ALL, forms, 3) == -1
    assert lib.hcf_debug_conv_route(4, P_EXACT, 0, ALL, forms, 4) == -1
    assert lib.hcf_debug_conv_route(9, 32, 0, ALL, forms, 4) == -1
    assert lib.hcf_debug_conv_route(9, P_EXACT, 0, 16, forms, 4) == -1
