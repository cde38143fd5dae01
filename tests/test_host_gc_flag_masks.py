"""CPU-side check of the one bit the GC-ADPCM encoder's hot frame forms from its two overflows (gc_encode_core.hpp,
frame_goes_cold: four compares and lane-mask logic) against frame_flags, which the cold branch keeps deriving the single
flags from: for every tuple `cold == generic || resume || inexact`, fin_a equal, and for a cold lane the four flags the
branch hands to the cold block equal to frame_flags' own.  Host logic under test, not a product path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_flag_masks_driver.cpp")
HDR = os.path.join(HERE, "..", "vgaudio_amd", "csrc", "gc_encode_core.hpp")
SO = os.path.join(HERE, "host", "libgc_flag_masks_driver.so")

INTP = C.POINTER(C.c_int)
LLP = C.POINTER(C.c_longlong)
OVERFLOWS = [0, 1, 2, 3, 4, 247, 248, 249, 12384, 2 ** 31 - 1]
COLD, FIN_A_MASK, FIN_A, GENERIC, RESUME, INEXACT, BUMP_A, IN_GENERIC, IN_RESUME, IN_INEXACT, IN_BUMP_A = range(11)


@pytest.fixture(scope="module")
def drv():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off",
                        "-fno-fast-math", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    L.fm_check.argtypes = [C.c_int] * 5 + [INTP]
    L.fm_enumerate.argtypes = [INTP, C.c_int, LLP, INTP]
    return L


def _check(L, sp_a, ov_a, ov_2, coef_ok):
    out = np.zeros(11, np.int32)
    bits = L.fm_check(sp_a, min(sp_a + 1, 12), ov_a, ov_2, int(coef_ok), out.ctypes.data_as(INTP))
    return bits, out


def test_the_one_bit_equals_frame_flags_over_the_enumeration(drv):
    ovs = np.array(OVERFLOWS, np.int32)
    counts = np.zeros(7, np.int64)
    first = np.zeros(5, np.int32)
    bad = drv.fm_enumerate(ovs.ctypes.data_as(INTP), len(ovs), counts.ctypes.data_as(LLP), first.ctypes.data_as(INTP))
    assert bad == 0, ("first tuple that differs (sp_a, ov_a, ov_2, coef_ok, bits)", first.tolist())
    assert counts[0] == 13 * len(OVERFLOWS) ** 2 * 2
    # every kind of lane occurs, and none is all there is
    for i in range(1, 7):
        assert 0 < counts[i] < counts[0], (i, counts.tolist())


def test_the_python_restatement_agrees_tuple_by_tuple(drv):
    """the same enumeration with the expected flags written out here (frame_flags restated), so that a change to BOTH
    functions of the header is seen"""
    for sp_a in range(13):
        sp_b = min(sp_a + 1, 12)
        cap_a, cap_b = sp_a >= 12, sp_b >= 12
        for ov_a in OVERFLOWS:
            for ov_2 in OVERFLOWS:
                for ok in (False, True):
                    fin_a = cap_a or ov_a < 2
                    bump_a = not cap_a and ov_a > 248
                    bump_b = not fin_a and not cap_b and ov_2 > 248
                    generic = (not ok) or bump_a or bump_b
                    inexact = not generic and ((cap_a and ov_a > 3) if fin_a else (cap_b and ov_2 > 3))
                    resume = not generic and not fin_a and not cap_b and ov_2 >= 2
                    bits, out = _check(drv, sp_a, ov_a, ov_2, ok)
                    t = (sp_a, ov_a, ov_2, ok, out.tolist())
                    assert bits == 0, t
                    assert out[COLD] == int(generic or resume or inexact), t
                    assert out[FIN_A_MASK] == int(fin_a) and out[FIN_A] == int(fin_a), t
                    if out[COLD]:
                        assert [out[IN_GENERIC], out[IN_RESUME], out[IN_INEXACT], out[IN_BUMP_A]] == \
                               [int(generic), int(resume), int(inexact), int(bump_a)], t
                    else:
                        assert not (out[IN_GENERIC] or out[IN_RESUME] or out[IN_INEXACT] or out[IN_BUMP_A]), t


@pytest.mark.parametrize("sp_a,ov_a,ov_2,ok,cold,fin_a", [
    (5, 1, 0, True, 0, 1),             # A final below the cap
    (5, 2, 1, True, 0, 0),             # B final
    (5, 2, 2, True, 1, 0),             # both overflowed: resume
    (5, 248, 1, True, 0, 0),           # the largest overflow without a bump
    (5, 249, 0, True, 1, 0),           # bump_a
    (5, 2, 249, True, 1, 0),           # bump_b
    (11, 2, 3, True, 0, 0),            # B at the cap: up to 3 is exact
    (11, 2, 4, True, 1, 0),            # ... 4 is inexact
    (12, 3, 2 ** 31 - 1, True, 0, 1),  # A at the cap ends the loop; ov_2 is its own overflow in the kernel, unread here
    (12, 4, 4, True, 1, 1),            # inexact at the cap
    (0, 0, 0, False, 1, 1),            # hostile coefficients: always cold
])
def test_named_cases(drv, sp_a, ov_a, ov_2, ok, cold, fin_a):
    bits, out = _check(drv, sp_a, ov_a, ov_2, ok)
    assert bits == 0 and out[COLD] == cold and out[FIN_A_MASK] == fin_a, out.tolist()
