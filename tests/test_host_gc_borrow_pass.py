"""CPU-side check of the GC-ADPCM encoder's quantise pass that takes its rounding sign from the subtract's borrow
(gc_encode_core.hpp, pass_fast_core_b, B1-B5): the header is compiled for the host with a small driver and the pass, rounded
and no-round, is compared with pass_fast_core_t on EVERY frame whose coefficients satisfy |c0| + |c1| <= 30720 -- nibbles mod
16 and as q2 + Z, packed history, error sum, overflow -- whether or not either pass vouches for itself: both are plain
integer arithmetic.  Beyond the bound the new pass must say exact == false.  Host logic under test, not a product path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_host_gc_packed_pass import ORDINARY, _rail_frames

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_borrow_pass_driver.cpp")
HDR = os.path.join(HERE, "..", "vgaudio_amd", "csrc", "gc_encode_core.hpp")
SO = os.path.join(HERE, "host", "libgc_borrow_pass_driver.so")

VARIANTS = {"rounded": 0, "no_round": 1}
I16P = C.POINTER(C.c_int16)
INTP = C.POINTER(C.c_int)
LLP = C.POINTER(C.c_longlong)
BOUND = 30720

ON_BOUND = [(30720, 0), (0, -30720), (-15360, -15360), (-28672, 2048)]
PAST_BOUND = [(30721, 0), (-15360, -15361)]
FAR = [(32767, 0), (0, 32767), (-32768, -32768), (32767, -32768), (20000, 20000)]
SCALES = list(range(13))


@pytest.fixture(scope="module")
def drv():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off",
                        "-fno-fast-math", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    L.bp_compare.argtypes = [I16P, C.c_int, C.c_int, C.c_int, C.c_int]
    L.bp_compare_many.argtypes = [I16P, INTP, INTP, INTP, C.c_int, C.c_int, LLP]
    L.bp_ranges.argtypes = [I16P, C.c_int, C.c_int, C.c_int, LLP]
    L.bp_ranges.restype = None
    return L


def _many(L, frames, c0, c1, sp, variant):
    frames = np.ascontiguousarray(frames, np.int16)
    c0, c1, sp = (np.ascontiguousarray(a, np.int32) for a in (c0, c1, sp))
    counts = np.zeros(4, np.int64)
    first = L.bp_compare_many(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP),
                              sp.ctypes.data_as(INTP), len(frames), variant, counts.ctypes.data_as(LLP))
    assert first < 0, ("first bad frame", frames[first].tolist(), int(c0[first]), int(c1[first]), int(sp[first]))
    assert counts[1] == 0 and counts[3] == 0, counts.tolist()
    inside = np.abs(c0.astype(np.int64)) + np.abs(c1.astype(np.int64)) <= BOUND
    assert counts[0] == int(inside.sum()) and counts[2] == int((~inside).sum()), counts.tolist()   # no frame left out
    return counts


def _ranges(L, x, c0, c1, sp):
    out = np.zeros(7, np.int64)
    x = np.ascontiguousarray(x, np.int16)
    L.bp_ranges(x.ctypes.data_as(I16P), c0, c1, sp, out.ctypes.data_as(LLP))
    return out


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rail_frames_at_every_scale_on_and_past_the_bound(drv, variant):
    frames, c0s, c1s, sps = [], [], [], []
    for x in _rail_frames():
        for (c0, c1) in ORDINARY + ON_BOUND + PAST_BOUND + FAR:
            for sp in SCALES:
                frames.append(x); c0s.append(c0); c1s.append(c1); sps.append(sp)
    counts = _many(drv, np.stack(frames), c0s, c1s, sps, VARIANTS[variant])
    assert counts[0] == len(_rail_frames()) * len(ORDINARY + ON_BOUND) * 13
    assert counts[2] == len(_rail_frames()) * len(PAST_BOUND + FAR) * 13


def _tie_frames(sp, pred):
    """inputs that are odd multiples of 2^(sp - 1), both signs: with the zero predictor d = in * 2048 is congruent to
    2^(k - 1) mod 2^k (k = sp + 11) at every sample; with (2048, 0) d = (in - previous output) * 2048, and the previous
    output is a multiple of 2^sp, so the same holds"""
    unit = 1 << (sp - 1)
    top = min(32767 // unit, 15)
    odd = [m for m in range(-top, top + 1) if m % 2]
    rng = np.random.default_rng(1000 * sp + pred)
    frames = []
    for _ in range(24):
        body = rng.choice(odd, 14) * unit
        hist = rng.integers(-4, 5, 2) * (1 << sp)
        frames.append(np.concatenate([hist, body]))
    frames.append(np.concatenate([[0, 0], np.resize([unit, -unit], 14)]))
    frames.append(np.concatenate([[0, 0], np.resize([-unit, -unit, unit], 14)]))
    return np.stack(frames).clip(-32768, 32767).astype(np.int16)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_exact_ties_of_both_signs(drv, variant):
    ties_pos = ties_neg = 0
    for sp in range(1, 13):
        for pred, (c0, c1) in enumerate([(0, 0), (2048, 0)]):
            frames = _tie_frames(sp, pred)
            _many(drv, frames, [c0] * len(frames), [c1] * len(frames), [sp] * len(frames), VARIANTS[variant])
            for x in frames:
                r = _ranges(drv, x, c0, c1, sp)
                assert r[4] == 0
                ties_pos += int(r[5]); ties_neg += int(r[6])
    # the set is only worth its name if the compared frames DO hit exact ties, above and below zero
    assert ties_pos > 1000 and ties_neg > 1000, (ties_pos, ties_neg)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_seeded_random_frames(drv, variant):
    rng = np.random.default_rng(20241019)
    n = 100000
    sp = rng.integers(0, 13, n)
    kind = rng.integers(0, 4, n)
    amp = rng.choice([8, 300, 5000, 32768], n)
    t = np.arange(16)
    frames = np.empty((n, 16), np.int64)
    noise = rng.integers(-32768, 32768, (n, 16))
    frames[:] = noise * amp[:, None] // 32768
    ramp = t[None, :] * rng.integers(-300, 300, n)[:, None] + rng.integers(-2000, 2000, n)[:, None]
    rails = np.where(rng.integers(0, 2, (n, 16)) > 0, 32767, -32768)
    sine = amp[:, None] * np.sin(t[None, :] * rng.uniform(0.02, 3.1, n)[:, None] + rng.uniform(0, 6.3, n)[:, None])
    frames = np.where((kind == 1)[:, None], ramp, frames)
    frames = np.where((kind == 2)[:, None], rails, frames)
    frames = np.where((kind == 3)[:, None], sine.astype(np.int64), frames)
    frames = frames.clip(-32768, 32767).astype(np.int16)
    wide = rng.integers(0, 3, n) == 0
    c0 = np.where(wide, rng.integers(-32768, 32768, n), rng.integers(-4096, 4097, n))
    c1 = np.where(wide, rng.integers(-32768, 32768, n), rng.integers(-2048, 2049, n))
    counts = _many(drv, frames, c0, c1, sp, VARIANTS[variant])
    assert counts[0] > 70000 and counts[2] > 5000, counts.tolist()


def test_extreme_t_of_b3_and_the_operand_ranges(drv):
    """B1-B3 at their corners: histories and inputs on the rails with coefficients on the bound.  The operands of the subtract
    stay in [0, 2^31), the borrow is the sign, and t reaches -2^31 + 1024 (d = -2^30, scale 0, with its borrow) but not below
    -2^31.  One past the bound the same corner would leave int32: that is why the bound is 30720."""
    lo_t = 1 << 62
    for (c0, c1) in ON_BOUND + [(-30720, 0), (0, 30720), (15360, 15360)]:
        for h in ((-32768, -32768), (32767, 32767), (-32768, 32767), (32767, -32768)):
            for fill in (-32768, 32767):
                x = np.array(list(h) + [fill] * 14, np.int16)
                for sp in SCALES:
                    for variant in (0, 1):
                        assert drv.bp_compare(x.ctypes.data_as(I16P), c0, c1, sp, variant) == 0
                    r = _ranges(drv, x, c0, c1, sp)
                    assert r[0] >= -(1 << 31) and r[1] < (1 << 31), (c0, c1, h, fill, sp, r.tolist())
                    assert r[2] >= 0 and r[3] < (1 << 31) and r[4] == 0, (c0, c1, h, fill, sp, r.tolist())
                    lo_t = min(lo_t, int(r[0]))
    assert lo_t == -(1 << 31) + 1024, lo_t
    x = np.array([-32768, -32768] + [-32768] * 14, np.int16)
    assert _ranges(drv, x, -15360, -15361, 0)[0] < -(1 << 31)
    assert drv.bp_compare(x.ctypes.data_as(I16P), -15360, -15361, 0, 0) == 2
