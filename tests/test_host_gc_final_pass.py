"""CPU-side check of the GC-ADPCM encoder's frame resolution in the (channel, predictor) layout (gc_encode_core.hpp,
final_pass_pair and frame_flags): the pass at s1 for its overflow only, ONE final pass at the scale that overflow names, the
flags from the two overflows -- against the form it replaces (passes B and A with both result sets kept, 21 selects, the
flags as the frame code wrote them), restated in tests/host/gc_final_pass_driver.cpp from the header's functions.
Compared per lane: nibbles mod 16, history pair, error sum, final scale, and whether the lane asks for the cold block (with
what the cold block derives: generic, inexact, resume, bump_a).  The no-round pair, where it vouches for itself, is held
against the ROUNDED old form.  Host logic under test, not a product path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_host_gc_borrow_pass import FAR, ON_BOUND, PAST_BOUND, SCALES, _tie_frames
from test_host_gc_packed_pass import ORDINARY, _rail_frames

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_final_pass_driver.cpp")
HDR = os.path.join(HERE, "..", "vgaudio_amd", "csrc", "gc_encode_core.hpp")
SO = os.path.join(HERE, "host", "libgc_final_pass_driver.so")

VARIANTS = {"rounded": 0, "no_round": 1}
I16P = C.POINTER(C.c_int16)
INTP = C.POINTER(C.c_int)
LLP = C.POINTER(C.c_longlong)
FIN_A, COLD, OV_A, OV_B, FINAL_SP, GENERIC, INEXACT, RESUME, BUMP_A = range(9)


@pytest.fixture(scope="module")
def drv():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off",
                        "-fno-fast-math", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    L.fp_compare_many.argtypes = [I16P, INTP, INTP, INTP, C.c_int, C.c_int, LLP, INTP]
    L.fp_first_scale.argtypes = [I16P, C.c_int, C.c_int]
    L.fp_enumerate_flags.argtypes = [INTP, C.c_int, LLP]
    return L


def _many(L, frames, c0, c1, s1, variant):
    """every frame compared; returns (counts by return code, info rows of the old form)"""
    frames = np.ascontiguousarray(frames, np.int16)
    n = len(frames)
    c0, c1, s1 = (np.ascontiguousarray(np.broadcast_to(a, (n,)), np.int32) for a in (c0, c1, s1))
    counts = np.zeros(3, np.int64)
    info = np.zeros((n, 9), np.int32)
    first = L.fp_compare_many(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP),
                              s1.ctypes.data_as(INTP), n, variant, counts.ctypes.data_as(LLP), info.ctypes.data_as(INTP))
    assert first < 0, ("first bad frame", frames[first].tolist(), int(c0[first]), int(c1[first]), int(s1[first]), info[first].tolist())
    assert counts[1] == 0 and counts.sum() == n, counts.tolist()
    if variant == 0:
        assert counts[2] == 0, counts.tolist()          # the rounded pair is always compared
    return counts, info


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rail_frames_at_thirteen_scales_on_and_past_the_coefficient_bound(drv, variant):
    frames, c0s, c1s, s1s = [], [], [], []
    for x in _rail_frames():
        for (c0, c1) in ORDINARY + ON_BOUND + PAST_BOUND + FAR:
            for s1 in SCALES:
                frames.append(x); c0s.append(c0); c1s.append(c1); s1s.append(s1)
    counts, info = _many(drv, np.stack(frames), c0s, c1s, s1s, VARIANTS[variant])
    assert counts[0] > len(frames) // (2 if variant == "rounded" else 8), counts.tolist()
    assert info[:, COLD].any() and not info[:, COLD].all()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_exact_ties_of_both_signs(drv, variant):
    compared = 0
    for sp in range(1, 13):
        for pred, (c0, c1) in enumerate([(0, 0), (2048, 0)]):
            frames = _tie_frames(sp, pred)
            for s1 in {max(sp - 1, 0), sp}:              # the tie scale as pass B's and as pass A's
                counts, _ = _many(drv, frames, c0, c1, s1, VARIANTS[variant])
                compared += int(counts[0])
    assert compared > (1000 if variant == "rounded" else 500), compared


def _random_frames(n):
    """the frame set of tests/test_host_gc_borrow_pass.py::test_seeded_random_frames (same seed, same draws)"""
    rng = np.random.default_rng(20241019)
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
    return frames, c0, c1, sp


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_seeded_random_frames_at_a_drawn_scale_and_at_their_own(drv, variant):
    frames, c0, c1, sp = _random_frames(100000)
    counts, info = _many(drv, frames, c0, c1, sp, VARIANTS[variant])
    assert counts[0] > (99999 if variant == "rounded" else 20000), counts.tolist()
    for col in (FIN_A, COLD, GENERIC, INEXACT, RESUME, BUMP_A):          # every kind of lane is in the set
        assert info[:, col].any() and not info[:, col].all(), col
    # ... and at the scale the kernel's pre-scan gives the frame (the first 20000: the pre-scan is a call per frame)
    m = 20000
    own = np.array([drv.fp_first_scale(frames[i].ctypes.data_as(I16P), int(c0[i]), int(c1[i])) for i in range(m)], np.int32)
    counts, info = _many(drv, frames[:m], c0[:m], c1[:m], own, VARIANTS[variant])
    assert counts[0] > (m - 1 if variant == "rounded" else m // 4), counts.tolist()
    assert info[:, FIN_A].any() and info[:, RESUME].any()


def _scan(drv, s1, variant):
    """alternating full-scale frames, the history on the rail against them, c0 from 0 upwards in steps of 8: the distance of
    every sample grows by 32768 * 8 a step, the overflow of a pass at scale 11 or 12 by far less than one"""
    x = np.array([32767, -32768] + [32767, -32768] * 7, np.int16)
    c0 = np.arange(0, 6000, 8)
    frames = np.broadcast_to(x, (len(c0), 16))
    return _many(drv, frames, c0, 0, s1, variant)[1]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_built_frames_meet_every_case_of_the_resolution(drv, variant):
    v = VARIANTS[variant]
    # A is final: a quiet frame at its own scale
    quiet = np.array([0, 0] + [3, -2, 5, 1, -4, 2, 0, 6, -7, 3, 1, -1, 2, 0], np.int16)[None, :]
    info = _many(drv, quiet, 0, 0, 0, v)[1]
    assert info[0, FIN_A] == 1 and info[0, COLD] == 0 and info[0, FINAL_SP] == 0
    # A at the cap with overflow 3 (final, hot) and 4 (final, inexact: cold)
    info = _scan(drv, 12, v)
    for ov, cold in ((3, 0), (4, 1)):
        rows = info[info[:, OV_A] == ov]
        assert len(rows) and (rows[:, FIN_A] == 1).all() and (rows[:, COLD] == cold).all() and (rows[:, INEXACT] == cold).all(), ov
        assert (rows[:, FINAL_SP] == 12).all()
    # B at the cap with overflow 3 and 4, A (scale 11) overflowing without a bump
    info = _scan(drv, 11, v)
    for ov, cold in ((3, 0), (4, 1)):
        rows = info[(info[:, OV_B] == ov) & (info[:, FIN_A] == 0) & (info[:, BUMP_A] == 0)]
        assert len(rows) and (rows[:, COLD] == cold).all() and (rows[:, INEXACT] == cold).all() and (rows[:, FINAL_SP] == 12).all(), ov
    # ov_a of 248 (on to pass B, which overflows as well: resume) and 249 (the bump loop: generic), zero predictor at scale 0
    for top, ov, bump in ((255, 248, 0), (256, 249, 1), (-256, 248, 0), (-257, 249, 1)):
        x = np.array([0, 0] + [top, 0] * 7, np.int16)[None, :]
        info = _many(drv, x, 0, 0, 0, v)[1]
        assert info[0, OV_A] == ov and info[0, FIN_A] == 0 and info[0, COLD] == 1, (top, info[0].tolist())
        assert info[0, BUMP_A] == bump and info[0, GENERIC] == bump and info[0, RESUME] == 1 - bump, (top, info[0].tolist())
    # both passes overflowing by a little: a frame at a scale two below its own
    x = np.array([0, 0] + [100, -90, 80, -100, 60, 90, -70, 100, -100, 50, 40, -30, 20, 100], np.int16)[None, :]
    own = drv.fp_first_scale(x[0].ctypes.data_as(I16P), 0, 0)
    info = _many(drv, x, 0, 0, own - 2, v)[1]
    assert info[0, RESUME] == 1 and info[0, COLD] == 1 and 1 < info[0, OV_B] < info[0, OV_A] <= 248, info[0].tolist()


def test_the_flags_from_the_final_pass_and_as_one_bit_equal_the_expressions_they_replace(drv):
    ovs = np.array([0, 1, 2, 3, 4, 248, 249, 250], np.int32)
    visited = C.c_longlong(0)
    bad = drv.fp_enumerate_flags(ovs.ctypes.data_as(INTP), len(ovs), C.byref(visited))
    assert visited.value == 13 * 8 * 8 * 2
    assert bad == 0
