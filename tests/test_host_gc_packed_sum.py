"""CPU-side check of the GC-ADPCM encoder's error sum in packed pairs (gc_encode_core.hpp E1-E5, round 8): the header is
compiled for the host with a small driver (tests/host/gc_packed_sum_driver.cpp).  First the pass alone, lane by lane against
the scalar 64-bit error sum of the same nibbles: equal below 2^28, at least 2^28 otherwise.  Then whole channels through a
lane emulator of the kernel's frame -- exact-sum rule included -- against the oracle, byte for byte.  Host logic under test,
not a product path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gc_packed_sum_cases as cases_mod

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_packed_sum_driver.cpp")
HDR = os.path.join(HERE, "..", "vgaudio_amd", "csrc", "gc_encode_core.hpp")
SO = os.path.join(HERE, "host", "libgc_packed_sum_driver.so")

I16P = C.POINTER(C.c_int16)
INTP = C.POINTER(C.c_int)
VARIANTS = {"rounded": 0, "no_round": 1}


@pytest.fixture(scope="module")
def drv():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off",
                        "-fno-fast-math", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    L.ps_check_many.argtypes = [I16P, INTP, INTP, INTP, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    L.ps_encode8.argtypes = [I16P, C.c_int, I16P, C.c_int16, C.c_int16, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
    return L


def _check(L, frames, c0, c1, sp, variant):
    frames = np.ascontiguousarray(frames, np.int16)
    c0, c1, sp = (np.ascontiguousarray(a, np.int32) for a in (c0, c1, sp))
    counts = np.zeros(6, np.int64)
    first = L.ps_check_many(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP),
                            sp.ctypes.data_as(INTP), len(frames), variant, counts.ctypes.data_as(C.POINTER(C.c_longlong)))
    assert first < 0, ("first violating frame", frames[first].tolist(), int(c0[first]), int(c1[first]), int(sp[first]))
    assert counts[2] == 0
    return counts


def _rail_frames():
    """inputs on one rail against outputs driven to the other: histories and bodies of +-32767 / -32768, alternating and in
    blocks, so that x - o reaches +-65535"""
    t = np.arange(14)
    bodies = [np.where(t % 2 == 0, 32767, -32768), np.where(t % 2 == 0, -32768, 32767),
              np.where((t // 2) % 2 == 0, 32767, -32768), np.where((t // 3) % 2 == 0, -32768, 32767),
              np.where((t // 7) % 2 == 0, 32767, -32768), np.full(14, 32767), np.full(14, -32768), np.full(14, -32767)]
    hists = [(-32768, -32768), (32767, 32767), (-32768, 32767), (32767, -32768), (0, 0)]
    return [np.concatenate([np.array(h), b]).astype(np.int16) for b in bodies for h in hists]


# (c0, c1): |c0| + |c1| = 32767 exactly, beyond it (the predictor can wrap: the pass does not vouch, the property still holds
# for the sum), and ordinary predictors
ON_BOUND = [(32767, 0), (0, 32767), (-32767, 0), (0, -32767), (16384, 16383), (-16384, 16383), (-16383, -16384), (4096, -28671)]
BEYOND = [(-32768, -32768), (-32768, 0), (0, -32768), (32767, 32767), (32767, -32768), (-32768, 32767), (20000, 20000),
          (16384, 16384), (30000, -2768)]
ORDINARY = [(0, 0), (-2048, 0), (2048, 0), (4095, -2047), (3900, -1900), (-3900, -1900), (0, -2048), (1200, 700)]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rails_at_every_scale_and_coefficients_on_and_beyond_the_bound(drv, variant):
    frames, c0s, c1s, sps = [], [], [], []
    for x in _rail_frames():
        for (c0, c1) in ON_BOUND + BEYOND + ORDINARY:
            for sp in range(13):
                frames.append(x); c0s.append(c0); c1s.append(c1); sps.append(sp)
    counts = _check(drv, np.stack(frames), c0s, c1s, sps, VARIANTS[variant])
    # the set is only worth its name if it holds sums on both sides of 2^28, saturated halves, sums past 2^31 and passes that vouch
    assert counts[0] > 0 and counts[1] > 1000 and counts[3] > 1000 and counts[4] > 1000 and counts[5] > 0, counts.tolist()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_seeded_random_frames_across_every_scale(drv, variant):
    rng = np.random.default_rng(20240808)
    n = 13 * 600
    sp = np.repeat(np.arange(13), 600)
    kind = rng.integers(0, 4, n)
    amp = rng.choice([8, 300, 5000, 32768], n)
    frames = np.empty((n, 16), np.int64)
    for i in range(n):
        if kind[i] == 0:
            frames[i] = rng.integers(-amp[i], amp[i], 16)
        elif kind[i] == 1:
            frames[i] = np.arange(16) * int(rng.integers(-300, 300)) + int(rng.integers(-2000, 2000))
        elif kind[i] == 2:
            frames[i] = np.where(rng.integers(0, 2, 16) > 0, 32767, -32768)
        else:
            frames[i] = amp[i] * np.sin(np.arange(16) * rng.uniform(0.02, 3.1) + rng.uniform(0, 6.3))
    frames = frames.clip(-32768, 32767).astype(np.int16)
    big = rng.integers(0, 4, n) == 0
    c0 = np.where(big, rng.integers(-32768, 32768, n), rng.integers(-4096, 4097, n))
    c1 = np.where(big, rng.integers(-32768, 32768, n), rng.integers(-2048, 2049, n))
    counts = _check(drv, frames, c0, c1, sp, VARIANTS[variant])
    assert counts[0] > 2000 and counts[1] > 500 and counts[5] > 600, counts.tolist()


def _emulate(L, pcm, coefs, h1, h2, nbytes):
    out = np.zeros((len(pcm) + 13) // 14 * 8, np.uint8)
    stats = np.zeros(8, np.uint64)
    pcm = np.ascontiguousarray(pcm)
    coefs = np.ascontiguousarray(coefs)
    L.ps_encode8(pcm.ctypes.data_as(I16P), len(pcm), coefs.ctypes.data_as(I16P), int(h1), int(h2),
                 out.ctypes.data_as(C.POINTER(C.c_uint8)), stats.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out[:nbytes], [int(v) for v in stats]


def test_whole_channels_through_the_lane_emulator_match_the_oracle(drv):
    """the first 18 seeded channels (every kind twice).  Required of the set: final lanes whose error does not fit int16, frames
    whose best sum is 2^28 or more, lanes sent through the wide pass, and frames where the packed sums taken as they are would
    have picked another predictor -- so that the exact-sum rule is what makes these bytes right."""
    pcm, coefs, h1, h2, want, _ = cases_mod.cases()
    total = np.zeros(8, np.int64)
    per_kind = {}
    for c in range(18):
        got, stats = _emulate(drv, pcm[c], coefs[c], h1[c], h2[c], want.shape[1])
        bad = np.argwhere(got != want[c])
        assert bad.size == 0, (c, "first differing byte", bad[0].tolist(), stats)
        total += np.array(stats, np.int64)
        per_kind.setdefault(c % len(cases_mod.KINDS), np.zeros(8, np.int64))
        per_kind[c % len(cases_mod.KINDS)] += np.array(stats, np.int64)
    assert total[1] > 0 and total[2] > 0 and total[3] > 0 and total[4] > 0 and total[5] > 0, total.tolist()
    # what the search found for coefficients that pass coef_ok (tests/gc_packed_sum_cases.py):
    assert per_kind[0][1] > 0 and per_kind[0][5] > 0, per_kind[0].tolist()      # white noise, coefficients on the bound: 64-bit keys
    assert per_kind[1][3] > 0 and per_kind[1][1] == 0, per_kind[1].tolist()     # clipped square, the oracle's own: |e| >= 32768 only
    assert per_kind[2][1] > 0 and per_kind[2][3] > 0, per_kind[2].tolist()      # clipped square, large coefficients: both
