"""CPU-side check of the GC-ADPCM encoder's fast quantise pass on a packed history pair (gc_encode_core.hpp, P1-P6): the
header is compiled for the host with a small driver and every instantiation of pass_fast_core_t is compared with the literal
pass -- nibbles, packed history, error sum, overflow -- wherever it vouches for itself.  Host logic under test, not a product
path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "gc_packed_pass_driver.cpp")
HDR = os.path.join(HERE, "..", "vgaudio_amd", "csrc", "gc_encode_core.hpp")
SO = os.path.join(HERE, "host", "libgc_packed_pass_driver.so")

VARIANTS = {"rounded": 0, "no_round": 1, "wide": 2}
I16P = C.POINTER(C.c_int16)
INTP = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def drv():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off",
                        "-fno-fast-math", SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    L.pp_compare.argtypes = [I16P, C.c_int, C.c_int, C.c_int, C.c_int]
    L.pp_compare_many.argtypes = [I16P, INTP, INTP, INTP, C.c_int, C.c_int, C.POINTER(C.c_longlong)]
    L.pp_rail_runs.argtypes = [I16P, C.c_int, C.c_int, C.c_int, INTP]
    L.pp_rail_runs.restype = None
    return L


def _many(L, frames, c0, c1, sp, variant):
    frames = np.ascontiguousarray(frames, np.int16)
    c0, c1, sp = (np.ascontiguousarray(a, np.int32) for a in (c0, c1, sp))
    counts = np.zeros(4, np.int64)
    first = L.pp_compare_many(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP),
                              sp.ctypes.data_as(INTP), len(frames), variant, counts.ctypes.data_as(C.POINTER(C.c_longlong)))
    assert first < 0, ("first differing frame", frames[first].tolist(), int(c0[first]), int(c1[first]), int(sp[first]))
    return counts


def _rail_frames():
    """full-scale frames whose reconstruction leaves the 16-bit range: alternating and blocked +-32768 / 32767, from
    histories on either rail"""
    t = np.arange(14)
    bodies = [np.where(t % 2 == 0, 32767, -32768), np.where(t % 2 == 0, -32768, 32767),
              np.where((t // 2) % 2 == 0, 32767, -32768), np.where((t // 3) % 2 == 0, -32768, 32767),
              np.full(14, 32767), np.full(14, -32768)]
    hists = [(-32768, -32768), (32767, 32767), (-32768, 32767), (32767, -32768), (0, 0)]
    return [np.concatenate([np.array(h), b]).astype(np.int16) for b in bodies for h in hists]


# coefficient pairs (c0, c1): the 16-bit extremes, pairs whose predictor can wrap int32 (|c0| + |c1| > 32767), pairs exactly on
# the bound, and ordinary predictors that overshoot a full-scale square (the reconstruction runs past the rails)
HOSTILE = [(-32768, -32768), (-32768, 0), (0, -32768), (32767, 32767), (32767, -32768), (-32768, 32767), (20000, 20000),
           (-16384, -16384), (30000, -2768)]
ON_BOUND = [(32767, 0), (0, 32767), (-32767, 0), (0, -32767), (16384, 16383), (-16384, 16383), (-16383, -16384), (4096, -28671)]
ORDINARY = [(0, 0), (-2048, 0), (2048, 0), (4095, -2047), (3900, -1900), (-3900, -1900), (0, -2048), (0, 2047), (1200, 700)]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_directed_frames_on_the_rails_and_hostile_coefficients(drv, variant):
    frames, c0s, c1s, sps = [], [], [], []
    for x in _rail_frames():
        for (c0, c1) in HOSTILE + ON_BOUND + ORDINARY:
            for sp in (0, 1, 6, 11, 12):
                frames.append(x); c0s.append(c0); c1s.append(c1); sps.append(sp)
    counts = _many(drv, np.stack(frames), c0s, c1s, sps, VARIANTS[variant])
    assert counts[0] > 0 and counts[2] > 0, counts.tolist()
    # coefficients that can wrap are never vouched for; at the bound and below the wide pass always is
    for (c0, c1) in HOSTILE:
        for x in _rail_frames()[:5]:
            assert drv.pp_compare(x.ctypes.data_as(I16P), c0, c1, 12, VARIANTS[variant]) == 2
    if variant == "wide":
        n_ok = len(_rail_frames()) * len(ON_BOUND + ORDINARY) * 5
        assert counts[0] == n_ok, (counts.tolist(), n_ok)


def test_compared_frames_saturate_an_out_of_range_value_twice_at_both_rails(drv):
    """the directed set is only worth its name if frames that ARE compared (exact) keep the unclamped reconstruction outside
    the 16-bit range for two samples running and more, above and below, at scale 0 and at the cap 12"""
    out = np.zeros(2, np.int32)
    seen = {(sp, rail): 0 for sp in (0, 12) for rail in (0, 1)}
    for x in _rail_frames():
        for (c0, c1) in ON_BOUND + ORDINARY:
            for sp in (0, 12):
                for variant in (0, 2):
                    if drv.pp_compare(x.ctypes.data_as(I16P), c0, c1, sp, variant) != 0:
                        continue
                    drv.pp_rail_runs(x.ctypes.data_as(I16P), c0, c1, sp, out.ctypes.data_as(INTP))
                    for rail in (0, 1):
                        if out[rail] >= 2:
                            seen[(sp, rail)] += 1
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_seeded_random_frames_across_every_scale(drv, variant):
    rng = np.random.default_rng(20240707)
    n = 13 * 400                                            # 400 frames per scale power
    sp = np.repeat(np.arange(13), 400)
    kind = rng.integers(0, 4, n)
    amp = rng.choice([8, 300, 5000, 32768], n)
    frames = np.empty((n, 16), np.int64)
    for i in range(n):
        if kind[i] == 0:
            frames[i] = rng.integers(-amp[i], amp[i], 16)
        elif kind[i] == 1:                                  # predictable: small scales come out exact too
            frames[i] = np.arange(16) * int(rng.integers(-300, 300)) + int(rng.integers(-2000, 2000))
        elif kind[i] == 2:
            frames[i] = np.where(rng.integers(0, 2, 16) > 0, 32767, -32768)
        else:
            frames[i] = amp[i] * np.sin(np.arange(16) * rng.uniform(0.02, 3.1) + rng.uniform(0, 6.3))
    frames = frames.clip(-32768, 32767).astype(np.int16)
    hostile = rng.integers(0, 5, n) == 0
    c0 = np.where(hostile, rng.integers(-32768, 32768, n), rng.integers(-4096, 4097, n))
    c1 = np.where(hostile, rng.integers(-32768, 32768, n), rng.integers(-2048, 2049, n))
    counts = _many(drv, frames, c0, c1, sp, VARIANTS[variant])
    assert counts[0] > (2500 if variant == "wide" else 600), counts.tolist()
    assert counts[2] > 0, counts.tolist()
