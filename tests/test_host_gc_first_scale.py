"""CPU-side check of the GC-ADPCM encoder's first-scale work (gc_encode_core.hpp F1-F5, N1-N2, round 9): the header is compiled
for the host with a small driver (tests/host/gc_first_scale_driver.cpp).
(i) the first scale from the frame's range against the form it replaces, EXHAUSTIVELY over dmax in [0, 32767] x dmin in
[-32768, 0] (2^30 pairs, split over the available threads; a few seconds);  (ii) the encoder wave's two head distances in the
numerator domain (no quotient) against prescan_range.  Code under test in (ii) and (iii): head_distance_numer,
predicted_p1024, first_scale_power_nt and first_scale_tie.  The range of s = 2..13 that stands beside them is the driver's own
copy of the helper wave's loop -- the helper is unchanged; its numerator-domain form was measured, did not pay and is not in
the tree (LABNOTES 14);  (iii) wrapping coefficients through the head that keeps the quotient, against the sequential pre-scan;
(iv) both lane emulators against the oracle on the seeded channels of tests/gc_packed_sum_cases.py;  (v) the fast pass with
step 0's dot product handed in (HAVE_P0) against the pass that forms it itself.  Host logic under test, not a product path."""
import concurrent.futures
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import gc_packed_sum_cases as cases_mod

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(HERE, "..", "vgaudio_amd", "csrc", "gc_encode_core.hpp")
I16P = C.POINTER(C.c_int16)
INTP = C.POINTER(C.c_int)
LLP = C.POINTER(C.c_longlong)


def _build(src, so):
    src, so = os.path.join(HERE, "host", src), os.path.join(HERE, "host", so)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fwrapv", "-ffp-contract=off",
                        "-fno-fast-math", src, "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def drv():
    L = _build("gc_first_scale_driver.cpp", "libgc_first_scale_driver.so")
    L.fs_check_first_scale.argtypes = [C.c_int, C.c_int, LLP, INTP]
    L.fs_check_first_scale_pairs.argtypes = [INTP, INTP, C.c_int]
    L.fs_check_numer.argtypes = [I16P, INTP, INTP, C.c_int, LLP]
    L.fs_check_prescan.argtypes = [I16P, INTP, INTP, C.c_int, C.c_int, LLP]
    L.fs_check_pass_p0.argtypes = [I16P, INTP, INTP, INTP, C.c_int]
    return L


def test_first_scale_equals_the_form_it_replaces_on_every_pair(drv):
    """all 2^30 pairs of the callers' domain, -100 included (one pass: about 15 s of CPU time, split over the threads)"""
    workers = max(1, min(16, len(os.sched_getaffinity(0))))
    edges = np.linspace(0, 32768, 4 * workers + 1).astype(int)

    def part(k):
        counts = np.zeros(2, np.int64)
        bad = np.zeros(2, np.int32)
        rc = drv.fs_check_first_scale(int(edges[k]), int(edges[k + 1]), counts.ctypes.data_as(LLP), bad.ctypes.data_as(INTP))
        return rc, counts, bad

    with concurrent.futures.ThreadPoolExecutor(workers) as pool:
        results = list(pool.map(part, range(len(edges) - 1)))
    for rc, _, bad in results:
        assert rc == 0, ("first differing (dmax, dmin)", bad.tolist())
    total = sum(c for _, c, _ in results)
    assert total[0] == 32768 * 32769
    # +M and -M with the four leading bits 1000: 8, 16-17, 32-35, ... 16384-18431 (32768 has no +M)
    assert total[1] == sum(1 << j for j in range(12))


def test_first_scale_beyond_sixteen_bits(drv):
    """the kernel's head distances are not clamped: values up to +-65535 and wrong-signed ones clamp as they always did"""
    rng = np.random.default_rng(9)
    dmax = np.concatenate([rng.integers(-70000, 70001, 200000), [32767, 32768, 65535, 40000, -5, 0]]).astype(np.int32)
    dmin = np.concatenate([rng.integers(-70000, 70001, 200000), [-32768, -32769, -65535, -40000, 5, 0]]).astype(np.int32)
    assert drv.fs_check_first_scale_pairs(dmax.ctypes.data_as(INTP), dmin.ctypes.data_as(INTP), len(dmax)) == -1


# (c0, c1) on |c0| + |c1| = 32767 in all four sign quadrants, and ordinary predictors
ON_BOUND = [(32767, 0), (0, 32767), (-32767, 0), (0, -32767), (16384, 16383), (-16384, 16383), (16384, -16383), (-16383, -16384),
            (4096, -28671), (-4096, 28671), (1, 32766), (-1, -32766), (28671, 4096), (-28671, -4096)]
ORDINARY = [(0, 0), (-2048, 0), (2048, 0), (4095, -2047), (3900, -1900), (-3900, -1900), (0, -2048), (1200, 700), (1, 0), (0, -1),
            (2047, 1), (-2047, -1)]
WRAPPING = [(-32768, -32768), (-32768, 0), (0, -32768), (32767, 32767), (32767, -32768), (-32768, 32767), (20000, 20000),
            (16384, 16384), (30000, -2768), (-32768, 1), (1, -32768)]


def _rail_frames():
    t = np.arange(16)
    out = [np.where(t % 2 == 0, 32767, -32768), np.where(t % 2 == 0, -32768, 32767), np.where((t // 2) % 2 == 0, 32767, -32768),
           np.where((t // 3) % 2 == 0, -32768, 32767), np.where((t // 7) % 2 == 0, 32767, -32768), np.full(16, 32767),
           np.full(16, -32768), np.full(16, -32767), np.where(t < 2, -32768, 32767), np.where(t < 2, 32767, -32768),
           np.where(t % 3 == 0, -32768, 0), np.zeros(16, int)]
    return [f.astype(np.int64) for f in out]


def _exact_d_frames():
    """frames and coefficients whose predictor sum D = a * c1 + b * c0 is exactly 0, +-1, +-2047, +-2048 at every sample, and
    frames whose numerator in * 2048 - D is a multiple of 2048 (D a multiple of 2048)"""
    frames, cs = [], []
    for target in (0, 1, -1, 2047, -2047, 2048, -2048, 4096, -6144):
        # a = 1 and c1 = target, b = 0: D = target wherever the pair is (1, 0); and b = 1, c0 = target with a = 0
        for c0, c1, a, b in ((0, target, 1, 0), (target, 0, 0, 1), (target, 0, 0, -1), (0, target, -1, 0)):
            for fill in (0, 5, -5, 32767, -32768):
                x = np.empty(16, np.int64)
                x[0::2], x[1::2] = a, b
                y = x.copy()
                y[2::4] = fill                      # some inputs elsewhere: the distance is in - D / 2048 with in = fill
                frames += [x, y, np.roll(x, 1), np.roll(y, 1)]
                cs += [(c0, c1)] * 4
    for m in (-3, -1, 0, 1, 2, 15):                # D = 2048 * m * b exactly (c0 = 2048 * m): numerators on multiples of 2048
        for x in ([3, 1, -1, 2, -2, 7, -7, 15, -16, 100, -100, 1000, -1000, 0, 0, 1], [0, 16, -16, 16, -16, 0, 1, -1, 1, -1, 2, -2, 2, -2, 3, -3]):
            if abs(2048 * m) <= 32767:
                frames.append(np.array(x, np.int64))
                cs.append((2048 * m, 0))
    return frames, cs


def _numer(drv, frames, c0, c1):
    frames = np.ascontiguousarray(np.asarray(frames).clip(-32768, 32767), np.int16)
    c0, c1 = (np.ascontiguousarray(a, np.int32) for a in (c0, c1))
    counts = np.zeros(3, np.int64)
    first = drv.fs_check_numer(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP), len(frames),
                               counts.ctypes.data_as(LLP))
    assert first == -1, ("first differing frame", first, frames[first].tolist(), int(c0[first]), int(c1[first]))
    for numer in (1, 0):                           # and the whole pre-scan, both branches, against the sequential one
        first = drv.fs_check_prescan(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP), len(frames),
                                     numer, np.zeros(2, np.int64).ctypes.data_as(LLP))
        assert first == -1, (numer, "first differing frame", first, frames[first].tolist(), int(c0[first]), int(c1[first]))
    return counts


def test_head_distances_and_range_on_rails_and_on_the_coefficient_bound(drv):
    frames, c0s, c1s = [], [], []
    for x in _rail_frames():
        for (c0, c1) in ON_BOUND + ORDINARY:
            frames.append(x); c0s.append(c0); c1s.append(c1)
    counts = _numer(drv, frames, c0s, c1s)
    assert counts[2] > 50, counts.tolist()          # distances beyond 16 bits: the clamp of pre[p] is exercised


def test_head_distances_and_range_where_the_sum_is_zero_one_or_a_multiple_of_2048(drv):
    frames, cs = _exact_d_frames()
    counts = _numer(drv, frames, [c[0] for c in cs], [c[1] for c in cs])
    assert counts[0] > 100 and counts[1] > 100, counts.tolist()


def test_head_distances_and_range_on_the_seeded_channels(drv):
    """every frame of the first 18 seeded channels with the coefficients the case gives it, predictors that can wrap left out"""
    pcm, coefs, h1, h2, _, _ = cases_mod.cases()
    frames, c0s, c1s = [], [], []
    for c in range(18):
        x = np.concatenate([[h2[c], h1[c]], pcm[c]]).astype(np.int64)
        nf = (len(x) - 2) // 14
        rows = np.stack([x[14 * f:14 * f + 16] for f in range(0, nf, 7)])
        for p in range(8):
            c0, c1 = int(coefs[c, 2 * p]), int(coefs[c, 2 * p + 1])
            if abs(c0) + abs(c1) <= 32767:
                frames.append(rows); c0s += [c0] * len(rows); c1s += [c1] * len(rows)
    _numer(drv, np.concatenate(frames), c0s, c1s)


def test_head_distances_and_range_on_a_million_random_frames(drv):
    rng = np.random.default_rng(20240909)
    n = 1_000_000
    amp = rng.choice([8, 300, 5000, 32768], n)[:, None]
    frames = (rng.integers(-32768, 32768, (n, 16)) * amp) >> 15
    rails = rng.integers(0, 8, (n, 16)) == 0
    frames = np.where(rails & (amp == 32768), np.where(frames < 0, -32768, 32767), frames)
    kind = rng.integers(0, 3, n)
    c0 = np.where(kind == 0, rng.integers(-32767, 32768, n), rng.integers(-4096, 4097, n))
    c1 = np.where(kind == 0, rng.integers(-32767, 32768, n), rng.integers(-2048, 2049, n))
    over = np.abs(c0) + np.abs(c1) > 32767          # onto the bound, signs kept
    c1 = np.where(over, np.sign(c1) * (32767 - np.abs(c0)), c1)
    assert (np.abs(c0) + np.abs(c1) <= 32767).all() and (np.abs(c0) + np.abs(c1) == 32767).sum() > 100000
    _numer(drv, frames, c0, c1)


def test_wrapping_coefficients_through_the_head_that_keeps_the_quotient(drv):
    frames, c0s, c1s = [], [], []
    rng = np.random.default_rng(5)
    rnd = [rng.integers(-32768, 32768, 16) for _ in range(40)] + [np.where(rng.integers(0, 2, 16) > 0, 32767, -32768) for _ in range(40)]
    for x in _rail_frames() + rnd:
        for (c0, c1) in WRAPPING + ON_BOUND[:4]:
            frames.append(x); c0s.append(c0); c1s.append(c1)
    frames = np.ascontiguousarray(np.asarray(frames), np.int16)
    c0, c1 = np.ascontiguousarray(c0s, np.int32), np.ascontiguousarray(c1s, np.int32)
    counts = np.zeros(2, np.int64)
    first = drv.fs_check_prescan(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP), len(frames), 0,
                                 counts.ctypes.data_as(LLP))
    assert first == -1, ("first differing frame", frames[first].tolist(), int(c0[first]), int(c1[first]))
    assert counts[0] > 0, "no frame whose predictor sum wraps int32: (-32768, -32768) . (-32768, -32768) is in the set"
    # the numerator domain refuses such coefficients
    assert drv.fs_check_prescan(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP), len(frames), 1,
                                counts.ctypes.data_as(LLP)) == -2


def test_both_lane_emulators_match_the_oracle_on_the_seeded_channels():
    """the emulators of the two lane layouts (tests/host/gc_encode_emulator.cpp) and the packed-sum emulator run the header's
    first scale: the first 18 seeded channels (every signal class of the packed-sum test twice), byte for byte"""
    emu = _build("gc_encode_emulator.cpp", "libgc_first_scale_emulator.so")
    ps = _build("gc_packed_sum_driver.cpp", "libgc_first_scale_packed_sum.so")
    U8P, U64P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)
    fns = [emu.emu_encode, emu.emu_encode8, ps.ps_encode8]
    for fn in fns:
        fn.argtypes = [I16P, C.c_int, I16P, C.c_int16, C.c_int16, U8P, U64P]
    pcm, coefs, h1, h2, want, _ = cases_mod.cases()
    for c in range(18):
        x, k = np.ascontiguousarray(pcm[c]), np.ascontiguousarray(coefs[c])
        for fn in fns:
            out = np.zeros((len(x) + 13) // 14 * 8, np.uint8)
            stats = np.zeros(8, np.uint64)
            fn(x.ctypes.data_as(I16P), len(x), k.ctypes.data_as(I16P), int(h1[c]), int(h2[c]), out.ctypes.data_as(U8P),
               stats.ctypes.data_as(U64P))
            bad = np.argwhere(out[:want.shape[1]] != want[c])
            assert bad.size == 0, (c, fns.index(fn), "first differing byte", bad[0].tolist())


def test_the_pass_with_its_first_dot_product_handed_in_equals_the_pass_that_forms_it(drv):
    """rails and random frames at every scale 0..12, coefficients on the bound, ordinary and wrapping ones (the clamped dot
    product is the same instruction in both, so they agree there too)"""
    rng = np.random.default_rng(77)
    rnd = [rng.integers(-32768, 32768, 16) for _ in range(60)] + [(rng.integers(-300, 300, 16)) for _ in range(30)]
    frames, c0s, c1s, sps = [], [], [], []
    for x in _rail_frames() + rnd:
        for (c0, c1) in ON_BOUND + ORDINARY + WRAPPING:
            for sp in range(13):
                frames.append(x); c0s.append(c0); c1s.append(c1); sps.append(sp)
    frames = np.ascontiguousarray(np.asarray(frames), np.int16)
    c0, c1, sp = (np.ascontiguousarray(a, np.int32) for a in (c0s, c1s, sps))
    first = drv.fs_check_pass_p0(frames.ctypes.data_as(I16P), c0.ctypes.data_as(INTP), c1.ctypes.data_as(INTP),
                                 sp.ctypes.data_as(INTP), len(frames))
    assert first == -1, ("first differing frame", frames[first].tolist(), int(c0[first]), int(c1[first]), int(sp[first]))
