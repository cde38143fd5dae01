"""The GC-ADPCM encoder's piece schedule with a descending tail (round 16; gc::plan_encode_pieces_on, gc_encode_kernel.hip),
walked on the host through vga_testing_gc_plan_pieces_n: the self-served shape on uniform batches cuts the end of every
channel into up to three levels of shorter and shorter pieces, and the groups of eight whose seams close slowly keep ONE
tail level of pieces no shorter than 4096 frames -- a schedule of their own (`coarse`), not runs of the fine pieces: the
kernels pick the group's schedule where they pick the group, so nothing has to line up between the two.  What must hold
is that EACH is a partition of [0, frames) into at most 1024 pieces with no empty piece, that the coarse one never cuts a
tail finer than 4096 frames, and that the two-size schedule of before is what comes out wherever the tail does not descend."""
import ctypes as C

import pytest

from vgaudio_amd import _lib

NO_END = 1 << 30
CUS = (1, 8, 256, 304)
CHANNELS = (8, 16, 24, 100, 512, 1024, 2040, 2048, 4096, 8192)
FRAMES = (1, 2, 63, 64, 1000, 3583, 3584, 14335, 14336, 20000, 205715, 1_000_000, 3_000_000)


def _plan(L, cus, channels, frames, coarse):
    groups = (channels + 15) // 16
    out = (C.c_int * 10)()
    assert L.vga_testing_gc_plan_pieces_n(cus, groups, frames, C.c_longlong(groups * frames), 0, int(coarse), out) == 0
    keys = ("pieces", "big", "nb", "small", "n1", "s2", "n2", "s3", "persistent")
    return dict(zip(keys, list(out)[:9]))


def _first(p, k):
    t = max(k - p["nb"], 0)
    a = min(t, p["n1"])
    b = min(t - a, p["n2"])
    return min(k, p["nb"]) * p["big"] + a * p["small"] + b * p["s2"] + (t - a - b) * p["s3"]


def _length(p, k):
    return _first(p, k + 1) - _first(p, k)


def _is_partition(p, frames):
    assert 1 <= p["pieces"] <= 1024, p
    assert _first(p, 0) == 0 and _first(p, p["pieces"]) >= frames, (p, frames)
    assert _first(p, p["pieces"] - 1) < frames, ("an empty piece at the end", p, frames)
    assert all(_length(p, k) > 0 for k in range(p["pieces"])), ("an empty piece", p)


@pytest.fixture()
def self_served():
    L = _lib.lib()
    old = L.vga_testing_gc_encoder_layout_this_thread(1)
    yield L
    L.vga_testing_gc_schedule_this_thread(0, None, None, 0)
    L.vga_testing_gc_encoder_layout_this_thread(old)


def _check_grid(L, min_coarse):
    for cus in CUS:
        for channels in CHANNELS:
            for frames in FRAMES:
                fine, coarse = _plan(L, cus, channels, frames, False), _plan(L, cus, channels, frames, True)
                assert fine["persistent"] == 1 and coarse["persistent"] == 1
                _is_partition(fine, frames)
                _is_partition(coarse, frames)
                # the tail descends
                tail = [_length(fine, k) for k in range(fine["nb"], fine["pieces"])]
                assert tail == sorted(tail, reverse=True), (fine, tail)
                # the coarse schedule has one tail level and no piece shorter than the floor but a channel's only one
                assert coarse["n1"] == NO_END, coarse
                if coarse["pieces"] > 1:
                    assert min(coarse["big"], coarse["small"]) >= min_coarse(frames, coarse), (coarse, frames)


def test_default_schedule_on_the_grid(self_served):
    # (equal pieces -- more than 1024 would be needed, or too few groups for a schedule -- are at least 3584 frames, as ever)
    _check_grid(self_served, lambda frames, p: 4096 if p["small"] != p["big"] else 3584)


@pytest.mark.parametrize("schedule", [(4, (6, 6, 6), (4096, 2048, 1024), 1024), (3, (6, 6, 0), (2048, 1024, 1024), 1024),
                                      (2, (2, 2, 2), (256, 128, 64), 64), (1, (0, 5, 0), (512, 100, 64), 64),
                                      (8, (400, 400, 400), (64, 64, 64), 64)])
def test_forced_schedules_on_the_grid(self_served, schedule):
    L = self_served
    big, counts, sizes, floor = schedule
    L.vga_testing_gc_schedule_this_thread(big, (C.c_int * 3)(*counts), (C.c_int * 3)(*sizes), floor)
    want = max(sizes[0], min(4096, 4 * floor))
    _check_grid(L, lambda frames, p: want if p["pieces"] < 1024 and p["small"] != p["big"] else 1)
    for cus in CUS:
        for channels in CHANNELS:
            for frames in FRAMES:
                fine = _plan(L, cus, channels, frames, False)
                if fine["pieces"] < 1024 and fine["pieces"] > fine["nb"]:
                    assert min(_length(fine, k) for k in range(fine["nb"], fine["pieces"])) >= floor, fine


def test_the_headline_shape_ends_on_three_rounds_of_shorter_items(self_served):
    """4096 channels x 205 715 frames on 256 compute units: 512 groups of eight for 3072 workgroups, six piece indices a
    round -- six pieces of 4096, of 2048 and of 1024 frames behind the big ones, which are whole rounds themselves"""
    fine = _plan(self_served, 256, 4096, 205715, False)
    assert (fine["small"], fine["n1"], fine["s2"], fine["n2"], fine["s3"]) == (4096, 6, 2048, 6, 1024), fine
    assert fine["pieces"] - fine["nb"] == 18 and (fine["nb"] * 512) % 3072 <= 512, fine
    coarse = _plan(self_served, 256, 4096, 205715, True)
    assert (coarse["pieces"], coarse["big"], coarse["nb"], coarse["small"], coarse["n1"]) == (31, 7246, 25, 4096, NO_END), coarse


# (cus, channels, frames) -> pieces, big, nb, small of the schedule before the tail descended: shapes below the schedule's
# threshold (fewer than one group of sixteen per 8 workgroups, or fewer than 4 x 3584 frames), where nothing may change
BEFORE = {(256, 1024, 205715): (16, 12858, 16, 12858),
          (256, 32, 3072): (1, 3072, 1, 3072),
          (256, 4096, 14335): (3, 4779, 3, 4779),
          (304, 304, 10_000_000): (64, 156250, 64, 156250)}
# ... and the two-size schedules it had where it now descends: what the groups that close slowly keep
COARSE_BEFORE = {(256, 4096, 205715): (31, 7246, 25, 4096),
                 (256, 2048, 205715): (51, 4096, 39, 4096),
                 (304, 4096, 205715): (36, 6105, 29, 4096),
                 (256, 8192, 205715): (15, 16119, 12, 4096),
                 (8, 128, 100000): (25, 4096, 19, 4096),
                 (1, 16, 20000): (5, 4096, 3, 4096),
                 (256, 4096, 14336): (4, 4096, 3, 4096),
                 (256, 16384, 3_000_000): (8, 498635, 6, 4096)}


def test_plans_below_the_threshold_are_the_ones_before(self_served):
    for (cus, channels, frames), want in BEFORE.items():
        for coarse in (False, True):
            p = _plan(self_served, cus, channels, frames, coarse)
            assert (p["pieces"], p["big"], p["nb"], p["small"], p["n1"]) == want + (NO_END,), ((cus, channels, frames), p)


def test_slow_groups_keep_the_two_size_schedule_of_before(self_served):
    for (cus, channels, frames), want in COARSE_BEFORE.items():
        p = _plan(self_served, cus, channels, frames, True)
        assert (p["pieces"], p["big"], p["nb"], p["small"], p["n1"]) == want + (NO_END,), ((cus, channels, frames), p)


def test_the_other_shapes_never_descend():
    L = _lib.lib()
    assert L.vga_testing_gc_encoder_layout_this_thread(0) == 0
    L.vga_testing_gc_schedule_this_thread(4, (C.c_int * 3)(6, 6, 6), (C.c_int * 3)(4096, 2048, 1024), 1024)
    try:
        for cus, channels, frames in ((256, 4096, 205715), (256, 2048, 205715), (304, 8192, 1_000_000)):
            p = _plan(L, cus, channels, frames, False)
            assert p["n1"] == NO_END and p == _plan(L, cus, channels, frames, True), p
        assert _plan(L, 256, 4096, 205715, False)["pieces"] == 21          # (the 2 + 1 shape's 3 big rounds and 2 small ones)
    finally:
        L.vga_testing_gc_schedule_this_thread(0, None, None, 0)
