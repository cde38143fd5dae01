"""GC-ADPCM encoder, self-served shape (vga_testing_gc_encoder_layout_this_thread(1)) on uniform batches, round 16: the
tail of the piece schedule descends (vga_testing_gc_schedule_this_thread forces big rounds and up to three tail levels), the
groups of eight that the prologue kernel flags as slow-closing keep one coarse tail level, and one launch in front of the
encoder (gc_self_served_prologue_kernel) builds the order table and fills the scratch three memsets used to.

Every encode is held bit for bit against the oracle, channel by channel, with the coefficients the device computed (or the
hand-built ones the case sets); the counters only show that a case walks the path it is about.

Shape: 24 channels x 43 008 samples (3072 frames).  Group 0: ordinary channels of the synthetic set.  Group 1: one
slow-closing tone (channel 93's generator).  Group 2: a channel with hostile coefficients (|c0| + |c1| = 30721 and 40000
among its predictors).  Schedule: 2 big rounds, tails of 256 / 128 / 64 frames."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

SELF_SERVED = 1
NCH, N = 24, 14 * 3072
TAILS = (256, 128, 64)
# (c0, c1) per predictor: ordinary ones, one past the pass's coefficient bound (30721) and one far past it (40000)
_HOSTILE = np.array([0, 0, 3900, -1900, 4095, -2047, 30720, 0, 30721, 0, -15360, -15360, 25000, -15000, 1200, 700], dtype=np.int16)


def _pcm(nch, n):
    from vgaudio_amd import synth
    pcm = synth.generate(nch, n).copy()
    if nch > 11:
        pcm[11] = signals.host("slow_channel_93", 1, n)[0]
    return pcm


def _device_coefs(pcm):
    import torch
    from vgaudio_amd import device as vdev
    nch, n = pcm.shape
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(nch, n, d)
    d_pcm[:, :n] = torch.from_numpy(np.ascontiguousarray(pcm)).to(d)
    coefs = vdev.gc_coefs(d_pcm, n)
    torch.cuda.synchronize()
    return coefs.cpu().numpy().astype(np.int16).reshape(nch, 16)


def _case(pcm, hostile=(18,)):
    """-> pcm, coefs (the device's; hand-built on the hostile channels), the oracle's bytes"""
    coefs = _device_coefs(pcm)
    ref_coefs, _ = po.gc_encode_batch(pcm)
    assert np.array_equal(coefs, ref_coefs)
    for c in hostile:
        if c < len(pcm):
            coefs[c] = _HOSTILE
    want = np.stack([po.gc_encode(pcm[c], coefs[c]) for c in range(len(pcm))])
    return pcm, coefs, want


@pytest.fixture(scope="module")
def whole():
    return _case(_pcm(NCH, N))


def _flagged_groups(coefs):
    from vgaudio_amd import _lib
    order = np.full((len(coefs) + 7) // 8, -1, dtype=np.int32)
    flat = np.ascontiguousarray(coefs, dtype=np.int16)
    slow = _lib.lib().vga_testing_gc_slow_order_host(flat.ctypes.data, len(coefs), order.ctypes.data)
    return sorted(order[:slow].tolist())


def _plan(L, nch, n, coarse):
    out = (C.c_int * 10)()
    groups16 = (nch + 15) // 16
    frames = (n + 13) // 14
    cus = _cus()
    assert L.vga_testing_gc_plan_pieces_n(cus, groups16, frames, C.c_longlong(groups16 * frames), 0, int(coarse), out) == 0
    return list(out)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _encode(case, schedule, handover=True):
    """schedule: None (the default) or (big rounds, three counts) with TAILS.  -> bytes, the nine counters, the two plans"""
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, _ = case
    nch, n = pcm.shape
    L = _lib.lib()
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(nch, n, d)
    d_pcm[:, :n] = torch.from_numpy(np.ascontiguousarray(pcm)).to(d)
    d_coefs = torch.from_numpy(coefs.copy()).to(d)
    stats = (C.c_ulonglong * 9)()
    L.vga_testing_gc_encoder_layout_this_thread(SELF_SERVED)
    if schedule:
        L.vga_testing_gc_schedule_this_thread(schedule[0], (C.c_int * 3)(*schedule[1]), (C.c_int * 3)(*TAILS), TAILS[-1])
    old_hand = L.vga_testing_gc_seam_handover_this_thread(1 if handover else 0)
    try:
        plans = _plan(L, nch, n, False), _plan(L, nch, n, True)
        assert L.vga_testing_gc_encode_stats_n(stats, 9, 1) == 0             # (clears the counters)
        out = vdev.gc_encode(d_pcm, n, d_coefs)
        torch.cuda.synchronize()
        assert L.vga_testing_gc_encode_stats_n(stats, 9, 1) == 0
    finally:
        L.vga_testing_gc_seam_handover_this_thread(old_hand)
        L.vga_testing_gc_schedule_this_thread(0, None, None, 0)
        L.vga_testing_gc_encoder_layout_this_thread(0)
    return out[:, :vdev.gc_byte_count(n)].cpu().numpy(), [int(s) for s in stats], plans


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist(), "of", len(bad))


def test_the_slow_tone_flags_its_group_and_no_other(whole):
    assert _flagged_groups(whole[1]) == [1]


def test_descending_tail_with_the_flagged_group_coarse(whole):
    got, stats, (fine, coarse) = _encode(whole, (2, (2, 2, 2)))
    print("counters", stats, "fine", fine, "coarse", coarse)
    _same(got, whole[2])
    assert fine[3:8] == [256, 2, 128, 2, 64] and coarse[3] == 256 and coarse[4] == 1 << 30, (fine, coarse)
    assert fine[0] > coarse[0] > 1
    # two groups in the fine pieces, one in the coarse ones: every seam was run once, none of another schedule's
    assert stats[0] + stats[1] == 16 * (fine[0] - 1) + 8 * (coarse[0] - 1), (stats, fine, coarse)
    assert stats[6] == 2 * fine[0] + coarse[0]
    assert stats[8] > 0, "the slow tone's seams outlive 256 frames: the kernel must have walked its chain"
    assert stats[5] == 0


def test_descending_tail_without_the_handover_leaves_it_to_the_chain_launch(whole):
    got, stats, (fine, _) = _encode(whole, (2, (2, 2, 2)), handover=False)
    print("counters", stats)
    _same(got, whole[2])
    assert stats[8] == 0 and stats[5] > 0
    assert stats[0] + stats[1] == 24 * (fine[0] - 1)                       # (nobody has the flags: one schedule for all)


def test_default_schedule(whole):
    got, stats, _ = _encode(whole, None)
    print("counters", stats)
    _same(got, whole[2])


@pytest.mark.parametrize("n, counts", [(14 * 3072 - 13, (2, 2, 2)),        # 43 001 samples: a partial last frame
                                       (14 * 1111 + 3, (1, 3, 40)),        # the 64-frame level asked for more pieces than the stream holds
                                       (14 * 700, (9, 9, 9))])             # half the stream is all the tail gets: levels cut short
def test_ragged_stream_ends(n, counts):
    case = _case(_pcm(NCH, n))
    for handover in (True, False):
        got, stats, (fine, coarse) = _encode(case, (2, counts), handover=handover)
        print("counters", stats, "fine", fine, "coarse", coarse)
        _same(got, case[2])


def test_every_group_flagged_takes_the_coarse_pieces():
    n = 14 * 3072
    pcm = signals.host("sine440", 16, n)
    case = _case(pcm, hostile=())
    assert _flagged_groups(case[1]) == [0, 1]
    got, stats, (fine, coarse) = _encode(case, (2, (2, 2, 2)))
    print("counters", stats, "fine", fine, "coarse", coarse)
    _same(got, case[2])
    assert fine[0] != coarse[0]
    assert stats[6] == 2 * coarse[0] and stats[0] + stats[1] == 16 * (coarse[0] - 1), "no fine piece, no fine seam"


def _numpy_rule(coefs):
    """a group of eight is flagged when any predictor of any of its channels has -c1 >= 2040 and complex poles"""
    c0 = coefs[:, 0::2].astype(np.int64)
    c1 = coefs[:, 1::2].astype(np.int64)
    slow = ((-c1 >= 2040) & (c0 * c0 < -8192 * c1)).any(axis=1)
    groups = (len(coefs) + 7) // 8
    flags = np.zeros(groups, bool)
    np.logical_or.at(flags, np.arange(len(coefs)) // 8, slow)
    return flags


@pytest.mark.parametrize("nch", [8, 9, 520, 4096])
@pytest.mark.parametrize("pattern", ["random", "none", "all", "last_partial_group"])
def test_prologue_kernel_on_poisoned_scratch(nch, pattern):
    import torch
    from vgaudio_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(1600 + nch)
    groups = (nch + 7) // 8
    if pattern == "random":                                                # whole-range tables: the rule itself, thresholds and signs
        coefs = rng.integers(-32768, 32768, (nch, 16)).astype(np.int16)
        coefs[rng.integers(0, nch, nch // 2 + 1), 2 * rng.integers(0, 8, nch // 2 + 1) + 1] = rng.integers(-2050, -2030, nch // 2 + 1)
    else:
        coefs = rng.integers(-1500, 1500, (nch, 16)).astype(np.int16)
        which = {"none": [], "all": range(groups), "last_partial_group": [groups - 1]}[pattern]
        for g in which:
            coefs[min(8 * g + int(rng.integers(0, 8)), nch - 1), 2 * int(rng.integers(0, 8)):][:2] = (int(rng.integers(-100, 100)), -2040)
    flags = _numpy_rule(coefs)
    if pattern != "random":
        assert flags.sum() == {"none": 0, "all": groups, "last_partial_group": 1}[pattern]
    table = np.full(2 * groups + 1, -7, dtype=np.int32)
    bad = C.c_int(-1)
    d_coefs = torch.from_numpy(coefs.copy()).to(torch.device("cuda:0"))
    zero_ints = 4 + 2 * 37 * groups                                        # a queue head, 37 seams' counters and words
    s = L.vga_testing_gc_prologue_device(d_coefs.data_ptr(), nch, zero_ints, table.ctypes.data, C.addressof(bad))
    assert s == int(flags.sum()) and table[groups] == s
    assert np.array_equal(table[:groups], np.concatenate([np.flatnonzero(flags), np.flatnonzero(~flags)]))
    assert np.array_equal(table[groups + 1:], flags.astype(np.int32))
    assert bad.value == 0
