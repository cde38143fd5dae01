"""GC-ADPCM encoder, self-served shape (vga_testing_gc_encoder_layout_this_thread(1)) on uniform batches: open seams are
handed on inside the encode launch (round 15, self_served_seams in gc_encode_kernel.hip), and groups of channels whose seams
are likely to close slowly are taken from the queue first.  Every case encodes twice -- with the hand-over and with
vga_testing_gc_seam_handover_this_thread(0), which leaves every open seam to the chain launch as before -- and holds both
against the oracle: bytes, and the history the stream ends on, from coefficients the test hands in.

Seams that stay open the natural way: a square and a sine whose period is the frame length (14 samples) and the 440 Hz sine,
each next to noise channels in the same group of eight; the forced way: vga_testing_force_open_seams_this_thread 1 (every
seam) and 2 (even seams of every third channel) on the same signals.

Shapes: 9, 17 and 72 channels x 4205 samples in 4 pieces; 24 channels x 57 400 samples in 16 pieces (a chain crosses several
pieces and meets runs that were flagged themselves), and x 57 405, which leaves a partial last frame behind runs that never
meet (the chain launch's own case); 160 channels x 143 367 samples in 160 pieces with tones in every third group.

Counters (vga_testing_gc_encode_stats_n): with the hand-over [5], the channels the chain launch walked, is 0 wherever no run
reaches a partial last frame, and [8], the channels whose chain the kernel walked, equals [5] without it; [1], the seams left
open at the end of their own run, does not depend on the hand-over."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

N = 14 * 300 + 5                       # 4205: a partial last frame; four pieces of 76 frames
LONG_N = 14 * 4100                     # 57 400: sixteen pieces of 257 frames, no partial frame
SELF_SERVED = 1


def _tones(nch, n, first_channel=0):
    """channel c: c % 4 == 0 a square of period 14, 1 a sine of period 14, 2 the 440 Hz sine, each on a noise floor, 3 noise --
    every group of eight holds seams that stay open for good, seams that close after a few hundred frames and seams that
    close at once (a PURE tone is coded without loss: its seams close in one frame)"""
    return signals.tones_in_noise(nch, n, first_channel=first_channel)


def _case(pcm, seed):
    nch, n = pcm.shape
    coefs = np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(nch)]).astype(np.int16)
    rng = np.random.default_rng(seed)
    h1, h2 = rng.integers(-32768, 32768, nch).astype(np.int16), rng.integers(-32768, 32768, nch).astype(np.int16)
    want = np.stack([po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(nch)])
    end = np.stack([po.gc_decode(want[c], coefs[c], n, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(nch)])
    return pcm, coefs, h1, h2, want, end


@pytest.fixture(scope="module")
def short():
    return _case(_tones(72, N), 1501)


@pytest.fixture(scope="module")
def long_even():
    return _case(_tones(24, LONG_N, first_channel=100), 1502)


@pytest.fixture(scope="module")
def long_partial():
    return _case(_tones(24, LONG_N + 5, first_channel=100), 1503)


def _encode(case, nch, pieces, handover, force_open=0):
    """-> bytes, final (two last decoded samples), the nine counters"""
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2 = (a[:nch] for a in case[:4])
    L = _lib.lib()
    d = torch.device("cuda:0")
    n = pcm.shape[1]
    d_pcm = vdev.alloc_pcm(nch, n, d)
    d_pcm[:, :n] = torch.from_numpy(np.ascontiguousarray(pcm)).to(d)
    d_coefs = torch.from_numpy(coefs.copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
    stats = (C.c_ulonglong * 9)()
    L.vga_testing_gc_encoder_layout_this_thread(SELF_SERVED)
    L.vga_testing_gc_encoder_segments_this_thread(pieces)
    old_open = L.vga_testing_force_open_seams_this_thread(force_open)
    old_hand = L.vga_testing_gc_seam_handover_this_thread(1 if handover else 0)
    try:
        assert L.vga_testing_gc_encode_stats_n(stats, 9, 1) == 0         # (clears the counters)
        out = vdev.gc_encode(d_pcm, n, d_coefs, hist1=d_h1, hist2=d_h2)
        torch.cuda.synchronize()
        assert L.vga_testing_gc_encode_stats_n(stats, 9, 1) == 0
        dec, _ = vdev.gc_decode(out, d_coefs, n, hist1=d_h1, hist2=d_h2)
        torch.cuda.synchronize()
    finally:
        L.vga_testing_gc_seam_handover_this_thread(old_hand)
        L.vga_testing_force_open_seams_this_thread(old_open)
        L.vga_testing_gc_encoder_segments_this_thread(0)
        L.vga_testing_gc_encoder_layout_this_thread(0)
    return out[:, :vdev.gc_byte_count(n)].cpu().numpy(), dec[:, n - 2:n].cpu().numpy(), [int(s) for s in stats]


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist(), "of", len(bad))


def _both_ways(case, nch, pieces, force_open, partial_tail):
    want, end = case[4][:nch], case[5][:nch]
    on, on_end, s_on = _encode(case, nch, pieces, True, force_open)
    off, off_end, s_off = _encode(case, nch, pieces, False, force_open)
    print("counters with the hand-over", s_on, "without", s_off)
    _same(off, want)
    _same(on, want)
    assert np.array_equal(on, off)
    assert np.array_equal(on_end, end) and np.array_equal(off_end, end)
    assert s_off[8] == 0
    assert s_on[1] == s_off[1] and s_on[0] == s_off[0], (s_on, s_off)
    assert s_on[8] == s_off[5], (s_on, s_off)
    assert s_off[1] > 0 and s_off[5] > 0, "the case must leave seams open"
    if partial_tail:
        assert s_on[5] <= s_off[5]
    else:
        assert s_on[5] == 0, s_on
    # the kernel's continuations re-encode what the chain launch would have: the same frames, wherever they run
    assert s_on[2] == s_off[2], (s_on, s_off)
    return s_on, s_off


@pytest.mark.parametrize("force_open", [0, 1, 2])
@pytest.mark.parametrize("nch", [9, 17, 72])
def test_four_pieces_match_the_oracle_with_and_without_the_handover(short, nch, force_open):
    _both_ways(short, nch, 4, force_open, partial_tail=True)


@pytest.mark.parametrize("force_open", [0, 1, 2])
def test_chains_across_sixteen_pieces(long_even, force_open):
    s_on, _ = _both_ways(long_even, 24, 16, force_open, partial_tail=False)
    if force_open == 1:
        assert s_on[1] == 24 * 15                                      # every seam of every channel stayed open


@pytest.mark.parametrize("force_open", [0, 1, 2])
def test_a_run_that_never_meets_leaves_the_partial_last_frame_to_the_chain_launch(long_partial, force_open):
    s_on, s_off = _both_ways(long_partial, 24, 16, force_open, partial_tail=True)
    if force_open == 1:
        assert s_on[5] == 24 and s_off[5] == 24                        # every run arrives apart: every tail frame is the chain launch's


def test_no_open_seam_leaves_nothing_to_either():
    pcm = (signals.host("white_full_scale", 17, N, first_channel=900) // 8).astype(np.int16)
    case = _case(pcm, 1504)
    on, on_end, s_on = _encode(case, 17, 4, True)
    off, _, s_off = _encode(case, 17, 4, False)
    _same(on, case[4])
    _same(off, case[4])
    assert np.array_equal(on_end, case[5])
    assert s_on[1] == 0 and s_on[5] == 0 and s_on[8] == 0 and s_off[5] == 0, (s_on, s_off)


def _slow_order(L, coefs, device):
    """the order of the groups of eight and the number of flagged ones, from the host function or the encoder's kernel"""
    import torch
    nch = len(coefs)
    order = np.full((nch + 7) // 8, -1, dtype=np.int32)
    flat = np.ascontiguousarray(coefs, dtype=np.int16)
    if device:
        d_coefs = torch.from_numpy(flat.copy()).to(torch.device("cuda:0"))
        slow = L.vga_testing_gc_slow_order_device(d_coefs.data_ptr(), nch, order.ctypes.data)
    else:
        slow = L.vga_testing_gc_slow_order_host(flat.ctypes.data, nch, order.ctypes.data)
    return slow, order


def test_more_items_than_resident_workgroups_with_flags_on_a_third_of_the_groups():
    from vgaudio_amd import _lib, synth
    nch, n, pieces = 160, 143367, 160
    pcm = synth.generate(nch, n).copy()
    tone_groups = list(range(0, nch // 8, 3))                          # a third of the groups: one never-closing tone each
    for g in tone_groups:
        pcm[8 * g + g % 8] = _tones(1, n, first_channel=4 * g + 1)[0]
    coefs = np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(nch)]).astype(np.int16)
    for g in tone_groups:                                              # ... and a predictor on the unit circle, whatever the search found
        coefs[8 * g + g % 8, 14:16] = (3000, -2048)
    slow, order = _slow_order(_lib.lib(), coefs, device=False)
    assert set(tone_groups) <= set(order[:slow].tolist()) and len(tone_groups) <= slow < nch // 8, (slow, order)
    zeros = np.zeros(nch, dtype=np.int16)
    want = np.stack([po.gc_encode(pcm[c], coefs[c]) for c in range(nch)])
    end = np.stack([po.gc_decode(want[c], coefs[c], n)[-2:] for c in range(nch)])
    _both_ways((pcm, coefs, zeros, zeros, want, end), nch, pieces, 0, partial_tail=True)


@pytest.mark.parametrize("nch", [1, 8, 9, 75, 513, 520, 4096])
@pytest.mark.parametrize("pattern", ["none", "all", "alternate", "random"])
def test_the_device_builds_the_order_of_the_host_function(nch, pattern):
    from vgaudio_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(1505 + nch)
    coefs = rng.integers(-1500, 1500, (nch, 16)).astype(np.int16)       # |c1| below the threshold: nothing flagged
    groups = (nch + 7) // 8
    flagged = {"none": np.zeros(groups, bool), "all": np.ones(groups, bool), "alternate": np.arange(groups) % 2 == 1,
               "random": rng.integers(0, 3, groups) == 0}[pattern]
    for g in np.flatnonzero(flagged):                                  # one channel of the group, one predictor: poles at +-i
        ch = min(8 * g + int(rng.integers(0, 8)), nch - 1)
        p = int(rng.integers(0, 8))
        coefs[ch, 2 * p:2 * p + 2] = (0, -2048)
    slow_h, order_h = _slow_order(L, coefs, device=False)
    slow_d, order_d = _slow_order(L, coefs, device=True)
    assert slow_h == int(flagged.sum()) and slow_d == slow_h
    assert np.array_equal(order_h, np.concatenate([np.flatnonzero(flagged), np.flatnonzero(~flagged)]))
    assert np.array_equal(order_d, order_h)
