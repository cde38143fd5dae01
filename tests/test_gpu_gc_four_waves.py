"""GC-ADPCM encoder on the GPU as the persistent kernel runs since round 12 -- a (channel slot, frame)'s row, pre-scan words
and record in one LDS slot reached from one address, the frame's flags as one bit with the single flags derived inside the
cold branch, a ragged slot's "this frame is mine" from the row's spare dword -- against the oracle, byte for byte,
coefficients from the oracle.  (Written for the round's build at four waves per SIMD and five workgroups per compute unit,
which was measured and not kept; the cases hold for either.)  The persistent kernel is forced
(vga_testing_gc_encoder_persistent_this_thread(2)):
 (a) 72 channels x 4205 samples, one and four pieces, uniform and ragged (lengths 1, 13, 14, 15, 4205);
 (b) more items than resident workgroups: 160 channels x 143 367 samples cut into 160 pieces -- the queue, the seam counters
     and the two-ended seam closing run with late-coming items -- and every planned piece is encoded;
 (c) sixteen channels each of full-scale noise and clipped square: `generic`, `inexact` and the 64-bit keys are frequent."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

N = 14 * 300 + 5                       # 4205: one partial last frame; four pieces of 76 frames (the last one shorter)
NCH = 72                               # five workgroups of 16 channel slots, the last one half empty
RAGGED_LENGTHS = (1, 13, 14, 15, N)
BIG_NCH, BIG_N, BIG_PIECES = 160, 143367, 160


def _select(L, pieces):
    L.vga_testing_gc_encoder_layout_this_thread(8)
    L.vga_testing_gc_encoder_segments_this_thread(pieces)
    L.vga_testing_gc_encoder_persistent_this_thread(2)


def _reset(L):
    L.vga_testing_gc_encoder_layout_this_thread(0)
    L.vga_testing_gc_encoder_segments_this_thread(0)
    L.vga_testing_gc_encoder_persistent_this_thread(0)


def _oracle(pcm, seed):
    """oracle coefficients, random start histories, the oracle's bytes and the history each stream ends on"""
    nch, n = pcm.shape
    rng = np.random.default_rng(seed)
    h1 = rng.integers(-32768, 32768, nch).astype(np.int16)
    h2 = rng.integers(-32768, 32768, nch).astype(np.int16)
    coefs = np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(nch)]).astype(np.int16)
    want = np.stack([po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(nch)])
    end = np.stack([po.gc_decode(want[c], coefs[c], n, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(nch)])
    return coefs, h1, h2, want, end


@pytest.fixture(scope="module")
def mixed():
    """72 channels, the six signal classes in turn (every encoder wave holds each of them)"""
    pcm = np.stack([signals.host(signals.CLASSES[c % len(signals.CLASSES)], 1, N, first_channel=c)[0] for c in range(NCH)])
    return (pcm,) + _oracle(pcm, 1201)


@pytest.fixture(scope="module")
def loud():
    """sixteen channels each of full-scale noise and clipped square"""
    pcm = np.concatenate([signals.host("white_full_scale", 16, N, first_channel=200),
                          signals.host("clipped_square", 16, N, first_channel=300)])
    return (pcm,) + _oracle(pcm, 1202)


def _encode_uniform(pcm, coefs, h1, h2, pieces):
    import torch
    from vgaudio_amd import _lib, device as vdev
    L = _lib.lib()
    d = torch.device("cuda:0")
    nch, n = pcm.shape
    d_pcm = vdev.alloc_pcm(nch, n, d)
    d_pcm[:, :n] = torch.from_numpy(pcm).to(d)
    d_coefs = torch.from_numpy(coefs.copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
    try:
        _select(L, pieces)
        out = vdev.gc_encode(d_pcm, n, d_coefs, hist1=d_h1, hist2=d_h2)
        dec, _ = vdev.gc_decode(out, d_coefs, n, hist1=d_h1, hist2=d_h2)
        torch.cuda.synchronize()
    finally:
        _reset(L)
    return out[:, :vdev.gc_byte_count(n)].cpu().numpy(), dec[:, n - 2:n].cpu().numpy()


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist(), "of", len(bad))


@pytest.mark.parametrize("pieces", [1, 4])
def test_uniform_batch_matches_the_oracle(mixed, pieces):
    pcm, coefs, h1, h2, want, end = mixed
    got, got_end = _encode_uniform(pcm, coefs, h1, h2, pieces)
    _same(got, want)
    assert np.array_equal(got_end, end)


@pytest.mark.parametrize("pieces", [1, 4])
def test_ragged_batch_matches_the_oracle(mixed, pieces):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, _ = mixed
    L = _lib.lib()
    d = torch.device("cuda:0")
    lengths = [RAGGED_LENGTHS[(c + c // 8) % 5] for c in range(NCH)]      # every wave holds every length
    assert lengths[:8].count(N) >= 1 and set(lengths) == set(RAGGED_LENGTHS)
    batch = vdev.GcRaggedBatch(lengths, d)
    try:
        d_pcm = batch.put_pcm(batch.alloc_pcm(), [pcm[c][:n] for c, n in enumerate(lengths)])
        d_coefs = torch.from_numpy(coefs.copy()).to(d)
        d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
        try:
            _select(L, pieces)
            out = batch.encode(d_pcm, d_coefs, hist1=d_h1, hist2=d_h2)
            torch.cuda.synchronize()
        finally:
            _reset(L)
        rows = batch.rows(out, batch.adpcm_offsets, batch.byte_counts)
    finally:
        batch.close()
    for c, n in enumerate(lengths):
        exp = want[c] if n == N else po.gc_encode(pcm[c][:n], coefs[c], hist1=int(h1[c]), hist2=int(h2[c]))
        assert np.array_equal(rows[c], exp), ("channel", c, "length", n)


@pytest.mark.parametrize("pieces", [1, 4])
def test_loud_signals_match_the_oracle(loud, pieces):
    pcm, coefs, h1, h2, want, end = loud
    got, got_end = _encode_uniform(pcm, coefs, h1, h2, pieces)
    _same(got, want)
    assert np.array_equal(got_end, end)


def test_more_items_than_resident_workgroups():
    import torch
    from vgaudio_amd import _lib, device as vdev, synth
    L = _lib.lib()
    d = torch.device("cuda:0")
    host = synth.generate(BIG_NCH, BIG_N)
    wc, wa = po.gc_encode_batch(host, threads=4)
    frames = (BIG_N + 13) // 14
    assert frames == 10241 and BIG_N % 14 != 0
    # the schedule the test hook asks for: 160 equal pieces; the ones that begin past the channels' end do not exist
    pieces = min(max(frames // 64, 1), BIG_PIECES)
    per_piece = (frames + pieces - 1) // pieces
    groups = (BIG_NCH + 15) // 16
    planned = groups * ((frames + per_piece - 1) // per_piece)
    resident = 5 * torch.cuda.get_device_properties(0).multi_processor_count     # (five per compute unit is the most a build can hold)
    assert pieces == BIG_PIECES and groups * pieces == 1600
    assert groups * pieces > resident and planned > resident, (groups * pieces, planned, resident)
    d_pcm = vdev.alloc_pcm(BIG_NCH, BIG_N, d)
    d_pcm[:, :BIG_N] = torch.from_numpy(host).to(d)
    d_coefs = torch.from_numpy(wc.copy()).to(d)
    stats = (C.c_ulonglong * 8)()
    L.vga_testing_gc_encode_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    try:
        _select(L, BIG_PIECES)
        assert L.vga_testing_gc_encode_stats(stats, 1) == 0          # (clears the counters)
        out = vdev.gc_encode(d_pcm, BIG_N, d_coefs)
        torch.cuda.synchronize()
        assert L.vga_testing_gc_encode_stats(stats, 1) == 0
    finally:
        _reset(L)
    _same(out[:, :vdev.gc_byte_count(BIG_N)].cpu().numpy(), wa)
    assert stats[6] == planned, ("pieces encoded", int(stats[6]), "planned", planned)
