"""GC-ADPCM encoder on the GPU in the self-served shape (round 13: one-wave workgroups of eight channel slots that take
(group of eight, piece) items from a queue; each wave is helper and encoder of its own channels, one tile buffer of eight
frames, no workgroup barrier), forced through vga_testing_gc_encoder_layout_this_thread(1) and held against the oracle byte
for byte, coefficients from the oracle:
 (a) partial and full groups of eight: 1, 7, 8, 9, 72 and 75 channels x 4205 samples, in one piece and in four;
 (b) the edges of the eight-frame tile: lengths 1, 13, 14, 15, 111, 112, 113, 335, 336, 337 and 4205, every length as a
     uniform batch and all of them in one ragged batch;
 (c) 72 channels of each of the six signal classes;
 (d) sixteen channels each of full-scale noise and clipped square (the cold block's `generic`, `inexact` and 64-bit keys);
 (e) more items than resident workgroups: 160 channels x 143 367 samples in 160 pieces -- every planned piece is encoded;
 (f) the ragged batch of (b) on 72 channels with the 2 + 1 shape forced: the same bytes."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

N = 14 * 300 + 5                       # 4205: one partial last frame; four pieces of 76 frames (the last one shorter)
NCH = 75                               # ten groups of eight channel slots, the last one with three channels
GROUP_COUNTS = (1, 7, 8, 9, 72, 75)
EDGE_LENGTHS = (1, 13, 14, 15, 111, 112, 113, 335, 336, 337, N)   # 8 frames = 112 samples, 24 frames = 336
EDGE_NCH = 9                           # a full group and one channel
RAGGED_NCH = 72
BIG_NCH, BIG_N, BIG_PIECES = 160, 143367, 160
SELF_SERVED, TWO_PLUS_ONE = 1, 8


def _select(L, shape, pieces):
    L.vga_testing_gc_encoder_layout_this_thread(shape)
    L.vga_testing_gc_encoder_segments_this_thread(pieces)
    if shape == TWO_PLUS_ONE:
        L.vga_testing_gc_encoder_persistent_this_thread(2)


def _reset(L):
    L.vga_testing_gc_encoder_layout_this_thread(0)
    L.vga_testing_gc_encoder_segments_this_thread(0)
    L.vga_testing_gc_encoder_persistent_this_thread(0)


def _histories(nch, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-32768, 32768, nch).astype(np.int16), rng.integers(-32768, 32768, nch).astype(np.int16))


def _oracle(pcm, coefs, h1, h2):
    """the oracle's bytes and the history each stream ends on"""
    nch, n = pcm.shape
    want = np.stack([po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(nch)])
    end = np.stack([po.gc_decode(want[c], coefs[c], n, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(nch)])
    return want, end


def _coefs(pcm):
    return np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(len(pcm))]).astype(np.int16)


@pytest.fixture(scope="module")
def mixed():
    """75 channels, the six signal classes in turn (every wave holds each of them)"""
    pcm = np.stack([signals.host(signals.CLASSES[c % len(signals.CLASSES)], 1, N, first_channel=c)[0] for c in range(NCH)])
    coefs = _coefs(pcm)
    h1, h2 = _histories(NCH, 1301)
    return (pcm, coefs, h1, h2) + _oracle(pcm, coefs, h1, h2)


@pytest.fixture(scope="module")
def loud():
    """sixteen channels each of full-scale noise and clipped square"""
    pcm = np.concatenate([signals.host("white_full_scale", 16, N, first_channel=200),
                          signals.host("clipped_square", 16, N, first_channel=300)])
    coefs = _coefs(pcm)
    h1, h2 = _histories(len(pcm), 1302)
    return (pcm, coefs, h1, h2) + _oracle(pcm, coefs, h1, h2)


def _encode_uniform(pcm, coefs, h1, h2, pieces, shape=SELF_SERVED):
    import torch
    from vgaudio_amd import _lib, device as vdev
    L = _lib.lib()
    d = torch.device("cuda:0")
    nch, n = pcm.shape
    d_pcm = vdev.alloc_pcm(nch, n, d)
    d_pcm[:, :n] = torch.from_numpy(np.ascontiguousarray(pcm)).to(d)
    d_coefs = torch.from_numpy(coefs.copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
    try:
        _select(L, shape, pieces)
        out = vdev.gc_encode(d_pcm, n, d_coefs, hist1=d_h1, hist2=d_h2)
        dec, _ = vdev.gc_decode(out, d_coefs, n, hist1=d_h1, hist2=d_h2)
        torch.cuda.synchronize()
    finally:
        _reset(L)
    return out[:, :vdev.gc_byte_count(n)].cpu().numpy(), dec[:, max(n - 2, 0):n].cpu().numpy()


def _encode_ragged(pcm, coefs, h1, h2, lengths, pieces, shape):
    import torch
    from vgaudio_amd import _lib, device as vdev
    L = _lib.lib()
    d = torch.device("cuda:0")
    try:
        _select(L, shape, pieces)                  # (the batch plans its pieces when it is made)
        batch = vdev.GcRaggedBatch(lengths, d)
        try:
            d_pcm = batch.put_pcm(batch.alloc_pcm(), [pcm[c][:n] for c, n in enumerate(lengths)])
            d_coefs = torch.from_numpy(coefs.copy()).to(d)
            d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
            out = batch.encode(d_pcm, d_coefs, hist1=d_h1, hist2=d_h2)
            torch.cuda.synchronize()
            return batch.rows(out, batch.adpcm_offsets, batch.byte_counts)
        finally:
            batch.close()
    finally:
        _reset(L)


def _same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist(), "of", len(bad))


@pytest.mark.parametrize("pieces", [1, 4])
@pytest.mark.parametrize("nch", GROUP_COUNTS)
def test_partial_and_full_groups_match_the_oracle(mixed, nch, pieces):
    pcm, coefs, h1, h2, want, end = mixed
    got, got_end = _encode_uniform(pcm[:nch], coefs[:nch], h1[:nch], h2[:nch], pieces)
    _same(got, want[:nch])
    assert np.array_equal(got_end, end[:nch])


@pytest.mark.parametrize("n", EDGE_LENGTHS)
def test_tile_edges_uniform_match_the_oracle(mixed, n):
    pcm, coefs, h1, h2, want, _ = mixed
    k = EDGE_NCH
    exp = want[:k] if n == N else np.stack([po.gc_encode(pcm[c][:n], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(k)])
    got, _ = _encode_uniform(pcm[:k, :n], coefs[:k], h1[:k], h2[:k], 1)
    _same(got, exp)


def _ragged_lengths(nch):
    lengths = [EDGE_LENGTHS[(c + c // 8) % len(EDGE_LENGTHS)] for c in range(nch)]
    assert set(lengths) == set(EDGE_LENGTHS)
    return lengths


def _ragged_expected(mixed, lengths):
    pcm, coefs, h1, h2, want, _ = mixed
    return [want[c] if n == N else po.gc_encode(pcm[c][:n], coefs[c], hist1=int(h1[c]), hist2=int(h2[c]))
            for c, n in enumerate(lengths)]


@pytest.mark.parametrize("pieces", [1, 4])
def test_tile_edges_ragged_match_the_oracle(mixed, pieces):
    pcm, coefs, h1, h2, _, _ = mixed
    lengths = _ragged_lengths(RAGGED_NCH)
    k = RAGGED_NCH
    rows = _encode_ragged(pcm[:k], coefs[:k], h1[:k], h2[:k], lengths, pieces, SELF_SERVED)
    for c, (n, exp) in enumerate(zip(lengths, _ragged_expected(mixed, lengths))):
        assert np.array_equal(rows[c], exp), ("channel", c, "length", n)


def test_ragged_batch_gives_the_same_bytes_in_the_two_plus_one_shape(mixed):
    pcm, coefs, h1, h2, _, _ = mixed
    lengths = _ragged_lengths(RAGGED_NCH)
    k = RAGGED_NCH
    new = _encode_ragged(pcm[:k], coefs[:k], h1[:k], h2[:k], lengths, 4, SELF_SERVED)
    old = _encode_ragged(pcm[:k], coefs[:k], h1[:k], h2[:k], lengths, 4, TWO_PLUS_ONE)
    for c, n in enumerate(lengths):
        assert np.array_equal(new[c], old[c]), ("channel", c, "length", n)


@pytest.mark.parametrize("cls", signals.CLASSES[:6])
def test_signal_classes_match_the_oracle(cls):
    assert len(signals.CLASSES) >= 6
    pcm = signals.host(cls, 72, N, first_channel=1000)
    coefs = _coefs(pcm)
    h1, h2 = _histories(72, 1303)
    want, end = _oracle(pcm, coefs, h1, h2)
    got, got_end = _encode_uniform(pcm, coefs, h1, h2, 4)
    _same(got, want)
    assert np.array_equal(got_end, end)


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
    groups = (BIG_NCH + 7) // 8
    planned = groups * ((frames + per_piece - 1) // per_piece)
    resident = 12 * torch.cuda.get_device_properties(0).multi_processor_count     # twelve one-wave workgroups per compute unit
    assert pieces == BIG_PIECES and groups * pieces == 3200
    assert groups * pieces > resident and planned > resident, (groups * pieces, planned, resident)
    d_pcm = vdev.alloc_pcm(BIG_NCH, BIG_N, d)
    d_pcm[:, :BIG_N] = torch.from_numpy(host).to(d)
    d_coefs = torch.from_numpy(wc.copy()).to(d)
    stats = (C.c_ulonglong * 8)()
    L.vga_testing_gc_encode_stats.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    try:
        _select(L, SELF_SERVED, BIG_PIECES)
        assert L.vga_testing_gc_encode_stats(stats, 1) == 0          # (clears the counters)
        out = vdev.gc_encode(d_pcm, BIG_N, d_coefs)
        torch.cuda.synchronize()
        assert L.vga_testing_gc_encode_stats(stats, 1) == 0
    finally:
        _reset(L)
    _same(out[:, :vdev.gc_byte_count(BIG_N)].cpu().numpy(), wa)
    assert stats[6] == planned, ("pieces encoded", int(stats[6]), "planned", planned)
