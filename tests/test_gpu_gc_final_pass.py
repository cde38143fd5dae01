"""GC-ADPCM encoder on the GPU with the frame resolution of round 11 -- the pass at s1 for its overflow, ONE final pass at
the lane's own scale, the flags from the two overflows (gc_encode_core.hpp final_pass_pair, frame_flags) -- against the oracle,
byte for byte: coefficients and start histories given, bytes and the history the stream ends on compared.  The (channel,
predictor) layout, one and four time pieces, the plain grid and the persistent kernel, a uniform batch and a ragged one.
Channels 0..7 (ONE encoder wave) are hand-built: their frames put lanes the reference ends at s1 for, lanes at the cap,
lanes in the bump loop, third-trip lanes and a lane one past the coefficient bound side by side; the fixture proves that
from the oracle's own trajectory with the host driver of tests/test_host_gc_final_pass.py."""
import numpy as np
import pytest

from oracle import pyoracle as po
from test_host_gc_final_pass import BUMP_A, COLD, FIN_A, FINAL_SP, GENERIC, I16P, RESUME, _many, drv  # noqa: F401 (drv: fixture)
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

FRAMES = 300
N = 14 * FRAMES + 5                    # one partial last frame; four pieces of 76 frames (the last one shorter)
NCH = 72                               # five workgroups of 16 channel slots, the last one half empty
RAGGED_LENGTHS = (1, 13, 14, 15, N)
# (c0, c1) per predictor of the hand-built channels: the zero predictor, three ordinary ones, one that doubles its error
# every sample, one ON the pass's coefficient bound (|c0| + |c1| = 30720: fifteen times the last error), one PAST it (30721:
# the reference's loop as written), one on the bound with both taps
_HAND = np.array([0, 0, 3900, -1900, 4095, -2047, 30720, 0, 30721, 0, -15360, -15360, 2048, 0, 1200, 700], dtype=np.int16)


def _hand_row(c, n):
    """a tone whose level moves through 30, 300, 3000 and 30000 every eight frames, each channel at another step of it:
    at any frame the wave's eight channels hold quiet and loud frames side by side"""
    t = np.arange(n)
    rng = np.random.default_rng(1100 + c)
    amp = np.array([30, 300, 3000, 30000])[((t // (14 * 8)) + c) % 4]
    v = amp * np.sin(0.3 * t + c) + rng.integers(-3, 4, n)
    return v.clip(-32768, 32767).astype(np.int16)


def _lane_kinds(L, pcm, coefs, h1, h2, want):
    """per (frame, predictor) of one channel, along the oracle's trajectory: the info rows of the host driver"""
    dec = po.gc_decode(want, coefs, N, hist1=int(h1), hist2=int(h2)).astype(np.int64)
    x = np.concatenate([[int(h2), int(h1)], dec])                      # x[14 f], x[14 f + 1]: the history of frame f
    frames = np.zeros((FRAMES, 16), np.int16)
    for f in range(FRAMES):
        frames[f, :2] = x[14 * f:14 * f + 2]
        frames[f, 2:] = pcm[14 * f:14 * f + 14]
    out = np.zeros((FRAMES, 8, 9), np.int32)
    for p in range(8):
        c0, c1 = int(coefs[2 * p]), int(coefs[2 * p + 1])
        s1 = np.array([L.fp_first_scale(frames[f].ctypes.data_as(I16P), c0, c1) for f in range(FRAMES)], np.int32)
        out[:, p] = _many(L, frames, c0, c1, s1, 0)[1]
    return out


@pytest.fixture(scope="module")
def case(drv):  # noqa: F811
    """72 channels: eight hand-built ones, sixteen each of full-scale noise, clipped square and sine with the oracle's
    coefficients, sixteen with the hand-built coefficients on noise and squares; the oracle's bytes and end history for
    each, computed once"""
    pcm = np.empty((NCH, N), np.int16)
    coefs = np.empty((NCH, 16), np.int16)
    rng = np.random.default_rng(79)
    h1 = rng.integers(-32768, 32768, NCH).astype(np.int16)
    h2 = rng.integers(-32768, 32768, NCH).astype(np.int16)
    for c in range(NCH):
        if c < 8:
            pcm[c] = _hand_row(c, N)
            coefs[c] = _HAND
            h1[c] = h2[c] = 0
        elif c < 56:
            pcm[c] = signals.host(("white_full_scale", "clipped_square", "sine440")[(c - 8) // 16], 1, N, first_channel=c)[0]
            coefs[c] = po.gc_calculate_coefficients(pcm[c])
        else:
            pcm[c] = signals.host(("white_full_scale", "clipped_square")[c % 2], 1, N, first_channel=c)[0]
            coefs[c] = _HAND
    want = [po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(NCH)]
    end = [po.gc_decode(want[c], coefs[c], N, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(NCH)]
    # the hand-built wave: at some frame index its 64 lanes hold every kind at once
    kinds = np.stack([_lane_kinds(drv, pcm[c], coefs[c], h1[c], h2[c], want[c]) for c in range(8)], axis=1)   # [frame, channel, predictor, 9]
    k = kinds.reshape(FRAMES, 64, 9)
    ok = k[:, :, GENERIC] == 0
    fin_a = ((k[:, :, FIN_A] == 1) & (k[:, :, COLD] == 0)).any(1)
    cap = ((k[:, :, FINAL_SP] == 12) & ok).any(1)
    bump = (k[:, :, BUMP_A] == 1).any(1)
    third = (k[:, :, RESUME] == 1).any(1)
    together = fin_a & cap & bump & third              # (the lane at 30721 is in every frame of every one of the eight channels)
    assert together.any(), (int(fin_a.sum()), int(cap.sum()), int(bump.sum()), int(third.sum()))
    assert int(np.abs(_HAND[8:10].astype(np.int64)).sum()) == 30721
    return pcm, coefs, h1, h2, np.stack(want), np.stack(end)


_KERNELS = [(1, 1), (1, 2), (4, 1), (4, 2)]           # (time pieces, 1 = plain grid / 2 = persistent kernel)


def _select(L, pieces, persistent):
    L.vga_testing_gc_encoder_layout_this_thread(8)
    L.vga_testing_gc_encoder_segments_this_thread(pieces)
    L.vga_testing_gc_encoder_persistent_this_thread(persistent)


def _reset(L):
    L.vga_testing_gc_encoder_layout_this_thread(0)
    L.vga_testing_gc_encoder_segments_this_thread(0)
    L.vga_testing_gc_encoder_persistent_this_thread(0)


@pytest.mark.parametrize("pieces,persistent", _KERNELS)
def test_uniform_batch_matches_the_oracle(case, pieces, persistent):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, end = case
    L = _lib.lib()
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(NCH, N, d)
    d_pcm[:, :N] = torch.from_numpy(pcm).to(d)
    d_coefs = torch.from_numpy(coefs.copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
    nb = vdev.gc_byte_count(N)
    assert want.shape[1] == nb
    try:
        _select(L, pieces, persistent)
        out = vdev.gc_encode(d_pcm, N, d_coefs, hist1=d_h1, hist2=d_h2)
        dec, _ = vdev.gc_decode(out, d_coefs, N, hist1=d_h1, hist2=d_h2)
        torch.cuda.synchronize()
    finally:
        _reset(L)
    got = out[:, :nb].cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist())
    assert np.array_equal(dec[:, N - 2:N].cpu().numpy(), end)


@pytest.mark.parametrize("pieces,persistent", _KERNELS)
def test_ragged_batch_matches_the_oracle(case, pieces, persistent):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, _ = case
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
            _select(L, pieces, persistent)
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
