"""GC-ADPCM encoder on the GPU with the quantise pass that takes its rounding sign from the subtract's borrow
(gc_encode_core.hpp B1-B5) against the oracle, byte for byte: coefficients and start histories given, bytes and the history
the stream ends on compared.  Both lane layouts, one and four time pieces, the plain grid and the persistent kernel.  The
hand-built rows mix, among the eight predictors of ONE channel, ordinary pairs, the zero predictor and (2048, 0) on tie-rich
input, pairs on the pass's coefficient bound (|c0| + |c1| = 30720), one past it, at 32767 and beyond: lanes of the fast pass,
lanes that newly take the reference's loop as written and lanes that always did share a wave."""
import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

N = 14 * 3300 + 4                      # one partial last frame; four pieces of 825 frames
NCH = 72                               # five workgroups of 16 channel slots, the last one half empty; the first 9 rows are the small case
# (c0, c1) per predictor
_MIXED = np.array([[0, 0, 2048, 0, 30720, 0, 30721, 0, 32767, 0, -32768, -32768, 3900, -1900, -15360, -15360],
                   [4095, -2047, 0, -30720, -15360, -15361, 0, 0, 2048, 0, 16384, 16383, 32767, 32767, -28672, 2048],
                   [2048, 0, 0, 0, 1200, 700, -2048, 0, 0, 30720, 20000, 10721, 0, -2048, 3900, -1900]], dtype=np.int16)


def _tie_row(k, n):
    """odd multiples of powers of two, both signs, the power changing every few frames: with the zero predictor and with
    (2048, 0) the distance sits exactly half way between two nibbles, above and below zero (the rounding sign decides)"""
    rng = np.random.default_rng(500 + k)
    t = np.arange(n)
    e = (t // (14 * (3 + k % 3))) % 12                      # 2^e, e = 0..11
    m = 2 * rng.integers(-8, 8, n) + 1                      # odd, -15..15
    return (m * (1 << e)).clip(-32768, 32767).astype(np.int16)


def _rail_row(k, n):
    t = np.arange(n)
    block = (1, 2, 3, 7)[k % 4]
    row = np.where((t // block) % 2 == 0, 32767, -32768)
    held = (t // 211) % 5 == 4
    return np.where(held, 32767 if k % 2 else -32768, row).astype(np.int16)


@pytest.fixture(scope="module")
def case():
    """72 channels: clipped square, sine, full-scale noise with the oracle's coefficients and a hand-built row (tie-rich or
    on the rails) with mixed coefficients, in turn; the oracle's bytes and end history for each, computed once"""
    pcm = np.empty((NCH, N), np.int16)
    coefs = np.empty((NCH, 16), np.int16)
    rng = np.random.default_rng(78)
    h1 = rng.integers(-32768, 32768, NCH).astype(np.int16)
    h2 = rng.integers(-32768, 32768, NCH).astype(np.int16)
    for c in range(NCH):
        kind = c % 4
        if kind < 3:
            pcm[c] = signals.host(("clipped_square", "sine440", "white_full_scale")[kind], 1, N, first_channel=c)[0]
            coefs[c] = po.gc_calculate_coefficients(pcm[c])
        else:
            k = c // 4
            pcm[c] = _tie_row(k, N) if k % 3 else _rail_row(k, N)
            coefs[c] = _MIXED[k % 3]
            if k % 2:
                h1[c] = h2[c] = 0
    want = [po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(NCH)]
    end = [po.gc_decode(want[c], coefs[c], N, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(NCH)]
    return pcm, coefs, h1, h2, np.stack(want), np.stack(end)


@pytest.mark.parametrize("layout", [4, 8])
@pytest.mark.parametrize("nch", [9, NCH])
def test_bytes_and_end_history_match_the_oracle(case, nch, layout):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, end = case
    L = _lib.lib()
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(nch, N, d)
    d_pcm[:, :N] = torch.from_numpy(pcm[:nch]).to(d)
    d_coefs = torch.from_numpy(coefs[:nch].copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1[:nch].copy()).to(d), torch.from_numpy(h2[:nch].copy()).to(d)
    nb = vdev.gc_byte_count(N)
    assert want.shape[1] == nb
    try:
        L.vga_testing_gc_encoder_layout_this_thread(layout)
        for pieces in (1, 4):
            for persistent in (1, 2):
                L.vga_testing_gc_encoder_segments_this_thread(pieces)
                L.vga_testing_gc_encoder_persistent_this_thread(persistent)
                out = vdev.gc_encode(d_pcm, N, d_coefs, hist1=d_h1, hist2=d_h2)
                dec, _ = vdev.gc_decode(out, d_coefs, N, hist1=d_h1, hist2=d_h2)
                torch.cuda.synchronize()
                got = out[:, :nb].cpu().numpy()
                bad = np.argwhere(got != want[:nch])
                assert bad.size == 0, (pieces, persistent, "first differing (channel, byte)", bad[0].tolist())
                assert np.array_equal(dec[:, N - 2:N].cpu().numpy(), end[:nch]), (pieces, persistent)
    finally:
        L.vga_testing_gc_encoder_layout_this_thread(0)
        L.vga_testing_gc_encoder_segments_this_thread(0)
        L.vga_testing_gc_encoder_persistent_this_thread(0)
