"""GC-ADPCM encoder on the GPU with the tile head's pre-scan in the numerator domain (round 14: gc_encode_core.hpp
prescan_numer_word, N1 and N3-N7, behind a wave-uniform flag; a wave with a hostile channel keeps the unchecked sum and the
quotient) held against the oracle, bytes and final histories, with coefficients given by the test.  Every case runs in the
self-served shape, with the 2 + 1 shape forced, and on the default path of a small batch:
 (a) 9 and 17 channels x 4205 samples in one and four pieces, coefficients handcrafted so that the dividend D of a sample's
     prediction is a chosen input sample ((0, 1), (1, 0), (0, -1), (2047, 1), ...) or 2048 times one ((0, 2048), (2048, 0), ...),
     on frames whose samples sit at 0, +-1, +-2047, +-2048, +-2049 and at 2^j - 1, 2^j, 2^j + 1: D at and next to the multiples
     of 2048, distances at and next to the values where the first scale changes;
 (b) groups of eight with one hostile channel (|c0| + |c1| of 30721, and of 40000) among clean ones, next to a clean group:
     both sides of the flag in one launch;
 (c) lengths 1, 13, 14, 15, 113 and 4205 as one ragged batch;
 (d) eight channels each of silence, full-scale noise and clipped square.
The form is compiled into the self-served shape; the other two shapes run the loop they had and are held to the same bytes.
What this file holds is the plumbing: the flag and both sides of it in one launch, the negated pairs through ds_bpermute, the
rolled fallback's addressing, ragged and partial frames.  It does NOT see an arithmetic slip of one in a distance: with the
bias 2047 -> 2048 or the sign test the wrong way compiled in (every shape, scratch builds), 0 of the 24 cases fail, where
tests/test_host_gc_prescan_numer.py counts 24 831 and 851 725 differing words of 1 046 392.  A distance off by one moves the
first scale only at a bracket's edge, and there the reference's loop reaches the same final scale from either start (it
begins one scale low and walks up): the bytes depend on the lowest scale that passes, not on where the search began
(LABNOTES 19.10).  The arithmetic is the host file's to hold."""
import numpy as np
import pytest

from oracle import pyoracle as po
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

N = 14 * 300 + 5                       # 4205: one partial last frame; four pieces of 76 frames (the last one shorter)
SELF_SERVED, TWO_PLUS_ONE, DEFAULT = 1, 8, 0
SHAPES = (SELF_SERVED, TWO_PLUS_ONE, DEFAULT)
RAGGED_LENGTHS = (1, 13, 14, 15, 113, N)

# (c0, c1) per predictor.  D = x[s] * c1 + x[s + 1] * c0: rows 0 and 1 make D an input sample (and sample + 2047 * next), row 2
# makes it 2048 times one, so that the quotient is the sample itself and D is a multiple of 2048 whenever it is not zero
_CRAFTED = np.array([[0, 1, 1, 0, 0, -1, -1, 0, 2047, 1, 1, 2047, -2047, 1, 2047, -1],
                     [1, 1, 1, -1, 0, 2047, 2049, 0, 0, -2049, 3, 5, 4095, -2047, 0, 0],
                     [0, 2048, 2048, 0, 0, -2048, -2048, 0, 2048, 2048, 2048, -2048, 4096, -2048, 0, 4096],
                     [3900, -1900, 0, 1, 2048, 0, 1, 0, 0, 2048, 2047, 1, 0, -2048, 30719, 1]], dtype=np.int16)


def _crafted_row(rng, n):
    """per frame one magnitude A = 2^j; the samples sit at and next to 0, +-2047 / 2048 / 2049 and +-A"""
    frames = (n + 13) // 14
    out = np.empty(frames * 14, np.int64)
    for f in range(frames):
        a = 1 << int(rng.integers(3, 15))
        near = np.array([0, 1, -1, 2, -2, a - 1, a, a + 1, 1 - a, -a, -a - 1, 2047, 2048, 2049, -2047, -2048, -2049,
                         (9 * a) // 8 - 1, (9 * a) // 8, -((9 * a) // 8), 1 - (9 * a) // 8])
        near = near[np.abs(near) <= max(a + 1, 8) if f % 3 else np.ones(len(near), bool)]
        out[f * 14:(f + 1) * 14] = rng.choice(near, 14)
    return np.clip(out[:n], -32768, 32767).astype(np.int16)


def _histories(nch, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-32768, 32768, nch).astype(np.int16), rng.integers(-32768, 32768, nch).astype(np.int16))


def _oracle(pcm, coefs, h1, h2):
    nch, n = pcm.shape
    want = np.stack([po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(nch)])
    end = np.stack([po.gc_decode(want[c], coefs[c], n, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(nch)])
    return want, end


@pytest.fixture(scope="module")
def crafted():
    rng = np.random.default_rng(1401)
    nch = 17
    pcm = np.stack([_crafted_row(rng, N) for _ in range(nch)])
    coefs = np.stack([_CRAFTED[c % len(_CRAFTED)] for c in range(nch)])
    h1, h2 = _histories(nch, 1402)
    h1[:4], h2[:4] = (2047, -2048, 2049, 0), (-1, 2048, 0, -2049)
    return (pcm, coefs, h1, h2) + _oracle(pcm, coefs, h1, h2)


@pytest.fixture(scope="module")
def flagged():
    """24 channels: a group of eight with one channel at |c0| + |c1| = 30721, one with one at 40000, a clean group"""
    rng = np.random.default_rng(1403)
    nch = 24
    pcm = np.stack([_crafted_row(rng, N) if c % 3 else signals.host("white_full_scale", 1, N, first_channel=c)[0] for c in range(nch)])
    coefs = np.stack([_CRAFTED[c % len(_CRAFTED)] for c in range(nch)])
    coefs[3, 4:8] = (30720, -1, -15361, -15360)                         # two predictors of channel 3: the sum is 30721
    coefs[13, 0:6] = (20000, 20000, -32768, -7232, 32767, 7233)        # three of channel 13: 40000
    pcm[3], pcm[13] = signals.host("clipped_square", 2, N, first_channel=7)
    assert [int(np.abs(coefs[c].astype(int)).reshape(8, 2).sum(1).max()) for c in (3, 13)] == [30721, 40000]
    assert all(np.abs(coefs[c].astype(int)).reshape(8, 2).sum(1).max() <= 30720 for c in range(nch) if c not in (3, 13))
    h1, h2 = _histories(nch, 1404)
    return (pcm, coefs, h1, h2) + _oracle(pcm, coefs, h1, h2)


@pytest.fixture(scope="module")
def classes():
    pcm = np.concatenate([signals.host(cls, 8, N, first_channel=500 + 8 * i)
                          for i, cls in enumerate(("silence", "white_full_scale", "clipped_square"))])
    coefs = np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(len(pcm))]).astype(np.int16)
    h1, h2 = _histories(len(pcm), 1405)
    return (pcm, coefs, h1, h2) + _oracle(pcm, coefs, h1, h2)


def _select(L, shape, pieces):
    L.vga_testing_gc_encoder_layout_this_thread(shape)
    if shape != DEFAULT:
        L.vga_testing_gc_encoder_segments_this_thread(pieces)
    if shape == TWO_PLUS_ONE:
        L.vga_testing_gc_encoder_persistent_this_thread(2)


def _reset(L):
    L.vga_testing_gc_encoder_layout_this_thread(0)
    L.vga_testing_gc_encoder_segments_this_thread(0)
    L.vga_testing_gc_encoder_persistent_this_thread(0)


def _check_uniform(case, nch, pieces, shape):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, end = (v[:nch] for v in case)
    L = _lib.lib()
    d = torch.device("cuda:0")
    n = pcm.shape[1]
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
    got = out[:, :vdev.gc_byte_count(n)].cpu().numpy()
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist(), "of", len(bad))
    assert np.array_equal(dec[:, n - 2:n].cpu().numpy(), end)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pieces", [1, 4])
@pytest.mark.parametrize("nch", [9, 17])
def test_dividends_at_the_multiples_of_2048_match_the_oracle(crafted, nch, pieces, shape):
    _check_uniform(crafted, nch, pieces, shape)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pieces", [1, 4])
def test_hostile_and_clean_groups_in_one_launch_match_the_oracle(flagged, pieces, shape):
    _check_uniform(flagged, 24, pieces, shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_silence_noise_and_clipped_square_match_the_oracle(classes, shape):
    _check_uniform(classes, 24, 4, shape)


@pytest.mark.parametrize("shape", SHAPES)
def test_ragged_lengths_match_the_oracle(crafted, shape):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, _ = (v[:12] for v in crafted)
    lengths = [RAGGED_LENGTHS[(c + c // 6) % 6] for c in range(12)]
    assert sorted(set(lengths)) == sorted(RAGGED_LENGTHS)
    L = _lib.lib()
    d = torch.device("cuda:0")
    try:
        _select(L, shape, 4)                       # (the batch plans its pieces when it is made)
        batch = vdev.GcRaggedBatch(lengths, d)
        try:
            d_pcm = batch.put_pcm(batch.alloc_pcm(), [pcm[c][:n] for c, n in enumerate(lengths)])
            d_coefs = torch.from_numpy(coefs.copy()).to(d)
            d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
            out = batch.encode(d_pcm, d_coefs, hist1=d_h1, hist2=d_h2)
            torch.cuda.synchronize()
            rows = batch.rows(out, batch.adpcm_offsets, batch.byte_counts)
        finally:
            batch.close()
    finally:
        _reset(L)
    for c, n in enumerate(lengths):
        exp = want[c] if n == N else po.gc_encode(pcm[c][:n], coefs[c], hist1=int(h1[c]), hist2=int(h2[c]))
        assert np.array_equal(rows[c], exp), ("channel", c, "length", n)
