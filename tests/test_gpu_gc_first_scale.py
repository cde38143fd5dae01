"""GC-ADPCM encoder on the GPU with the first-scale work off the quotient (gc_encode_core.hpp F1-F5, N1-N2, round 9) against
the oracle, byte for byte.  Two shapes, because the tails and the launch forms cannot be had in one:

* 24 channels x (14 x 37 + 5) samples: one full workgroup of sixteen channel slots and a partial one, a partial last tile, a
  zero-padded last frame.  38 frames are ONE piece whatever the hooks say (a piece has at least 64 frames), so the forms
  named below all come down to the plain grid kernel (both lane layouts) or the persistent kernel on a single piece, with no
  seam: the test asserts exactly that (one piece planned, one piece per channel group encoded, no seam run).  Also the ragged
  `_v` entry point with lengths 5, 14, 15 and 523.
* 72 channels x (14 x 192 + 5) samples, the smallest shape that makes three pieces (193 frames, the segments hook at 3; 72 > 64
  channels so that the lane-per-candidate layout takes the sixteen-lane seam and chain kernels): the plain grid plus the seam
  and chain launches in both layouts, and persistent workgroups on uniform pieces -- later pieces start from guessed history,
  the seam runs re-encode from the true one and call the rewritten first scale.  Each with the seams as they fall and with
  `vga_testing_force_open_seams_this_thread(1)`, which leaves every seam to the chain kernel.  The test asserts the pieces
  planned (`vga_testing_gc_plan_pieces`) and, from the device's counters, the pieces encoded, the seams run and the channels
  the chain kernel walked.

NOT reached here: persistent workgroups on the launcher's own two-size schedule.  It needs 4 x 3584 frames and 128 channel
groups (2048 channels x 200 704 samples), far beyond what a test of seconds can hold to the oracle sample by sample;
`tests/test_gpu_full_size.py` runs it (4096 channels x 60 s against committed digests).

Signals: the synthetic generator, white_full_scale and clipped_square with the oracle's coefficients, the three again with
caller-supplied coefficients on |c0| + |c1| = 32767, and a batch in which exactly ONE channel of a workgroup has coefficients
that can wrap int32, so that a wave whose head keeps the quotient runs beside ordinary ones."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import gc_packed_sum_cases as cases_mod
from vgaudio_amd import signals

pytestmark = pytest.mark.gpu

BATCHES = ("synthetic", "white_full_scale", "clipped_square", "on_bound", "one_hostile")
HOSTILE_CHANNEL = 3
SMALL = (24, 14 * 37 + 5)               # (channels, samples): the tails
PIECES = (72, 14 * 192 + 5)             # three pieces of 65, 65 and 63 frames
NCH, N = SMALL
# (segments hook, persistent hook)
FORMS = {"grid_seams": (3, 1), "persistent_uniform": (3, 2), "persistent_schedule": (0, 2)}
# |c0| + |c1| = 32767 in all four sign quadrants, eight predictors
ON_BOUND_B = np.array([16384, -16383, -16384, -16383, 1, 32766, -1, -32766, 28671, 4096, -28671, 4096, 32767, 0, 0, -32767], np.int16)


def _signal(cls, first_channel, n, nch=1):
    if cls == "synthetic":
        return po.synth_generate(nch, n, first_channel=first_channel)
    return signals.host(cls, nch, n, first_channel=first_channel)


@functools.lru_cache(maxsize=None)
def batch(name, shape=SMALL):
    """pcm [nch, n], coefs [nch, 16], hist1, hist2 [nch] and the oracle's bytes [nch, nbytes]; computed once, read-only"""
    nch, n = shape
    rng = np.random.default_rng(BATCHES.index(name) + 900)
    classes = ("synthetic", "white_full_scale", "clipped_square")
    if name in classes:
        pcm = np.ascontiguousarray(_signal(name, 0, n, nch), np.int16)
    else:
        pcm = np.stack([_signal(classes[c % 3], c, n)[0] for c in range(nch)]).astype(np.int16)
    if name == "on_bound":
        coefs = np.stack([cases_mod.ON_BOUND if c % 2 == 0 else ON_BOUND_B for c in range(nch)])
    else:
        coefs = np.stack([po.gc_calculate_coefficients(pcm[c]) for c in range(nch)]).astype(np.int16)
    if name == "one_hostile":
        coefs[HOSTILE_CHANNEL] = cases_mod.HOSTILE
    h1 = rng.integers(-32768, 32768, nch).astype(np.int16)
    h2 = rng.integers(-32768, 32768, nch).astype(np.int16)
    h1[::4], h2[::4] = 0, 0
    want = np.stack([po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(nch)])
    for a in (pcm, coefs, h1, h2, want):
        a.setflags(write=False)
    return pcm, coefs, h1, h2, want


def _encode(shape, name, layout, segments, persistent, force_open):
    """one encode call under the hooks; returns (bytes, the oracle's bytes, pieces planned, persistent planned, device counters)"""
    import torch
    from vgaudio_amd import _lib, device as vdev
    nch, n = shape
    pcm, coefs, h1, h2, want = batch(name, shape)
    L = _lib.lib()
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(nch, n, d)
    d_pcm[:, :n] = torch.from_numpy(pcm.copy()).to(d)
    d_coefs = torch.from_numpy(coefs.copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1.copy()).to(d), torch.from_numpy(h2.copy()).to(d)
    nb = vdev.gc_byte_count(n)
    assert want.shape[1] == nb
    frames = (n + 13) // 14
    groups = (nch + 15) // 16 if layout == 8 else (nch + 7) // 8         # channel slots per workgroup: 16 or 8
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stats = (C.c_ulonglong * 8)()
    plan = (C.c_int * 5)()
    old_open = 0
    try:
        L.vga_testing_gc_encoder_layout_this_thread(layout)
        L.vga_testing_gc_encoder_segments_this_thread(segments)
        L.vga_testing_gc_encoder_persistent_this_thread(persistent)
        old_open = L.vga_testing_force_open_seams_this_thread(force_open)
        assert L.vga_testing_gc_plan_pieces(cus, groups, frames, C.c_longlong(groups * frames), 0, plan) == 0
        assert L.vga_testing_gc_encode_stats(None, 1) == 0
        out = vdev.gc_encode(d_pcm, n, d_coefs, hist1=d_h1, hist2=d_h2)
        torch.cuda.synchronize()
        assert L.vga_testing_gc_encode_stats(stats, 1) == 0
    finally:
        L.vga_testing_force_open_seams_this_thread(old_open)
        L.vga_testing_gc_encoder_layout_this_thread(0)
        L.vga_testing_gc_encoder_segments_this_thread(0)
        L.vga_testing_gc_encoder_persistent_this_thread(0)
    return out[:, :nb].cpu().numpy(), want, plan[0], plan[4], [int(v) for v in stats], groups


def test_the_batches_are_what_their_names_say():
    wraps = lambda k: (np.abs(k[0::2].astype(int)) + np.abs(k[1::2].astype(int)) > 32767).any()
    for name in BATCHES:
        coefs = batch(name)[1]
        hostile = [c for c in range(NCH) if wraps(coefs[c])]
        assert hostile == ([HOSTILE_CHANNEL] if name == "one_hostile" else []), (name, hostile)
    k = batch("on_bound")[1].astype(int)
    assert (np.abs(k[:, 0::2]) + np.abs(k[:, 1::2]) == 32767).all()


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("layout", [4, 8])
@pytest.mark.parametrize("name", BATCHES)
def test_bytes_match_the_oracle(name, layout, form):
    """the small shape: 38 frames are one piece under every form -- asserted, so that nobody reads more into the names"""
    segments, persistent = FORMS[form]
    got, want, planned, _, stats, groups = _encode(SMALL, name, layout, segments, persistent, 0)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist())
    assert planned == 1
    assert stats[6] == groups, stats              # one piece per channel group encoded ...
    assert stats[0] == 0 and stats[1] == 0 and stats[2] == 0 and stats[5] == 0, stats     # ... and no seam, no chain


# (segments hook, persistent hook, layout): the plain grid with its seam and chain launches in both layouts (eight- and
# sixteen-lane seam runs), persistent workgroups that close the seams themselves
PIECE_FORMS = {"grid_seams_layout4": (3, 1, 4), "grid_seams_layout8": (3, 1, 8), "persistent_uniform": (3, 2, 8)}


@pytest.mark.parametrize("force_open", [0, 1], ids=["seams_as_they_fall", "every_seam_left_open"])
@pytest.mark.parametrize("form", sorted(PIECE_FORMS))
@pytest.mark.parametrize("name", BATCHES)
def test_three_pieces_with_seam_and_chain_runs_match_the_oracle(name, form, force_open):
    segments, persistent, layout = PIECE_FORMS[form]
    nch = PIECES[0]
    got, want, planned, planned_persistent, stats, groups = _encode(PIECES, name, layout, segments, persistent, force_open)
    bad = np.argwhere(got != want)
    assert bad.size == 0, ("first differing (channel, byte)", bad[0].tolist(), stats)
    assert planned == 3
    if layout == 8:                                # (the plan is asked for the product's layout; layout 4 never runs persistent)
        assert planned_persistent == (1 if persistent == 2 else 0)
    assert 3 * groups <= stats[6] <= 4 * groups, stats     # every (channel group, piece) item encoded (+ a repair pass at most)
    assert stats[0] + stats[1] == 2 * nch, stats   # a seam run per channel and seam
    if force_open:
        assert stats[0] == 0 and stats[1] == 2 * nch and stats[5] > 0, stats      # none accepted: the chain kernel walks them
    assert stats[2] > 0, stats                     # frames re-encoded from the true history


@pytest.mark.parametrize("name", ["synthetic", "white_full_scale", "clipped_square"])
def test_coefficients_match_the_oracle(name):
    import torch
    from vgaudio_amd import device as vdev
    pcm, coefs, _, _, _ = batch(name)
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(NCH, N, d)
    d_pcm[:, :N] = torch.from_numpy(pcm.copy()).to(d)
    got = vdev.gc_coefs(d_pcm, N)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().reshape(NCH, 16), coefs)


@pytest.mark.parametrize("persistent", [1, 2])
@pytest.mark.parametrize("name", BATCHES)
def test_ragged_batch_of_four_lengths(name, persistent):
    """the `_v` entry point: lengths 5 (less than a frame), 14 (one frame), 15 (a frame and one sample) and 523 in one call"""
    from vgaudio_amd import _lib
    pcm, coefs, h1, h2, _ = batch(name)
    L = _lib.lib()
    lens = [(N, 5, 14, 15)[c % 4] for c in range(NCH)]
    lens[HOSTILE_CHANNEL] = N                       # the hostile channel at full length
    chans = [np.ascontiguousarray(pcm[c, :n]) for c, n in enumerate(lens)]
    counts = np.array(lens, dtype=np.int32)
    given = np.ascontiguousarray(coefs)
    a1, a2 = np.ascontiguousarray(h1), np.ascontiguousarray(h2)
    outs = [np.full(L.vga_gcadpcm_sample_count_to_byte_count(n) + 1, 0xEE, dtype=np.uint8) for n in lens]
    ptrs = lambda t, arrays: (t * len(arrays))(*[a.ctypes.data_as(t) for a in arrays])
    try:
        L.vga_testing_gc_encoder_persistent_this_thread(persistent)
        _lib.check(L.vga_gcadpcm_encode_with_coefs_batch_v(ptrs(_lib.i16p, chans), counts.ctypes.data_as(C.POINTER(C.c_int)), NCH,
                                                           given.ctypes.data_as(_lib.i16p), a1.ctypes.data_as(_lib.i16p),
                                                           a2.ctypes.data_as(_lib.i16p), ptrs(_lib.u8p, outs)))
    finally:
        L.vga_testing_gc_encoder_persistent_this_thread(0)
    for c, n in enumerate(lens):
        assert outs[c][-1] == 0xEE, "wrote past the end of a row"
        want = po.gc_encode(chans[c], given[c], hist1=int(a1[c]), hist2=int(a2[c]))
        assert np.array_equal(outs[c][:-1], want), (c, n)
