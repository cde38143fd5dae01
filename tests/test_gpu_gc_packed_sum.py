"""GC-ADPCM encoder on the GPU with the error sum in packed pairs and the cold block's exact-sum rule (gc_encode_core.hpp
E1-E5, round 8) against the oracle, byte for byte: the seeded channels of tests/gc_packed_sum_cases.py (errors that do not fit
int16, best sums of 2^28 and more, hostile coefficients) next to ordinary ones.  1, 9 and 70 channels; 601 frames, the last one
partial, as one piece and as three; both lane layouts; the plain grid and the persistent kernel; a ragged batch; and the lot
again on poisoned allocations."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import gc_packed_sum_cases as cases_mod

pytestmark = pytest.mark.gpu

N = cases_mod.N


@pytest.fixture(params=[-1, 0xA5], ids=["clean", "poisoned"])
def poison(request):
    from vgaudio_amd import _lib
    L = _lib.lib()
    old = L.vga_testing_poison_allocations(request.param) if request.param >= 0 else L.vga_testing_poison_allocations(-1)
    yield request.param
    L.vga_testing_poison_allocations(-1)
    assert old == -1


@pytest.mark.parametrize("layout", [4, 8])
@pytest.mark.parametrize("nch", [1, 9, cases_mod.NCH])
def test_bytes_and_end_history_match_the_oracle(nch, layout, poison):
    import torch
    from vgaudio_amd import _lib, device as vdev
    pcm, coefs, h1, h2, want, end = cases_mod.cases()
    L = _lib.lib()
    d = torch.device("cuda:0")
    d_pcm = vdev.alloc_pcm(nch, N, d)
    d_pcm[:, :N] = torch.from_numpy(pcm[:nch].copy()).to(d)
    d_coefs = torch.from_numpy(coefs[:nch].copy()).to(d)
    d_h1, d_h2 = torch.from_numpy(h1[:nch].copy()).to(d), torch.from_numpy(h2[:nch].copy()).to(d)
    nb = vdev.gc_byte_count(N)
    assert want.shape[1] == nb
    try:
        L.vga_testing_gc_encoder_layout_this_thread(layout)
        for pieces in (1, 3):
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


@pytest.mark.parametrize("persistent", [1, 2])
def test_ragged_batch_of_three_lengths(persistent, poison):
    """18 seeded channels at three lengths (601, 201 and 38 frames, each with a partial last frame) in one call, coefficients
    given, three pieces for the longest"""
    from vgaudio_amd import _lib
    pcm, coefs, h1, h2, _, _ = cases_mod.cases()
    L = _lib.lib()
    lens = [(N, 14 * 200 + 5, 14 * 37 + 5)[c % 3] for c in range(18)]
    chans = [np.ascontiguousarray(pcm[c, :n]) for c, n in enumerate(lens)]
    counts = np.array(lens, dtype=np.int32)
    given = np.ascontiguousarray(coefs[:18])
    a1, a2 = np.ascontiguousarray(h1[:18]), np.ascontiguousarray(h2[:18])
    outs = [np.full(L.vga_gcadpcm_sample_count_to_byte_count(n) + 1, 0xEE, dtype=np.uint8) for n in lens]
    ptrs = lambda t, arrays: (t * len(arrays))(*[a.ctypes.data_as(t) for a in arrays])
    try:
        L.vga_testing_gc_encoder_segments_this_thread(3)
        L.vga_testing_gc_encoder_persistent_this_thread(persistent)
        _lib.check(L.vga_gcadpcm_encode_with_coefs_batch_v(ptrs(_lib.i16p, chans), counts.ctypes.data_as(C.POINTER(C.c_int)), 18,
                                                           given.ctypes.data_as(_lib.i16p), a1.ctypes.data_as(_lib.i16p),
                                                           a2.ctypes.data_as(_lib.i16p), ptrs(_lib.u8p, outs)))
    finally:
        L.vga_testing_gc_encoder_segments_this_thread(0)
        L.vga_testing_gc_encoder_persistent_this_thread(0)
    for c, n in enumerate(lens):
        assert outs[c][-1] == 0xEE, "wrote past the end of a row"
        want = po.gc_encode(chans[c], given[c], hist1=int(a1[c]), hist2=int(a2[c]))
        assert np.array_equal(outs[c][:-1], want), (c, n)
