"""Seeded GC-ADPCM encode cases for the error sum in packed pairs (gc_encode_core.hpp E1-E5): channels whose final lanes carry
errors that do not fit int16, channels whose best error sum is 2^28 or more (64-bit keys decide, the exact-sum rule of the
encoder's cold block runs), next to ordinary ones.  Shared by tests/test_host_gc_packed_sum.py and
tests/test_gpu_gc_packed_sum.py; the oracle's bytes are computed once per process.

How the seeds were found (CPU, tests/host/gc_packed_sum_driver.cpp's emulator next to the oracle, 40 channels of each
generator, 301 frames each, histories (0, 0) and (-32768, 32767)):
  * clipped_square with the oracle's own coefficients: 120-130 final lanes per channel with |e| >= 32768, never a best sum
    of 2^28 or more;  white_full_scale with the oracle's coefficients: neither;
  * caller-supplied coefficients ON the bound |c0| + |c1| = 32767 (ON_BOUND) and large ones below it (WILD; both pass
    coef_ok): white_full_scale -- every frame's best sum is >= 2^28, 270-1100 lanes through the wide pass, and in 90-280 of 301
    frames the packed sums taken as they are would have picked another predictor; clipped_square -- 180-280 such frames.
"""
import functools

import numpy as np

from oracle import pyoracle as po
from vgaudio_amd import signals

N = 14 * 600 + 5                        # 601 frames, the last one partial; three pieces of 200 frames under the segments hook
NCH = 70                                # four full workgroups of 16 channel slots and one with 6 (dead slots)
ON_BOUND = np.array([32767, 0, 0, 32767, -32767, 0, 0, -32767, 16384, 16383, -16384, 16383, -16383, -16384, 4096, -28671], np.int16)
WILD = np.array([30000, -2767, -30000, 2767, 20000, 12767, -20000, -12767, 32767, 0, 28000, -4767, -28000, 4767, 16384, -16383], np.int16)
# coefficients that can wrap int32 in some predictors, next to ordinary ones: those lanes walk the reference's loop as written
HOSTILE = np.array([-32768, -32768, 32767, 32767, -32768, 32767, 3900, -1900, 4095, -2047, -2048, 0, 20000, 20000, 0, 0], np.int16)
# (generator, coefficients or None = the oracle's own, (hist1, hist2))
KINDS = [("white_full_scale", ON_BOUND, (0, 0)),              # best sum >= 2^28 in every frame
         ("clipped_square", None, (0, 0)),                    # final lanes with |e| >= 32768
         ("clipped_square", WILD, (-32768, 32767)),           # both
         ("sine440", None, (0, 0)),                           # ordinary
         ("white_full_scale", WILD, (32767, -32768)),
         ("synthetic", None, (123, -456)),                    # ordinary
         ("clipped_square", ON_BOUND, (0, 0)),
         ("white_full_scale", HOSTILE, (-32768, -32768)),
         ("white_full_scale", None, (0, 0))]


@functools.lru_cache(maxsize=None)
def cases():
    """pcm [NCH, N], coefs [NCH, 16], hist1, hist2 [NCH], the oracle's bytes [NCH, nbytes] and the two samples its decoder
    ends on [NCH, 2]"""
    pcm = np.empty((NCH, N), np.int16)
    coefs = np.empty((NCH, 16), np.int16)
    h1 = np.empty(NCH, np.int16)
    h2 = np.empty(NCH, np.int16)
    for c in range(NCH):
        gen, cs, (a, b) = KINDS[c % len(KINDS)]
        pcm[c] = po.synth_generate(1, N, first_channel=c)[0] if gen == "synthetic" else signals.host(gen, 1, N, first_channel=c)[0]
        coefs[c] = po.gc_calculate_coefficients(pcm[c]) if cs is None else cs
        h1[c], h2[c] = a, b
    want = np.stack([po.gc_encode(pcm[c], coefs[c], hist1=int(h1[c]), hist2=int(h2[c])) for c in range(NCH)])
    end = np.stack([po.gc_decode(want[c], coefs[c], N, hist1=int(h1[c]), hist2=int(h2[c]))[-2:] for c in range(NCH)])
    for a in (pcm, coefs, h1, h2, want, end):
        a.setflags(write=False)
    return pcm, coefs, h1, h2, want, end
