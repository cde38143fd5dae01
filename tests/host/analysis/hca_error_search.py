"""Analysis, not a test: which inputs make CriHcaEncoder.EncodeFrame throw -- "Bitrate is set too low." (CriHcaEncoder.cs:471,
the oracle's -3) and the NotImplementedException of CalculateEvaluationBoundary (:499, the oracle's -4).  The lowest bitrates
CriHcaEncoder.Initialize accepts, crossed with silence, full-scale noise, impulse trains and alternating full scale for 1-8
channels at three sample rates; the oracle's path counters (po.hca_encode_paths) say what each encode did.  10920 encodes
of three frames each, a few seconds.  tests/hca_encoder_path_cases.py (ERROR_CASES) holds what it found.
    python tests/host/analysis/hca_error_search.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "..", ".."), os.path.join(HERE, "..", "..")]
import hca_encoder_path_cases as pc  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

n = 3000
bitrates = list(range(1, 200, 7)) + list(range(200, 4000, 100)) + list(range(4000, 16000, 500))
outcome = {}          # (rc, signal) -> [(rate, channels, bitrate, frame size, coded bands, band drops)]
refused_by_initialize = 0
for rate in (48000, 44100, 8000):
    for nch in range(1, 9):
        signals = {"silence": np.zeros((nch, n), np.int16), "noise": pc.noise(nch, n, nch), "impulse4": pc.impulse_train(nch, n, 4),
                   "impulse64": pc.impulse_train(nch, n, 64), "alternating": pc.alternating(nch, n)}
        for bitrate in bitrates:
            p = po.hca_params(nch, n, sample_rate=rate, quality="Lowest", bitrate=bitrate)
            rc, info = po.hca_init(p)
            if rc:
                refused_by_initialize += 1
                continue
            for name, x in signals.items():
                rc, info, _ = po.hca_encode(x, p)
                c = po.hca_encode_paths()
                assert (rc == -3) == (c["error_minus3"] > 0) and (rc == -4) == (c["error_minus4"] > 0)
                outcome.setdefault((rc, name), []).append((rate, nch, bitrate, info.frame_size, info.base_band_count + info.stereo_band_count,
                                                           c["band_drops"]))
print("parameter sets Initialize refused:", refused_by_initialize)
for (rc, name), rows in sorted(outcome.items()):
    top = max(rows, key=lambda r: r[2])
    after_drops = sum(1 for r in rows if r[5] > 0)
    print("rc %2d %-11s %5d encodes; highest bitrate %6d (%d Hz, %d channels, %d-byte frames, %d coded bands); %d after dropping bands"
          % (rc, name, len(rows), top[2], top[0], top[1], top[3], top[4], after_drops))
print("-4 reached:", sum(len(rows) for (rc, _), rows in outcome.items() if rc == -4), "times")
