#!/usr/bin/env python3
"""Round 15, gate 0 (CPU, oracle only): can the channels whose encoder seams close slowly be told from their coefficients?

For every channel: how many frames a seam needs to close -- a host model of the two runs: the oracle's encode of the whole
stream (the true run) next to its encode from the seam on, started from the two input samples before it (the guessed run);
closed = both decoded histories coincide at a frame end -- next to the largest pole radius among the channel's eight
predictors (complex poles: r^2 = -c1 / 2048; real poles: the larger root's square).

    python tools/gc_slow_seam_table.py [frames] > profiles/r15_gate0_slow_seams.log
"""
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import pyoracle as po                      # noqa: E402
from vgaudio_amd import signals, synth                 # noqa: E402

FRAMES = int(sys.argv[1]) if len(sys.argv) > 1 else 10240
SEAMS = tuple(FRAMES * k // 16 for k in (1, 3, 5, 9, 13))   # frames the model's seams start at
SLOW = 1024


def closing_frames(pcm, coefs, true_dec, f0):
    s = f0 * 14
    h1, h2 = int(pcm[s - 1]), int(pcm[s - 2])
    guess = po.gc_encode(pcm[s:], coefs, hist1=h1, hist2=h2)
    dec = po.gc_decode(guess, coefs, len(pcm) - s, hist1=h1, hist2=h2)
    frames = (len(pcm) - s) // 14
    a = true_dec[s:s + frames * 14].reshape(frames, 14)[:, 12:]
    b = dec[:frames * 14].reshape(frames, 14)[:, 12:]
    same = np.flatnonzero((a == b).all(axis=1))
    return int(same[0]) + 1 if same.size else frames + 1   # (frames + 1: never inside the stream)


def radius2(coefs):
    """largest squared pole radius over the eight predictors, and the largest -c1 among those with complex poles"""
    best, best_c1 = 0.0, 0
    for p in range(8):
        a, b = coefs[2 * p] / 2048.0, coefs[2 * p + 1] / 2048.0     # z^2 = a z + b
        disc = a * a + 4.0 * b
        if disc < 0:
            r2 = -b
            best_c1 = max(best_c1, -int(coefs[2 * p + 1]))
        else:
            r2 = max(abs(a + disc ** 0.5), abs(a - disc ** 0.5)) ** 2 / 4.0
        best = max(best, r2)
    return best, best_c1


def one_channel(pcm):
    coefs = po.gc_calculate_coefficients(pcm)
    dec = po.gc_decode(po.gc_encode(pcm, coefs), coefs, len(pcm))
    return ([closing_frames(pcm, coefs, dec, f0) for f0 in SEAMS],) + radius2(coefs)


def main():
    n = FRAMES * 14
    rows = [("synth", c, synth.generate(1, n, first_channel=c)[0]) for c in range(128)]
    for cls in signals.CLASSES:
        rows += [(cls, c, signals.host(cls, 1, n, first_channel=c)[0]) for c in range(16)]
    rows += [("tones_in_noise", c, signals.tones_in_noise(1, n, first_channel=c)[0]) for c in range(16)]   # (the seam tests' signals)
    print("# %d frames per channel, model seams at frames %s; slow = more than %d frames" % (FRAMES, list(SEAMS), SLOW))
    print("%-18s %4s %s %8s %8s" % ("set", "ch", " ".join("%8s" % ("@%d" % f) for f in SEAMS), "max r^2", "max -c1"))
    table = []
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        for (name, c, _), (close, r2, c1) in zip(rows, pool.imap(one_channel, [r[2] for r in rows])):
            table.append((name, c, max(close), r2, c1))
            print("%-18s %4d %s %8.4f %8d" % (name, c, " ".join("%8d" % f for f in close), r2, c1), flush=True)
    for what, part in (("gate set (synthetic 0-127, 16 per signal class)", [t for t in table if t[0] != "tones_in_noise"]),
                       ("tones_in_noise (outside the gate set)", [t for t in table if t[0] == "tones_in_noise"])):
        slow = [t for t in part if t[2] > SLOW]
        fast = [t for t in part if t[2] <= SLOW]
        print("# %s: %d slow channels of %d" % (what, len(slow), len(part)))
        if slow:
            lo = min(t[4] for t in slow)
            print("#   smallest max -c1 among the slow channels: %d (r^2 = %.4f)" % (lo, lo / 2048.0))
            print("#   fast channels at or above it (false positives): %d" % sum(1 for t in fast if t[4] >= lo))
        print("#   largest max -c1 among the fast channels: %d" % max(t[4] for t in fast))


if __name__ == "__main__":
    main()
