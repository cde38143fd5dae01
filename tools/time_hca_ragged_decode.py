#!/usr/bin/env python3
"""Wall time of vga_hca_decode_batch_v on a folder's worth of HCA streams of different lengths.

    python tools/time_hca_ragged_decode.py [--streams 2048] [--min-seconds 1] [--max-seconds 60] [--quality 2] [--seed 1]
    VGAUDIO_HIP_LIBRARY=/path/to/another/libvgaudio_hip.so python tools/time_hca_ragged_decode.py     # another build, same script

Encodes N mono and stereo streams of log-uniform lengths (48 kHz, one quality) with vga_hca_encode_batch_v, then times
vga_hca_decode_batch_v on them: 3 warm-up and 10 timed calls, wall clock around the call.  For scale the same streams, padded
to the longest of their channel count, go through vga_hca_decode_batch (equal lengths: the kernels' plain path).  Prints one
JSON line; "stats" are the counters of vga_testing_hca_decode_v_stats (jobs, chunks, classes, own frames, frame slots) or
null when the library under test has no such hook.  The library is loaded here with the handful of signatures the script
needs, so that a build from before the hook loads too."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib, synth  # noqa: E402


def load():
    _lib._preload_torch_hip_runtime()
    L = C.CDLL(_lib.SO_PATH)
    for name in ("vga_hca_encoder_initialize", "vga_hca_encode_batch_v", "vga_hca_decode_batch_v", "vga_hca_decode_batch", "vga_last_error"):
        f = getattr(L, name)
        f.restype, f.argtypes = _lib.SIGNATURES[name]
    return L


def ptrs(t, arrays):
    return (t * len(arrays))(*[a.ctypes.data_as(t) for a in arrays])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--max-seconds", type=float, default=60.0)
    ap.add_argument("--quality", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    L = load()

    def check(rc):
        if rc:
            raise SystemExit("error %d: %s" % (rc, L.vga_last_error().decode()))

    rng = np.random.default_rng(a.seed)
    ns = a.streams
    lens = np.exp(rng.uniform(np.log(a.min_seconds * 48000), np.log(a.max_seconds * 48000), ns)).astype(np.int64)
    nchs = [1 + (s & 1) for s in range(ns)]
    cps = (_lib.HcaParamsC * ns)(*[_lib.HcaParamsC(a.quality, 0, 0, nchs[s], 48000, int(lens[s]), 0, 0, 0) for s in range(ns)])
    infos = (_lib.HcaInfoC * ns)()
    for s in range(ns):
        check(L.vga_hca_encoder_initialize(C.byref(cps[s]), C.byref(infos[s])))
    # every channel is a window of one long synthetic signal
    base = synth.generate(2, int(lens.max()))
    rows = [base[c][:int(lens[s])] for s in range(ns) for c in range(nchs[s])]
    frames = [np.zeros(infos[s].frame_count * infos[s].frame_size, np.uint8) for s in range(ns)]
    check(L.vga_hca_encode_batch_v(ptrs(_lib.i16p, rows), ns, cps, infos, ptrs(_lib.u8p, frames)))
    outs = [np.zeros(int(lens[s]), np.int16) for s in range(ns) for _ in range(nchs[s])]
    fp, op = ptrs(_lib.u8p, frames), ptrs(_lib.i16p, outs)

    def timed(call):
        for _ in range(a.warmup):
            check(call())
        t = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            rc = call()
            t.append((time.perf_counter() - t0) * 1e3)
            check(rc)
        return t

    ragged = timed(lambda: L.vga_hca_decode_batch_v(infos, fp, ns, op))
    stats = None
    if hasattr(L, "vga_testing_hca_decode_v_stats"):
        out = (C.c_longlong * 5)()
        L.vga_testing_hca_decode_v_stats.restype, L.vga_testing_hca_decode_v_stats.argtypes = C.c_int, [C.POINTER(C.c_longlong), C.c_int]
        L.vga_testing_hca_decode_v_stats(out, 5)
        stats = dict(zip(("jobs", "chunks", "classes", "own_frames", "frame_slots"), [int(v) for v in out]))
    checksum = int(sum(int(o[::97].astype(np.int64).sum()) for o in outs))

    # for scale: the same streams padded to the longest of their channel count, one equal-length call per channel count
    padded = []
    for nch in (1, 2):
        idx = [s for s in range(ns) if nchs[s] == nch]
        if not idx:
            continue
        top = max(idx, key=lambda s: infos[s].frame_count)
        h = _lib.HcaInfoC.from_buffer_copy(infos[top])
        fb = h.frame_count * h.frame_size
        fr = []
        for s in idx:
            # a shorter stream's frames, then repeats of its last frame up to the longest (valid frames: sync word and all)
            own = frames[s].reshape(infos[s].frame_count, h.frame_size)
            pad = np.repeat(own[-1:], h.frame_count - infos[s].frame_count, axis=0)
            fr.append(np.ascontiguousarray(np.concatenate([own, pad]).reshape(-1)))
            assert fr[-1].size == fb
        po = [np.zeros(h.sample_count, np.int16) for _ in range(len(idx) * nch)]
        padded.append((h, ptrs(_lib.u8p, fr), len(idx), ptrs(_lib.i16p, po), fr, po))

    def equal_call():
        for h, f, n, o, _, _ in padded:
            rc = L.vga_hca_decode_batch(C.byref(h), f, n, o)
            if rc:
                return rc
        return 0

    equal = timed(equal_call)
    own_frames = int(sum(infos[s].frame_count for s in range(ns)))
    print(json.dumps({
        "tool": "time_hca_ragged_decode", "library": os.path.basename(os.path.dirname(_lib.SO_PATH)) + "/" + os.path.basename(_lib.SO_PATH),
        "streams": ns, "seconds": [a.min_seconds, a.max_seconds], "quality": a.quality, "seed": a.seed,
        "own_frames": own_frames, "pcm_mb": round(sum(o.nbytes for o in outs) / 1e6, 1),
        "ragged_ms": {"median": round(float(np.median(ragged)), 2), "min": round(min(ragged), 2), "max": round(max(ragged), 2)},
        "equal_length_padded_ms": {"median": round(float(np.median(equal)), 2), "min": round(min(equal), 2), "max": round(max(equal), 2),
                                   "frames": int(sum(h.frame_count * n for h, _, n, _, _, _ in padded))},
        "stats": stats, "checksum": checksum}))


if __name__ == "__main__":
    main()
