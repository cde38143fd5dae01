#!/usr/bin/env python3
"""How much wave-time does the GC-ADPCM encode launch leave idle at its end?  Needs a -DVGA_DEBUG_TIMESTAMPS build (see
tools/time_wave_ends.py).  Per workgroup (one wave of the self-served shape) the start and the end; printed: the
distribution of the ends, the idle wave-time between each wave's end and the launch's end as a fraction of the launch, and
a histogram of the ends over the last milliseconds.
    VGAUDIO_HIP_LIBRARY=tools/variants/libvga_ts.so python tools/time_wave_idle.py [--channels 4096] [--seconds 60]
        [--signal sine440] [--schedule big,n1,n2,n3,s1,s2,s3,floor]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--signal", default="")
    ap.add_argument("--schedule", default="", help="vga_testing_gc_schedule_this_thread: big rounds, three counts, three sizes, floor")
    ap.add_argument("--launches", type=int, default=3)
    a = ap.parse_args()
    import torch
    from vgaudio_amd import _lib, device as vdev
    raw = C.CDLL(_lib.SO_PATH)
    dev = torch.device("cuda:0")
    n = int(a.seconds * 48000)
    nch = a.channels
    if a.signal:
        from vgaudio_amd import signals
        pcm = signals.device(a.signal, nch, n, dev)
    else:
        pcm = vdev.synth_pcm(nch, n, dev)
    coefs = vdev.gc_coefs(pcm, n)
    out = vdev.alloc_adpcm(nch, n, dev)
    if a.schedule:
        v = [int(x) for x in a.schedule.split(",")]
        raw.vga_testing_gc_schedule_this_thread(v[0], (C.c_int * 3)(*v[1:4]), (C.c_int * 3)(*v[4:7]), v[7])
    for _ in range(a.launches):
        vdev.gc_encode(pcm, n, coefs, out=out)
    torch.cuda.synchronize()
    ts = np.zeros(1 << 16, dtype=np.uint64)
    raw.vga_debug_encode_timestamps(ts.ctypes.data_as(C.c_void_p), ts.size)
    t = ts.reshape(-1, 2).astype(np.float64) / 1e5                                # 100 MHz ticks -> ms
    t = t[t[:, 1] > 0]
    t0 = t[:, 0].min()
    end = t[:, 1] - t0
    launch = float(end.max())
    q = np.percentile(end, [0, 50, 95, 100])
    idle = float((launch - end).mean())
    print(json.dumps({"library": os.path.basename(_lib.SO_PATH), "channels": nch, "signal": a.signal or "synthetic", "schedule": a.schedule or "default",
                      "waves": int(t.shape[0]), "launch_ms": round(launch, 3),
                      "end_ms": {"min": round(float(q[0]), 3), "p50": round(float(q[1]), 3), "p95": round(float(q[2]), 3), "max": round(float(q[3]), 3)},
                      "start_spread_ms": round(float((t[:, 0] - t0).max()), 3),
                      "idle_wave_ms_mean": round(idle, 3), "idle_fraction_of_launch": round(idle / launch, 5)}))
    edges = launch - np.arange(16, -1, -1, dtype=np.float64)                        # one-millisecond bins over the last 16 ms
    hist, _ = np.histogram(end, bins=edges)
    print(json.dumps({"ends_before_last_16_ms": int((end < edges[0]).sum()),
                      "ends_per_ms_before_launch_end": {f"-{16 - i}..-{15 - i}": int(h) for i, h in enumerate(hist)}}))


if __name__ == "__main__":
    main()
