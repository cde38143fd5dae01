#!/usr/bin/env python3
"""One GC-ADPCM encode call, timed: the mean of --launches launches (events around each), in a process of its own, under a
schedule forced through vga_testing_gc_schedule_this_thread (round 16: the descending tail of the self-served shape).
    python tools/time_encode_tail.py [--channels 4096] [--seconds 60] [--signal sine440]
        [--schedule big,n1,n2,n3,s1,s2,s3,floor] [--checksum] [--stats]
--checksum: two position-weighted sums over the output bytes (the same bytes whatever the schedule).
--stats: vga_testing_gc_encode_stats_n of the last launch.  A library without the hook (a parent build) runs its own schedule."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--signal", default="")
    ap.add_argument("--schedule", default="")
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--checksum", action="store_true")
    ap.add_argument("--stats", action="store_true")
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
    for _ in range(2):
        vdev.gc_encode(pcm, n, coefs, out=out)
    torch.cuda.synchronize()
    ms = []
    for i in range(a.launches):
        if a.stats and i == a.launches - 1:
            raw.vga_testing_gc_encode_stats_n((C.c_ulonglong * 9)(), 9, 1)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        vdev.gc_encode(pcm, n, coefs, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    r = {"library": os.path.basename(_lib.SO_PATH), "channels": nch, "signal": a.signal or "synthetic", "schedule": a.schedule or "default",
         "launches": a.launches, "encode_ms_mean": round(sum(ms) / len(ms), 3), "encode_ms_min": round(min(ms), 3), "encode_ms_max": round(max(ms), 3)}
    if a.stats:
        st = (C.c_ulonglong * 9)()
        raw.vga_testing_gc_encode_stats_n(st, 9, 0)
        r["stats"] = [int(x) for x in st]
    if a.checksum:
        b = out.view(torch.uint8).reshape(nch, -1)
        w = (torch.arange(b.shape[1], device=dev, dtype=torch.int64) % 65521) + 1
        s0 = s1 = 0
        for lo in range(0, nch, 64):
            x = b[lo:lo + 64].to(torch.int64)
            s0 += int(x.sum())
            s1 += int(((x * w).sum(dim=1) * (torch.arange(lo, lo + x.shape[0], device=dev, dtype=torch.int64) + 1)).sum())
        r["checksum"] = [s0, s1 % (1 << 61)]
    print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
