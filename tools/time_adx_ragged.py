#!/usr/bin/env python3
"""GPU time of the packed ADX calls (vga_adx_encode_device_v / vga_adx_decode_device_v) on the file set of bench.py's ragged
block: 10 008 files of 1-120 s at 48 kHz (seed 0xBA7C4, log-uniform, as many as hold 4096 x 60 s), PCM generated on the device
by vga_synth_pcm16_device.

    python tools/time_adx_ragged.py [--calls 10] [--warmup 2] [--files N] [--subset 1000]

Device events around the calls on one stream, medians (and the spread) of --calls repeats after --warmup, one process.  Per
direction:
  packed    one *_device_v call on the packed buffers (the whole set, and the subset below when it is used);
  per_file  what a caller with device-resident files had before: one vga_adx_encode_device / vga_adx_decode_device call per
            file on the same packed buffers.  The whole set if all its repeats finish inside a minute (estimated from the
            first 100 files), else a seeded --subset of the files -- then `packed` is timed on that subset as well;
  equal     one vga_adx_*_device call on as many channels of equal length with the same total number of samples
            (BASELINE configs[2]'s shape): the rate ceiling.
One JSON line per (direction, form, set)."""
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
from vgaudio_amd.criadx import RaggedAdx  # noqa: E402


def bench_lengths():
    rng = np.random.default_rng(0xBA7C4)
    lens, total = [], 0
    while total < 4096 * 2_880_000:
        lens.append(int(np.exp(rng.uniform(np.log(48000.0), np.log(120 * 48000.0)))))
        total += lens[-1]
    return lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=0, help="only the first N files of the set (0 = all)")
    ap.add_argument("--subset", type=int, default=1000, help="files of the seeded subset the per-file route falls back to")
    a = ap.parse_args()
    assert a.calls >= 10 or a.files, "at least 10 repetitions"
    import torch
    L = _lib.lib()
    check = _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    nch = len(lens)
    p = _lib.AdxParams()
    L.vga_adx_default_params(C.byref(p))
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def timed(call):
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    def line(direction, form, which, t, samples, files):
        print(json.dumps({"tool": "time_adx_ragged", "set": which, "files": files, "direction": direction, "form": form,
                          "samples": int(samples), **t, "msamples_per_s": round(samples / t["median_ms"] / 1e3, 1)}), flush=True)

    class Set:
        """a ragged object over `lens`, its packed buffers, PCM generated in place"""

        def __init__(self, lens, first_channel=0):
            self.lens = lens
            self.r = RaggedAdx(p, lens)
            t = self.r.totals
            self.pcm = torch.zeros(t.pcm_samples, dtype=torch.int16, device=dev)
            self.adx = torch.zeros(t.adx_bytes, dtype=torch.uint8, device=dev)
            self.out = torch.zeros(t.pcm_samples, dtype=torch.int16, device=dev)
            self.ws = torch.empty(max(t.encode_workspace_bytes, t.decode_workspace_bytes, 16), dtype=torch.uint8, device=dev)
            self.status = torch.zeros(len(lens), dtype=torch.int32, device=dev)
            params = torch.from_numpy(np.array([synth.channel_params(first_channel + c) for c in range(len(lens))],
                                               dtype=np.uint32).reshape(len(lens), 4).view(np.int32)).to(dev)
            for c, n in enumerate(lens):                               # one launch per file: set-up, not the timed path
                check(L.vga_synth_pcm16_device(self.pcm.data_ptr() + 2 * int(self.r.pcm_offsets[c]), max(n, 8), 1, n, first_channel + c,
                                               params[c].data_ptr(), S))
            torch.cuda.synchronize()
            self.nbytes = [L.vga_adx_encoded_byte_count(n, C.byref(p)) for n in lens]

        def packed(self, direction):
            if direction == "encode":
                self.r.encode_device(self.pcm, self.adx, self.ws)
            else:
                self.r.decode_device(self.adx, self.out, self.ws, self.status)

        def per_file(self, direction, count=None):
            po, ao = self.r.pcm_offsets, self.r.adx_offsets
            for c in range(count if count is not None else len(self.lens)):
                n, nb = self.lens[c], self.nbytes[c]
                if direction == "encode":
                    check(L.vga_adx_encode_device(self.pcm.data_ptr() + 2 * int(po[c]), (n + 7) // 8 * 8, 1, n, C.byref(p),
                                                  self.adx.data_ptr() + int(ao[c]), (nb + 15) // 16 * 16, None, S))
                else:
                    check(L.vga_adx_decode_device(self.adx.data_ptr() + int(ao[c]), (nb + 15) // 16 * 16, nb, 1, n, C.byref(p),
                                                  self.out.data_ptr() + 2 * int(po[c]), (n + 7) // 8 * 8, self.status.data_ptr(), S))

    whole = Set(lens)
    total = sum(lens)
    print(json.dumps({"tool": "time_adx_ragged", "files": nch, "samples": total, "encode_workspace_bytes": whole.r.totals.encode_workspace_bytes,
                      "decode_workspace_bytes": whole.r.totals.decode_workspace_bytes}), flush=True)
    # will the per-file route over the whole set fit into a minute?  (first 100 files, scaled by samples)
    probe = min(100, nch)
    whole.per_file("encode", probe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    whole.per_file("encode", probe)
    whole.per_file("decode", probe)
    torch.cuda.synchronize()
    estimate = (time.perf_counter() - t0) * total / sum(lens[:probe]) * (a.calls + a.warmup)
    sub = None
    if estimate > 60.0 and nch > a.subset:
        pick = sorted(np.random.default_rng(0x5B5E7).choice(nch, a.subset, replace=False).tolist())
        sub = Set([lens[i] for i in pick], first_channel=nch)
    print(json.dumps({"tool": "time_adx_ragged", "per_file_estimate_s": round(estimate, 1), "per_file_set": "subset" if sub else "whole"}), flush=True)

    # the equal-length call at the same total sample count
    eq_n = total // nch // 32 * 32
    eq_pitch, eq_bytes = eq_n, L.vga_adx_encoded_byte_count(eq_n, C.byref(p))
    eq_out_pitch = (eq_bytes + 15) // 16 * 16
    eq_adx = torch.zeros(nch * eq_out_pitch, dtype=torch.uint8, device=dev)
    eq_status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert whole.pcm.numel() >= nch * eq_pitch

    def equal(direction):
        if direction == "encode":
            check(L.vga_adx_encode_device(whole.pcm.data_ptr(), eq_pitch, nch, eq_n, C.byref(p), eq_adx.data_ptr(), eq_out_pitch, None, S))
        else:
            check(L.vga_adx_decode_device(eq_adx.data_ptr(), eq_out_pitch, eq_bytes, nch, eq_n, C.byref(p), whole.out.data_ptr(), eq_pitch,
                                          eq_status.data_ptr(), S))

    for direction in ("encode", "decode"):                             # (the decoders read what the encoders wrote)
        line(direction, "packed", "whole", timed(lambda: whole.packed(direction)), total, nch)
        line(direction, "equal", "whole", timed(lambda: equal(direction)), eq_n * nch, nch)
        s = sub or whole
        if sub:
            line(direction, "packed", "subset", timed(lambda: sub.packed(direction)), sum(sub.lens), len(sub.lens))
        line(direction, "per_file", "subset" if sub else "whole", timed(lambda: s.per_file(direction)), sum(s.lens), len(s.lens))
    torch.cuda.synchronize()
    bad = int((whole.status != 0).sum().item()) + (int((sub.status != 0).sum().item()) if sub else 0)
    # the packed call and the per-file calls wrote the same bytes (the last writer of `adx` was the per-file route)
    s = sub or whole
    ref = s.adx.clone()
    s.packed("encode")
    torch.cuda.synchronize()
    same = bool(torch.equal(ref, s.adx))
    print(json.dumps({"tool": "time_adx_ragged", "status_words_set": bad, "packed_equals_per_file": same}), flush=True)
    if bad or not same:
        raise SystemExit("the routes disagree")


if __name__ == "__main__":
    main()
