#!/usr/bin/env python3
"""GPU time of the packed loop-alignment re-encode (vga_gcadpcm_align_channels_device_v; include/vgaudio_hip/gc_files_aligned.h) on
the file set of bench.py's ragged block: 10 008 files of 1-120 s at 48 kHz (seed 0xBA7C4, log-uniform, as many as hold 4096 x
60 s), already encoded and resident.  Even files are mono and do not loop; odd files are stereo and loop from a seeded loop
start to their end, with the NintendoWare writers' default alignment multiple of 14 336 (so practically every one of them needs
the re-encode) and seek entries every 0x3800 samples.  PCM is generated on the device by vga_synth_pcm16_device and encoded by
the ragged codec calls.

    python tools/time_gc_aligned.py [--calls 10] [--warmup 2] [--files N] [--subset 1000]

Device events around the calls on one stream, medians (and the spread) of --calls repeats after a warm-up of every shape, one
process:
  packed    one vga_gcadpcm_align_channels_device_v call (aligned ADPCM, seek tables, loop contexts) over the whole set, and over
            a seeded --subset of the files;
  per_file  what a caller with device-resident files had before, on the subset: one vga_gcadpcm_build_channels_device call per
            file on the same packed buffers; timed alternating with the packed call, repeat by repeat;
  copy      hipMemcpyAsync device to device of out_adpcm_bytes: the copy floor.
The bytes of both routes are compared before anything is timed.  One JSON line per (form, set)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib, synth  # noqa: E402
from vgaudio_amd.gcadpcm import AlignedFileSet  # noqa: E402

RATE, SPACING, MULTIPLE = 48000, 0x3800, 0x3800


def bench_lengths():
    rng = np.random.default_rng(0xBA7C4)
    lens, total = [], 0
    while total < 4096 * 2_880_000:
        lens.append(int(np.exp(rng.uniform(np.log(48000.0), np.log(120 * 48000.0)))))
        total += lens[-1]
    return lens


def hip_memcpy_async():
    import importlib.util
    path = os.path.join(os.path.dirname(importlib.util.find_spec("torch").origin), "lib", "libamdhip64.so")
    f = C.CDLL(path if os.path.exists(path) else "libamdhip64.so").hipMemcpyAsync
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=0, help="only the first N files of the set (0 = all)")
    ap.add_argument("--subset", type=int, default=1000, help="files of the seeded subset the per-file route runs on")
    a = ap.parse_args()
    assert a.calls >= 10 or a.files, "at least 10 repetitions"
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    starts = np.random.default_rng(0xA119).integers(1, 16000, len(lens))      # loop starts: aligned, they stay inside the shortest file
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    bc = L.vga_gcadpcm_sample_count_to_byte_count

    def timed(calls):
        """the calls of `calls` alternating, repeat by repeat: one result per call"""
        for call in calls:
            for _ in range(a.warmup):
                call()
        torch.cuda.synchronize()
        ms = [[] for _ in calls]
        for _ in range(a.calls):
            for k, call in enumerate(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [{"median_ms": round(float(np.median(m)), 3), "min_ms": round(min(m), 3), "max_ms": round(max(m), 3)} for m in ms]

    def line(form, which, t, nbytes, st):
        print(json.dumps({"tool": "time_gc_aligned", "set": which, "files": st.s.files, "aligned_channels": st.s.totals.aligned_channels,
                          "form": form, "bytes": int(nbytes), **t, "gb_per_s": round(nbytes / t["median_ms"] / 1e6, 1)}), flush=True)

    class Set:
        """files (index k of the whole set decides the shape), encoded and resident; the buffers of both routes"""

        def __init__(self, picks, both):
            copies = 2 if both else 1                                  # the per-file route writes buffers of its own
            self.shapes = [(1 + k % 2, lens[k], k % 2, int(starts[k]) if k % 2 else 0, lens[k] if k % 2 else 0) for k in picks]
            self.s = AlignedFileSet([(nch, RATE, n, loop, ls, le, MULTIPLE, SPACING) for nch, n, loop, ls, le in self.shapes])
            s, t = self.s, self.s.totals
            nch = s.channels
            po, self.ao = s.offsets("in")
            _, self.aout = s.offsets("out")
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            pcm = z(t.pcm_samples, torch.int16)
            self.adpcm, self.coefs = z(t.adpcm_bytes, torch.uint8), z(nch * 16, torch.int16)
            params = torch.from_numpy(np.array([synth.channel_params(c) for c in range(nch)], dtype=np.uint32).reshape(nch, 4).view(np.int32)).to(dev)
            c = 0
            for fnch, n, *_ in self.shapes:                            # one launch per channel: set-up, not the timed path
                for _ in range(fnch):
                    check(L.vga_synth_pcm16_device(pcm.data_ptr() + 2 * int(po[c]), max(n, 8), 1, n, c, params[c].data_ptr(), S))
                    c += 1
            cws = z(L.vga_gcadpcm_ragged_coefs_workspace_bytes(s.ragged_in), torch.uint8)
            check(L.vga_gcadpcm_coefs_device_v(s.ragged_in, pcm.data_ptr(), self.coefs.data_ptr(), cws.data_ptr(), cws.numel(), S))
            check(L.vga_gcadpcm_encode_device_v(s.ragged_in, pcm.data_ptr(), self.coefs.data_ptr(), None, None, self.adpcm.data_ptr(), S))
            torch.cuda.synchronize()
            del pcm, cws
            torch.cuda.empty_cache()
            self.ws = z(t.workspace_bytes, torch.uint8)
            self.seek, self.ctx = [z(t.seek_shorts, torch.int16) for _ in range(copies)], [z(nch * 3, torch.int16) for _ in range(copies)]
            self.out = [z(t.out_adpcm_bytes, torch.uint8) for _ in range(2)]      # ([1]: the copy's destination as well)
            self.status = z(1, torch.int32)
            # the per-file calls' arguments
            self.params = [_lib.GcChannelParamsC(n, loop, ls, le, MULTIPLE, SPACING) for _, n, loop, ls, le in self.shapes]
            self.file_ws = z(max(L.vga_gcadpcm_build_channels_workspace_bytes(fnch, C.byref(p)) for (fnch, *_), p in zip(self.shapes, self.params)),
                             torch.uint8)

        def packed(self):
            self.s.align_channels(self.adpcm, self.coefs, self.out[0], seek=self.seek[0], loop_context=self.ctx[0], status=self.status,
                                  workspace=self.ws)

        def per_file(self):
            s = self.s
            for f, ((fnch, n, *_), p, lay) in enumerate(zip(self.shapes, self.params, s.layouts)):
                c = int(s.first_channel[f])
                check(L.vga_gcadpcm_build_channels_device(
                    self.adpcm.data_ptr() + int(self.ao[c]), (bc(n) + 15) // 16 * 16, self.coefs.data_ptr() + 32 * c, fnch, C.byref(p),
                    self.out[1].data_ptr() + int(self.aout[c]), (bc(lay.sample_count_aligned) + 15) // 16 * 16, None, 0,
                    self.seek[1].data_ptr() + 2 * int(s.seek_offsets[c]), (2 * lay.seek_table_entries + 7) // 8 * 8, self.ctx[1].data_ptr() + 6 * c,
                    self.file_ws.data_ptr(), self.file_ws.numel(), S))

        def copy(self):
            check(0 if memcpy(self.out[1].data_ptr(), self.out[0].data_ptr(), self.s.totals.out_adpcm_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def close(self):
            torch.cuda.synchronize()
            self.s.close()

    def run(which, st, per_file):
        t = st.s.totals
        if per_file:                                                   # the bytes of both routes, before anything is timed
            st.packed()
            st.per_file()
            torch.cuda.synchronize()
            same = {"adpcm": bool(torch.equal(st.out[0], st.out[1])), "seek": bool(torch.equal(st.seek[0], st.seek[1])),
                    "loop_context": bool(torch.equal(st.ctx[0], st.ctx[1])), "status": int(st.status[0].item())}
            print(json.dumps({"tool": "time_gc_aligned", "set": which, "packed_equals_per_file": same}), flush=True)
            if not all(v is True for k, v in same.items() if k != "status") or same["status"]:
                raise SystemExit("the routes disagree")
            tp, tf = timed([st.packed, st.per_file])
            line("packed", which, tp, t.out_adpcm_bytes, st)
            line("per_file", which, tf, t.out_adpcm_bytes, st)
        else:
            line("packed", which, timed([st.packed])[0], t.out_adpcm_bytes, st)
        line("hipMemcpyAsync", which, timed([st.copy])[0], t.out_adpcm_bytes, st)

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    for which, picks, both in (("subset", pick, True), ("whole", list(range(nfiles)), False)):
        st = Set(picks, both)
        print(json.dumps({"tool": "time_gc_aligned", "set": which, "files": st.s.files, "channels": st.s.channels,
                          "aligned_channels": st.s.totals.aligned_channels, "out_adpcm_bytes": st.s.totals.out_adpcm_bytes,
                          "workspace_bytes": st.s.totals.workspace_bytes, "seek_shorts": st.s.totals.seek_shorts}), flush=True)
        run(which, st, both)
        st.close()
        del st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
