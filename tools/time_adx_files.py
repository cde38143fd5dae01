#!/usr/bin/env python3
"""GPU time of the packed ADX writer and reader (vga_adx_write_device_v / vga_adx_read_device_v; include/vgaudio_hip/adx_files.h)
on the file set of bench.py's ragged block: 10 008 files of 1-120 s at 48 kHz (seed 0xBA7C4, log-uniform, as many as hold
4096 x 60 s), once as mono files and once with the same lengths as stereo files; version 4, 18-byte frames, no loop.  Both calls
only move bytes, so the rows are filled with seeded random bytes on the device instead of being encoded: the images are
well-formed containers of noise.

    python tools/time_adx_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000] [--channels 1,2]

Device events around the calls on one stream, means and medians (and the spread) of --calls repeats after a warm-up of every
shape, one process:
  packed    one vga_adx_write_device_v call over the whole set, and over a seeded --subset of the files; then one
            vga_adx_read_device_v call over the images it wrote;
  general   the same calls under vga_adx_files_force_general_this_thread(1): every file in the general form, timed alternating
            with the packed call (the span form against the general form on the same set);
  per_file  what a caller with device-resident files had before, on the subset: one vga_adx_write_device (one
            vga_adx_read_device) call per file on the same packed buffers; timed alternating with the packed call;
  copy      hipMemcpyAsync device to device of image_bytes: the copy ceiling.
The bytes of all routes are compared before anything is timed, and on the subset the headers the reader's set is made from are
compared with vga_adx_parse of the images.  One JSON line per (form, set)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402
from vgaudio_amd.adx import AdxFileSet  # noqa: E402

RATE = 48000


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
    ap.add_argument("--channels", default="1,2", help="channel counts, one run of both sets each")
    a = ap.parse_args()
    assert a.calls >= 10 or a.files, "at least 10 repetitions"
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    up = lambda v, m: (v + m - 1) // m * m

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
        return [{"mean_ms": round(float(np.mean(m)), 3), "median_ms": round(float(np.median(m)), 3), "min_ms": round(min(m), 3),
                 "max_ms": round(max(m), 3)} for m in ms]

    def line(form, which, t, nbytes, st):
        print(json.dumps({"tool": "time_adx_files", "set": which, "files": st.s.files, "channels_per_file": st.nch, "form": form,
                          "bytes": int(nbytes), **t, "gb_per_s": round(nbytes / t["mean_ms"] / 1e6, 1)}), flush=True)

    class forced:
        def __enter__(self):
            L.vga_adx_files_force_general_this_thread(1)

        def __exit__(self, *exc):
            L.vga_adx_files_force_general_this_thread(0)

    class Set:
        """files of nch channels, their rows resident; the buffers of all routes"""

        def __init__(self, picks, nch, both):
            self.nch = nch
            self.files = [_lib.AdxFileC(nch, _lib.AdxFileParamsC(RATE, lens[k], 0, 0, 0, 0, 18, 4, 3, 500, 0, 1)) for k in picks]
            self.s = AdxFileSet(self.files)
            s, t = self.s, self.s.totals
            self.lay = [AdxFileSet.file_layout(f) for f in self.files]
            g = torch.Generator(device=dev)
            g.manual_seed(0x17)
            rnd = lambda nbytes, dt: torch.randint(0, 256, (up(max(int(nbytes), 16), 16),), dtype=torch.uint8, device=dev, generator=g).view(dt)
            self.audio, self.hist = rnd(t.audio_bytes, torch.uint8), rnd(s.channels * 2, torch.int16)
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            self.images = [z(t.image_bytes, torch.uint8) for _ in range(2)]       # ([1]: the other routes', the copy's destination)
            # the read side: the headers of the images as vga_adx_parse returns them (checked on the subset)
            self.infos = []
            for f, lay in zip(self.files, self.lay):
                i = _lib.AdxFileInfoC()
                i.header_size, i.frame_size, i.channel_count, i.sample_count, i.version = lay.header_size, 18, nch, lay.sample_count, 4
                i.audio_offset, i.samples_per_frame, i.frame_count, i.audio_bytes = lay.audio_offset, 32, lay.frame_count, lay.frame_count * 18
                self.infos.append(i)
            self.r = AdxFileSet.from_infos(self.infos, [int(o) for o in s.image_offsets])   # (an image ends with its audio for the reader)
            assert list(self.r.audio_offsets) == list(s.audio_offsets)
            self.rows = [z(self.r.totals.audio_bytes, torch.uint8) for _ in range(2)]
            self.both = both

        def packed(self):
            self.s.write_device(self.audio, self.images[0], history=self.hist)

        def general(self):
            with forced():
                self.s.write_device(self.audio, self.images[1], history=self.hist)

        def per_file(self):
            s = self.s
            for f, (file, lay) in enumerate(zip(self.files, self.lay)):
                c, n = int(s.first_channel[f]), lay.frame_count * 18
                check(L.vga_adx_write_device(self.audio.data_ptr() + int(s.audio_offsets[c]), up(n, 16), n, self.hist.data_ptr() + 2 * c, self.nch,
                                             C.byref(file.params), self.images[1].data_ptr() + int(s.image_offsets[f]), S))

        def read_packed(self):
            self.r.read_device(self.images[0], self.rows[0])

        def read_general(self):
            with forced():
                self.r.read_device(self.images[0], self.rows[1])

        def read_per_file(self):
            r = self.r
            for f, i in enumerate(self.infos):
                c = int(r.first_channel[f])
                check(L.vga_adx_read_device(C.byref(i), self.images[0].data_ptr() + int(r.image_offsets[f]), r.image_sizes[f], 1,
                                            self.rows[1].data_ptr() + int(r.audio_offsets[c]), up(i.audio_bytes, 16), S))

        def copy(self):
            check(0 if memcpy(self.images[1].data_ptr(), self.images[0].data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def check_infos(self):
            host = self.images[0].cpu().numpy()
            for f, i in enumerate(self.infos):
                at, got = int(self.s.image_offsets[f]), _lib.AdxFileInfoC()
                image = host[at:at + self.lay[f].file_size]
                check(L.vga_adx_parse(image.ctypes.data_as(_lib.u8p), len(image), C.byref(got)))
                for k in ("channel_count", "sample_count", "frame_size", "audio_offset", "frame_count", "audio_bytes", "version"):
                    assert getattr(got, k) == getattr(i, k), (f, k)

        def same(self, what):
            """images[1] / rows[1] against the packed call's, then cleared for the next route"""
            torch.cuda.synchronize()
            same = {"images": bool(torch.equal(self.images[0], self.images[1])), "rows": bool(torch.equal(self.rows[0], self.rows[1]))}
            print(json.dumps({"tool": "time_adx_files", "set": what, "equals_packed": same}), flush=True)
            if not all(same.values()):
                raise SystemExit("the routes disagree")
            self.images[1].zero_()
            self.rows[1].zero_()

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    def run(which, st):
        t = st.s.totals
        st.packed()
        st.read_packed()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "time_adx_files", "set": which, "write_stats": st.s.stats(), "read_stats": st.r.stats()}), flush=True)
        st.general()                                                   # the bytes of every route, before anything is timed
        st.read_general()
        st.same(which + ": general")
        if st.both:
            st.per_file()
            st.read_per_file()
            st.check_infos()
            st.same(which + ": per_file")
            tp, tg, tf = timed([st.packed, st.general, st.per_file])
            line("write per_file", which, tf, t.image_bytes, st)
        else:
            tp, tg = timed([st.packed, st.general])
        line("write packed", which, tp, t.image_bytes, st)
        line("write general", which, tg, t.image_bytes, st)
        if st.both:
            tp, tg, tf = timed([st.read_packed, st.read_general, st.read_per_file])
            line("read per_file", which, tf, t.image_bytes, st)
        else:
            tp, tg = timed([st.read_packed, st.read_general])
        line("read packed", which, tp, t.image_bytes, st)
        line("read general", which, tg, t.image_bytes, st)
        line("hipMemcpyAsync", which, timed([st.copy])[0], t.image_bytes, st)

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    for nch in [int(c) for c in a.channels.split(",")]:
        for which, picks, both in (("subset", pick, True), ("whole", list(range(nfiles)), False)):
            st = Set(picks, nch, both)
            which = "%s x%d" % (which, nch)
            print(json.dumps({"tool": "time_adx_files", "set": which, "files": st.s.files, "channels": st.s.channels,
                              "image_bytes": st.s.totals.image_bytes, "audio_bytes": st.s.totals.audio_bytes}), flush=True)
            run(which, st)
            st.close()
            del st
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
