#!/usr/bin/env python3
"""GPU time of the packed NintendoWare stream writer and reader (vga_nwstm_write_device_v / vga_nwstm_read_device_v;
include/vgaudio_hip/nw_files.h) on the file set of bench.py's ragged block: 10 008 files of 1-120 s at 48 kHz (seed 0xBA7C4,
log-uniform, as many as hold 4096 x 60 s).  Even files are mono and do not loop; odd files are stereo and loop from a seeded
loop start to their end.  BRSTM with the default configuration (interleave, seek spacing and loop alignment 14 336).  Both
calls only move bytes, so the rows, tables and per-channel arrays are filled with seeded random bytes on the device instead of
being encoded: the images are well-formed containers of noise.

    python tools/time_nw_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000]

Device events around the calls on one stream, medians (and the spread) of --calls repeats after a warm-up of every shape, one
process:
  packed    one vga_nwstm_write_device_v call over the whole set, and over a seeded --subset of the files; then one
            vga_nwstm_read_device_v call over the images it wrote;
  per_file  what a caller with device-resident files had before, on the subset: one vga_nwstm_write_device (one
            vga_nwstm_read_device) call per file on the same packed buffers; timed alternating with the packed call;
  copy      hipMemcpyAsync device to device of image_bytes: the copy ceiling.
The bytes of both routes are compared before anything is timed, and on the subset the headers the reader's set is made from
are compared with vga_nwstm_parse of the images.  One JSON line per (form, set)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402
from vgaudio_amd.nwstm import NwFileSet, NwTarget, _file_config  # noqa: E402

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
    a = ap.parse_args()
    assert a.calls >= 10 or a.files, "at least 10 repetitions"
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    starts = np.random.default_rng(0xA119).integers(1, 16000, len(lens))
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    cfg = _file_config(NwTarget.Revolution)
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
        return [{"median_ms": round(float(np.median(m)), 3), "min_ms": round(min(m), 3), "max_ms": round(max(m), 3)} for m in ms]

    def line(form, which, t, nbytes, st):
        print(json.dumps({"tool": "time_nw_files", "set": which, "files": st.s.files, "form": form, "bytes": int(nbytes), **t,
                          "gb_per_s": round(nbytes / t["median_ms"] / 1e6, 1)}), flush=True)

    class Set:
        """files (index k of the whole set decides the shape), their rows resident; the buffers of both routes"""

        def __init__(self, picks, both):
            self.files = [_lib.NwFileC(1 + k % 2, RATE, lens[k], k % 2, int(starts[k]) if k % 2 else 0, lens[k] if k % 2 else 0) for k in picks]
            self.s = NwFileSet(self.files, NwTarget.Revolution, cfg)
            s, t = self.s, self.s.totals
            nch = s.channels
            self.lay = [NwFileSet.file_layout(f, cfg) for f in self.files]
            g = torch.Generator(device=dev)
            g.manual_seed(0x17)
            rnd = lambda nbytes, dt: torch.randint(0, 256, (up(max(int(nbytes), 16), 16),), dtype=torch.uint8, device=dev, generator=g).view(dt)
            self.adpcm, self.coefs = rnd(t.adpcm_bytes, torch.uint8), rnd(nch * 32, torch.int16)
            self.seek, self.ctx = rnd(t.seek_shorts * 2, torch.int16), rnd(nch * 6, torch.int16)
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            self.images = [z(t.image_bytes, torch.uint8) for _ in range(2)]       # ([1]: the per-file route's, the copy's destination)
            ao = np.zeros(nch, np.int64)
            check(L.vga_gcadpcm_ragged_offsets(s.ragged, None, ao.ctypes.data_as(C.POINTER(C.c_int64))))
            self.ao = ao
            self.params = []
            for f in self.files:
                p = _lib.NwParamsC()
                p.target, p.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end = 0, f.sample_rate, f.sample_count, f.looping, f.loop_start, f.loop_end
                p.endianness = -1
                self.params.append(p)
            # the read side: the headers of the images as vga_nwstm_parse returns them (checked on the subset)
            self.infos = []
            for f, lay in zip(self.files, self.lay):
                i = _lib.NwInfoC()
                i.channel_count, i.sample_count, i.sample_rate = f.channels, lay.sample_count, f.sample_rate
                i.interleave_size, i.audio_data_offset, i.audio_data_length = lay.interleave_size, lay.audio_data_offset, lay.audio_data_size * f.channels
                i.adpcm_bytes = L.vga_gcadpcm_sample_count_to_byte_count(lay.sample_count)
                self.infos.append(i)
            self.r = NwFileSet.from_infos(self.infos)
            assert list(self.r.image_offsets) == list(s.image_offsets)
            self.rows = [z(self.r.totals.adpcm_bytes, torch.uint8) for _ in range(2 if both else 1)]
            rao = np.zeros(nch, np.int64)
            check(L.vga_gcadpcm_ragged_offsets(self.r.ragged, None, rao.ctypes.data_as(C.POINTER(C.c_int64))))
            self.rao = rao

        def packed(self):
            self.s.write(self.adpcm, self.coefs, self.images[0], loop_context=self.ctx, seek=self.seek)

        def per_file(self):
            s = self.s
            for f, (nf, p, lay) in enumerate(zip(self.files, self.params, self.lay)):
                c = int(s.first_channel[f])
                check(L.vga_nwstm_write_device(
                    C.byref(p), nf.channels, 1, None, self.adpcm.data_ptr() + int(self.ao[c]), up(lay.channel_adpcm_bytes, 16), lay.channel_adpcm_bytes,
                    self.coefs.data_ptr() + 32 * c, None, None, self.ctx.data_ptr() + 6 * c, self.seek.data_ptr() + 2 * int(s.seek_offsets[c]),
                    up(2 * lay.channel_seek_entries, 8), lay.channel_seek_entries, self.images[1].data_ptr() + int(s.image_offsets[f]), lay.file_size, S))

        def read_packed(self):
            self.r.read(self.images[0], self.rows[0])

        def read_per_file(self):
            r = self.r
            for f, i in enumerate(self.infos):
                c = int(r.first_channel[f])
                check(L.vga_nwstm_read_device(C.byref(i), self.images[0].data_ptr() + int(r.image_offsets[f]), r.image_sizes[f], 1,
                                              self.rows[1].data_ptr() + int(self.rao[c]), up(i.adpcm_bytes, 16), S))

        def copy(self):
            check(0 if memcpy(self.images[1].data_ptr(), self.images[0].data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def check_infos(self):
            host = self.images[0].cpu().numpy()
            for f, i in enumerate(self.infos):
                at, got = int(self.s.image_offsets[f]), _lib.NwInfoC()
                image = host[at:at + self.lay[f].file_size]
                check(L.vga_nwstm_parse(image.ctypes.data_as(_lib.u8p), len(image), C.byref(got)))
                for k in ("channel_count", "sample_count", "interleave_size", "audio_data_offset", "audio_data_length", "adpcm_bytes"):
                    assert getattr(got, k) == getattr(i, k), (f, k)

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    def run(which, st, both):
        t = st.s.totals
        st.packed()
        st.read_packed()
        torch.cuda.synchronize()
        if both:                                                       # the bytes of both routes, before anything is timed
            st.per_file()
            st.read_per_file()
            torch.cuda.synchronize()
            st.check_infos()
            same = {"images": bool(torch.equal(st.images[0], st.images[1])), "rows": bool(torch.equal(st.rows[0], st.rows[1]))}
            print(json.dumps({"tool": "time_nw_files", "set": which, "packed_equals_per_file": same}), flush=True)
            if not all(same.values()):
                raise SystemExit("the routes disagree")
            tp, tf = timed([st.packed, st.per_file])
            line("write packed", which, tp, t.image_bytes, st)
            line("write per_file", which, tf, t.image_bytes, st)
            tp, tf = timed([st.read_packed, st.read_per_file])
            line("read packed", which, tp, t.image_bytes, st)
            line("read per_file", which, tf, t.image_bytes, st)
        else:
            line("write packed", which, timed([st.packed])[0], t.image_bytes, st)
            line("read packed", which, timed([st.read_packed])[0], t.image_bytes, st)
        line("hipMemcpyAsync", which, timed([st.copy])[0], t.image_bytes, st)

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    for which, picks, both in (("subset", pick, True), ("whole", list(range(nfiles)), False)):
        st = Set(picks, both)
        print(json.dumps({"tool": "time_nw_files", "set": which, "files": st.s.files, "channels": st.s.channels,
                          "image_bytes": st.s.totals.image_bytes, "adpcm_bytes": st.s.totals.adpcm_bytes, "seek_shorts": st.s.totals.seek_shorts}),
              flush=True)
        run(which, st, both)
        st.close()
        del st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
