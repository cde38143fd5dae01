#!/usr/bin/env python3
"""GPU time of the packed GC-ADPCM file calls (vga_gcadpcm_build_channels_device_v, vga_dsp_write_device_v,
vga_dsp_read_device_v; include/vgaudio_hip/gc_files.h) on the file set of bench.py's ragged block: 10 008 files of 1-120 s at
48 kHz (seed 0xBA7C4, log-uniform, as many as hold 4096 x 60 s), already encoded and resident.  Even files are mono, odd files
stereo and looping from a quarter of their length to their end; seek entries every 0x3800 samples; the default
DspConfiguration.  PCM is generated on the device by vga_synth_pcm16_device and encoded by the ragged codec calls.

    python tools/time_gc_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000]

Device events around the calls on one stream, medians (and the spread) of --calls repeats after --warmup, one process:
  packed    one *_device_v call over the whole set, and over a seeded --subset of the files;
  per_file  what a caller with device-resident files had before, on the subset: one vga_gcadpcm_build_channels_device, one
            vga_dsp_write_device, one vga_dsp_read_device call per file on the same packed buffers;
  copy      hipMemcpyAsync device to device of image_bytes: the copy ceiling of the writer and the reader.
The bytes of both routes are compared.  One JSON line per (call, form, set)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib, synth  # noqa: E402
from vgaudio_amd.dsp import DspConfiguration, DspFileSet  # noqa: E402

RATE, SPACING = 48000, 0x3800


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
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    cfg = DspConfiguration()
    bc = L.vga_gcadpcm_sample_count_to_byte_count

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

    def line(call, form, which, t, nbytes, files):
        print(json.dumps({"tool": "time_gc_files", "set": which, "files": files, "call": call, "form": form, "bytes": int(nbytes), **t,
                          "gb_per_s": round(nbytes / t["median_ms"] / 1e6, 1)}), flush=True)

    class Set:
        """files (index k of the whole set decides the shape), encoded and resident; the buffers of both routes"""

        def __init__(self, picks, both):
            copies = 2 if both else 1                                  # the per-file route writes buffers of its own
            self.shapes = [(1 + k % 2, lens[k], k % 2, lens[k] // 4 if k % 2 else 0, lens[k] if k % 2 else 0) for k in picks]
            self.s = DspFileSet([(nch, RATE, n, loop, ls, le, 0, SPACING) for nch, n, loop, ls, le in self.shapes], cfg)
            s, t = self.s, self.s.totals
            nch = s.channels
            po, ao = np.zeros(nch, np.int64), np.zeros(nch, np.int64)
            i64p = C.POINTER(C.c_int64)
            check(L.vga_gcadpcm_ragged_offsets(s.ragged, po.ctypes.data_as(i64p), ao.ctypes.data_as(i64p)))
            self.po, self.ao = po, ao
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            pcm = z(t.pcm_samples, torch.int16)
            self.adpcm, self.coefs = z(t.adpcm_bytes, torch.uint8), z(nch * 16, torch.int16)
            params = torch.from_numpy(np.array([synth.channel_params(c) for c in range(nch)], dtype=np.uint32).reshape(nch, 4).view(np.int32)).to(dev)
            c = 0
            for fnch, n, *_ in self.shapes:                            # one launch per channel: set-up, not the timed path
                for _ in range(fnch):
                    check(L.vga_synth_pcm16_device(pcm.data_ptr() + 2 * int(po[c]), max(n, 8), 1, n, c, params[c].data_ptr(), S))
                    c += 1
            ws = z(max(L.vga_gcadpcm_ragged_coefs_workspace_bytes(s.ragged), t.build_workspace_bytes), torch.uint8)
            check(L.vga_gcadpcm_coefs_device_v(s.ragged, pcm.data_ptr(), self.coefs.data_ptr(), ws.data_ptr(), ws.numel(), S))
            check(L.vga_gcadpcm_encode_device_v(s.ragged, pcm.data_ptr(), self.coefs.data_ptr(), None, None, self.adpcm.data_ptr(), S))
            torch.cuda.synchronize()
            del pcm
            self.ws = ws
            self.seek, self.ctx = [z(t.seek_shorts, torch.int16) for _ in range(copies)], [z(nch * 3, torch.int16) for _ in range(copies)]
            self.images = [z(t.image_bytes, torch.uint8) for _ in range(2)]      # ([1]: the copy's destination as well)
            self.rows = [z(t.adpcm_bytes, torch.uint8) for _ in range(copies)]
            self.status = z(1, torch.int32)
            # the per-file calls' arguments
            self.params = [_lib.GcChannelParamsC(n, loop, ls, le, 0, SPACING) for _, n, loop, ls, le in self.shapes]
            self.dsp = [_lib.DspParamsC(RATE, n, loop, ls, le, cfg.SamplesPerInterleave, cfg.LoopPointAlignment, int(cfg.TrimFile))
                        for _, n, loop, ls, le in self.shapes]
            self.file_ws = z(max(L.vga_gcadpcm_build_channels_workspace_bytes(fnch, C.byref(p)) for (fnch, *_), p in zip(self.shapes, self.params)),
                             torch.uint8)
            self.infos = []
            for (fnch, n, *_), d in zip(self.shapes, self.dsp):
                lay, i = _lib.DspLayoutC(), _lib.DspInfoC()
                check(L.vga_dsp_layout_for(C.byref(d), fnch, C.byref(lay)))
                i.sample_count, i.nibble_count, i.sample_rate = lay.sample_count, L.vga_gcadpcm_sample_count_to_nibble_count(lay.sample_count), RATE
                i.channel_count, i.frames_per_interleave = fnch, lay.frames_per_interleave if fnch > 1 else 0
                i.audio_offset, i.adpcm_bytes = 0x60 * fnch, bc(lay.sample_count)
                i.interleave_size = i.frames_per_interleave * 8
                i.data_length = i.adpcm_bytes if fnch == 1 else (i.adpcm_bytes + 7) // 8 * 8 * fnch
                assert i.audio_offset + i.data_length == lay.file_size and lay.sample_count == n      # (nothing trimmed: the rows are the files')
                self.infos.append(i)
            self.r = DspFileSet.from_infos(self.infos)
            assert np.array_equal(self.r.image_offsets, s.image_offsets) and self.r.totals.adpcm_bytes == t.adpcm_bytes

        def build(self, packed):
            s, k = self.s, 0 if packed else 1
            if packed:
                s.build_channels(self.adpcm, self.coefs, seek=self.seek[0], loop_context=self.ctx[0], status=self.status, workspace=self.ws)
                return
            for f, ((fnch, n, *_), p) in enumerate(zip(self.shapes, self.params)):
                c = int(s.first_channel[f])
                entries = -(-n // SPACING)
                check(L.vga_gcadpcm_build_channels_device(
                    self.adpcm.data_ptr() + int(self.ao[c]), (bc(n) + 15) // 16 * 16, self.coefs.data_ptr() + 32 * c, fnch, C.byref(p), None, 0,
                    None, 0, self.seek[k].data_ptr() + 2 * int(s.seek_offsets[c]), (2 * entries + 7) // 8 * 8, self.ctx[k].data_ptr() + 6 * c,
                    self.file_ws.data_ptr(), self.file_ws.numel(), S))

        def write(self, packed):
            s = self.s
            if packed:
                s.write_images(self.adpcm, self.coefs, self.images[0], loop_context=self.ctx[0])
                return
            for f, ((fnch, n, *_), d) in enumerate(zip(self.shapes, self.dsp)):
                c = int(s.first_channel[f])
                check(L.vga_dsp_write_device(self.adpcm.data_ptr() + int(self.ao[c]), (bc(n) + 15) // 16 * 16, bc(n), self.coefs.data_ptr() + 32 * c,
                                             None, None, self.ctx[0].data_ptr() + 6 * c, fnch, C.byref(d),
                                             self.images[1].data_ptr() + int(s.image_offsets[f]), S))

        def read(self, packed):
            s = self.s
            if packed:
                self.r.read_images(self.images[0], self.rows[0])
                return
            for f, ((fnch, n, *_), i) in enumerate(zip(self.shapes, self.infos)):
                c = int(s.first_channel[f])
                check(L.vga_dsp_read_device(C.byref(i), self.images[0].data_ptr() + int(s.image_offsets[f]), i.audio_offset + i.data_length, 1,
                                            self.rows[1].data_ptr() + int(self.ao[c]), (bc(n) + 15) // 16 * 16, S))

        def copy(self):
            check(0 if memcpy(self.images[1].data_ptr(), self.images[0].data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    def run(which, st, per_file):
        t = st.s.totals
        pcm_bytes = 2 * sum(nch * n for nch, n, *_ in st.shapes)
        line("build_channels", "packed", which, timed(lambda: st.build(True)), pcm_bytes, st.s.files)
        line("write", "packed", which, timed(lambda: st.write(True)), t.image_bytes, st.s.files)
        line("read", "packed", which, timed(lambda: st.read(True)), t.image_bytes, st.s.files)
        line("copy", "hipMemcpyAsync", which, timed(st.copy), t.image_bytes, st.s.files)
        if not per_file:
            return
        line("build_channels", "per_file", which, timed(lambda: st.build(False)), pcm_bytes, st.s.files)
        line("write", "per_file", which, timed(lambda: st.write(False)), t.image_bytes, st.s.files)
        line("read", "per_file", which, timed(lambda: st.read(False)), t.image_bytes, st.s.files)
        st.write(True)                                                 # (the copy overwrote nothing of images[0]; images[1] holds the per-file route's)
        torch.cuda.synchronize()
        same = {"seek": bool(torch.equal(st.seek[0], st.seek[1])), "loop_context": bool(torch.equal(st.ctx[0], st.ctx[1])),
                "images": bool(torch.equal(st.images[0], st.images[1])), "rows": bool(torch.equal(st.rows[0], st.rows[1])),
                "rows_are_the_encoders": bool(torch.equal(st.rows[0], st.adpcm)),
                "status": int(st.status.item())}
        print(json.dumps({"tool": "time_gc_files", "set": which, "packed_equals_per_file": same}), flush=True)
        if not all(v is True for k, v in same.items() if k != "status") or same["status"]:
            raise SystemExit("the routes disagree")

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    sub = Set(pick, True)
    print(json.dumps({"tool": "time_gc_files", "set": "subset", "files": sub.s.files, "channels": sub.s.channels,
                      "image_bytes": sub.s.totals.image_bytes, "seek_shorts": sub.s.totals.seek_shorts}), flush=True)
    run("subset", sub, True)
    sub.close()
    del sub
    torch.cuda.empty_cache()
    whole = Set(list(range(nfiles)), False)
    print(json.dumps({"tool": "time_gc_files", "set": "whole", "files": whole.s.files, "channels": whole.s.channels,
                      "image_bytes": whole.s.totals.image_bytes, "seek_shorts": whole.s.totals.seek_shorts}), flush=True)
    run("whole", whole, False)
    whole.close()


if __name__ == "__main__":
    main()
