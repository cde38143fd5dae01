#!/usr/bin/env python3
"""GPU time of the HCA file sets (vga_hca_write_device_v / vga_hca_read_device_v; include/vgaudio_hip/hca_files.h) against
the per-file calls they replace and against a plain copy, on three shapes:

  equal     the shape of DESIGN 4.10: 1024 stereo streams of 2813 frames of 682 bytes.  The read with bad-CRC counts against
            vga_hca_read_device on the same images, the write against vga_hca_write_device; both again with one type-56 key,
            against the per-file call plus vga_hca_crypt_device; hipMemcpyAsync of the same bytes.
  ragged    bench.py's 10 008 file lengths (1-120 s at 48 kHz, seed 0xBA7C4) as stereo streams of one shape class: the write
            and the read alone, without and with a key.
  subset    a seeded 1 000 files of them against one per-file call per file (what a caller with device-resident files of
            different lengths had before).

    python tools/time_hca_files.py [--runs 7] [--warmup 2] [--shapes equal,ragged,subset] [--files N]

Both calls only move bytes, so the frames are seeded random bytes made on the device; their CRCs are made valid by one keyed
write under the identity table, so that the counting read counts nothing.  Device events around the calls on one stream; the
contenders of a comparison alternate run by run in one process; the minimum and the median of --runs runs each, and their
spread.  The bytes of the routes are compared before anything is timed.  One JSON line per (shape, call, route)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402
from vgaudio_amd.hca import HcaFileSet  # noqa: E402

KEY = 0xCC55463930DBE1AB


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


def info_for(samples):
    p, h = _lib.HcaParamsC(2, 0, 0, 2, 48000, samples, 0, 0, 0), _lib.HcaInfoC()
    _lib.check(_lib.lib().vga_hca_encoder_initialize(C.byref(p), C.byref(h)))
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="equal,ragged,subset")
    ap.add_argument("--files", type=int, default=0, help="only the first N lengths of the ragged set (0 = all)")
    ap.add_argument("--streams", type=int, default=1024, help="streams of the equal shape")
    a = ap.parse_args()
    import torch
    L, check = _lib.lib(), _lib.check
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    up = lambda v, m: (v + m - 1) // m * m
    u8 = lambda t: t.ctypes.data_as(_lib.u8p)
    dec, enc, ident = (np.zeros(256, np.uint8) for _ in range(3))
    check(L.vga_hca_key_tables(56, KEY, u8(dec), u8(enc)))
    ident[:] = np.arange(256)
    tables_w, tables_r = np.stack([enc, ident]), np.stack([dec, ident])

    def timed(calls):
        for call in calls:
            for _ in range(a.warmup):
                call()
        torch.cuda.synchronize()
        ms = [[] for _ in calls]
        for _ in range(a.runs):
            for k, call in enumerate(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return [{"min_ms": round(min(m), 3), "median_ms": round(float(np.median(m)), 3), "max_ms": round(max(m), 3)} for m in ms]

    def line(shape, call, route, t, nbytes, files):
        print(json.dumps({"tool": "time_hca_files", "shape": shape, "call": call, "route": route, "files": files, "bytes_each_way": int(nbytes),
                          **t, "gb_per_s_each_way": round(nbytes / t["min_ms"] / 1e6, 1)}), flush=True)

    def random_bytes(n):
        t = torch.empty(up(n, 8) // 8, dtype=torch.int64, device="cuda")
        t.random_()
        return t.view(torch.uint8)[:n]

    class Sets:
        """the four objects over one list of infos (write / read, plain / keyed) and their buffers; frames with valid CRCs"""

        def __init__(self, infos):
            self.infos, n = infos, len(infos)
            mk = lambda key, et, ids: [_lib.HcaFileC(h, None, 1.0, et, ids, key) for h in infos]
            self.w = {False: HcaFileSet(mk(-1, 0, 0)), True: HcaFileSet(mk(0, 56, 1), tables=tables_w)}
            fix = HcaFileSet(mk(1, 0, 0), tables=tables_w)
            t = self.w[False].totals
            self.frames = random_bytes(t.frame_bytes)
            self.images = {k: torch.empty(t.image_bytes, dtype=torch.uint8, device="cuda") for k in (False, True)}
            self.back = torch.empty(t.frame_bytes, dtype=torch.uint8, device="cuda")
            self.bad = torch.zeros(n, dtype=torch.int32, device="cuda")
            fix.write_device(self.frames, self.images[False])          # identity table: the CRCs become valid
            header = infos[0].header_size
            fi = []
            for h in infos:
                i = _lib.HcaFileInfoC()
                i.hca, i.frames_offset, i.volume = h, h.header_size, 1.0
                fi.append(i)
            self.fi = fi
            plain = HcaFileSet.from_infos(fi)
            plain.read_device(self.images[False], self.back)
            self.frames.copy_(self.back[:self.frames.numel()])
            fix.close()
            self.r = {False: plain, True: HcaFileSet.from_infos(fi, keys=[0] * n, tables=tables_r)}
            for k in (False, True):
                self.w[k].write_device(self.frames, self.images[k])
            # the routes agree before anything is timed: keyed write -> keyed read returns the frames, and counts nothing
            self.r[True].read_device(self.images[True], self.back, self.bad)
            torch.cuda.synchronize()
            assert torch.equal(self.back, self.frames) or torch.equal(self.back[:t.frame_bytes - 8], self.frames[:t.frame_bytes - 8])
            assert int(self.bad.sum()) == 0
            self.bytes = int(sum(h.frame_count * h.frame_size for h in infos))
            assert header == 96

        def write_v(self, keyed):
            return lambda: self.w[keyed].write_device(self.frames, self.images[keyed])

        def read_v(self, keyed, counts=True):
            return lambda: self.r[keyed].read_device(self.images[keyed], self.back, self.bad if counts else None)

    shapes = a.shapes.split(",")
    if "equal" in shapes:
        h, ns = info_for(2813 * 1024 - 128 - 1), a.streams
        h.frame_count = 2813
        s = Sets([h] * ns)
        fb, size = h.frame_count * h.frame_size, h.header_size + h.frame_count * h.frame_size
        fpitch, ipitch = up(fb, 4), up(size, 16)                       # the set's packed layouts are the per-file calls' pitches
        assert s.w[False].totals.frame_bytes == ns * fpitch + 8 and s.w[False].totals.image_bytes == ns * ipitch + 256
        pf_frames = torch.empty(ns * up(fb + 8, 4), dtype=torch.uint8, device="cuda")
        pf_images = torch.empty_like(s.images[False])
        info, fi = C.byref(h), C.byref(s.fi[0])

        def pf_write(keyed):
            def call():
                if keyed:
                    check(L.vga_hca_crypt_device(s.frames.data_ptr(), fpitch, ns, h.frame_count, h.frame_size, u8(enc), S))
                check(L.vga_hca_write_device(info, s.frames.data_ptr(), fpitch, ns, None, 1.0, 56 if keyed else 0, int(keyed),
                                             pf_images.data_ptr(), ipitch, S))
            return call

        def pf_read(keyed):
            def call():
                check(L.vga_hca_read_device(fi, s.images[keyed].data_ptr(), ipitch, ns, pf_frames.data_ptr(), up(fb + 8, 4), s.bad.data_ptr(), S))
                if keyed:
                    check(L.vga_hca_crypt_device(pf_frames.data_ptr(), up(fb + 8, 4), ns, h.frame_count, h.frame_size, u8(dec), S))
            return call

        pf_write(False)()                                              # the bytes agree (the keyed per-file write encrypts in place: timed last)
        pf_read(True)()
        torch.cuda.synchronize()
        assert torch.equal(pf_images[:ns * ipitch].view(ns, ipitch)[:, :size], s.images[False][:ns * ipitch].view(ns, ipitch)[:, :size])
        assert torch.equal(pf_frames.view(ns, -1)[:, :fb], s.frames[:ns * fpitch].view(ns, fpitch)[:, :fb])
        copy = lambda: memcpy(s.back.data_ptr(), s.frames.data_ptr(), s.bytes, 3, S)
        for call, pair in (("read", (s.read_v(False), pf_read(False), copy)), ("read_keyed", (s.read_v(True), pf_read(True), copy)),
                           ("write", (s.write_v(False), pf_write(False), copy)), ("write_keyed", (s.write_v(True), pf_write(True), copy))):
            for route, t in zip(("set", "per_file", "memcpy"), timed(pair)):
                line("equal", call, route, t, s.bytes, ns)
        for route, t in zip(("set_no_counts",), timed((s.read_v(False, counts=False),))):
            line("equal", "read", route, t, s.bytes, ns)
        del s, pf_frames, pf_images
        torch.cuda.empty_cache()

    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    if "ragged" in shapes:
        s = Sets([info_for(n) for n in lens])
        copy = lambda: memcpy(s.back.data_ptr(), s.frames.data_ptr(), s.bytes, 3, S)
        names = ("write", "write_keyed", "read", "read_keyed", "read_no_counts", "memcpy")
        calls = (s.write_v(False), s.write_v(True), s.read_v(False), s.read_v(True), s.read_v(False, counts=False), copy)
        for name, t in zip(names, timed(calls)):
            line("ragged", name, "set" if name != "memcpy" else "memcpy", t, s.bytes, len(lens))
        print(json.dumps({"tool": "time_hca_files", "shape": "ragged", "stats": s.w[False].stats(), "total_frames": int(s.w[False].totals.total_frames)}))
        del s
        torch.cuda.empty_cache()

    if "subset" in shapes:
        rng = np.random.default_rng(0x5B5E7)
        picks = sorted(rng.choice(len(lens), size=min(1000, len(lens)), replace=False))
        infos = [info_for(lens[k]) for k in picks]
        s = Sets(infos)
        w, r = s.w[False], s.r[False]
        out_i, out_f = torch.empty_like(s.images[False]), torch.empty(s.back.numel() + 8 * len(infos), dtype=torch.uint8, device="cuda")
        fo, io = [int(v) for v in w.frame_offsets], [int(v) for v in w.image_offsets]

        def pf_write():
            for k, h in enumerate(infos):
                n = h.frame_count * h.frame_size
                check(L.vga_hca_write_device(C.byref(h), s.frames.data_ptr() + fo[k], n, 1, None, 1.0, 0, 0, out_i.data_ptr() + io[k],
                                             h.header_size + n, S))

        def pf_read():
            for k, h in enumerate(infos):
                n = h.frame_count * h.frame_size
                check(L.vga_hca_read_device(C.byref(s.fi[k]), s.images[False].data_ptr() + io[k], h.header_size + n, 1,
                                            out_f.data_ptr() + fo[k] + 8 * k, up(n + 8, 4), s.bad.data_ptr() + 4 * k, S))

        for call, pair in (("write", (s.write_v(False), pf_write)), ("read", (s.read_v(False), pf_read))):
            for route, t in zip(("set", "per_file"), timed(pair)):
                line("subset", call, route, t, s.bytes, len(infos))


if __name__ == "__main__":
    main()
