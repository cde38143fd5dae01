#!/usr/bin/env python3
"""GPU time of the packed IDSP and HPS file calls (vga_idsp_write_device_v, vga_idsp_read_device_v,
include/vgaudio_hip_files/idsp_files.h; vga_hps_write_device_v, vga_hps_read_device_v, include/vgaudio_hip_files/hps_files.h) on
the file set of bench.py's ragged block: 10 008 files of 1-120 s at 48 kHz (seed
0xBA7C4, log-uniform, as many as hold 4096 x 60 s).  Even files are mono, odd files stereo; every file loops from a seeded
start to its end, so under the default IdspConfiguration (block size 0x10, trim) almost every loop start needs the alignment
and the rows are those of the aligned sample counts.  Both calls only move bytes, so the rows are random bytes of the aligned
sizes, made on the device: no encode and no re-encode runs here.  The HPS sets are the same files (their alignment is one
block: 114 688 samples mono, 57 344 stereo), their PCM rows zeros (two samples per block and channel are read of them), and
their parsed headers are built from vga_hps_block_map, as vga_hps_parse would return them for the images written.

    python tools/time_gc_stream_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000] [--block-size 16] [--formats idsp,hps]

Device events around the calls on one stream, medians (and the spread) of --calls repeats after --warmup, one process:
  packed    one *_device_v call over the whole set, and over a seeded --subset of the files;
  per_file  IDSP only: what a caller with device-resident files had before, on the subset: one vga_idsp_write_device, one
            vga_idsp_read_device call per file on the same packed buffers (the per-file HPS writer is not run at this size);
  copy      hipMemcpyAsync device to device of image_bytes: the copy ceiling of the writer and the reader.
The bytes of both IDSP routes are compared; the HPS rows read back are compared with the rows written.  One JSON line per
(format, call, form, set)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402
from vgaudio_amd.hps import HpsFileSet  # noqa: E402
from vgaudio_amd.idsp import IdspFileSet  # noqa: E402

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
    ap.add_argument("--block-size", type=int, default=0x10, help="IdspConfiguration.BlockSize of the set")
    ap.add_argument("--formats", default="idsp,hps")
    a = ap.parse_args()
    assert a.calls >= 10 or a.files, "at least 10 repetitions"
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    starts = np.random.default_rng(0x1D5B).integers(0, np.array(lens) // 2)      # the seeded loop starts
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    cfg = _lib.IdspFileConfigC(a.block_size, 1)

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

    def line(call, form, which, t, nbytes, files, fmt="idsp"):
        print(json.dumps({"tool": "time_gc_stream_files", "format": fmt, "set": which, "files": files, "call": call, "form": form,
                          "bytes": int(nbytes), **t, "gb_per_s": round(nbytes / t["median_ms"] / 1e6, 1)}), flush=True)

    class Set:
        """files (index k of the whole set decides the shape), their rows resident; the buffers of both routes"""

        def __init__(self, picks, both):
            copies = 2 if both else 1                                  # the per-file route writes buffers of its own
            self.files = [_lib.IdspFileC(1 + k % 2, RATE, lens[k], 1, int(starts[k]), lens[k]) for k in picks]
            self.s = IdspFileSet(self.files, cfg)
            s, t = self.s, self.s.totals
            nch = s.channels
            ao = np.zeros(nch, np.int64)
            check(L.vga_gcadpcm_ragged_offsets(s.ragged, None, ao.ctypes.data_as(C.POINTER(C.c_int64))))
            self.ao = ao
            self.adpcm = torch.randint(0, 256, (int(t.adpcm_bytes),), dtype=torch.uint8, device=dev)
            self.coefs = torch.randint(-2048, 2048, (nch * 16,), dtype=torch.int16, device=dev)
            self.ctx = torch.randint(-2048, 2048, (nch * 3,), dtype=torch.int16, device=dev)
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            self.images = [z(t.image_bytes, torch.uint8) for _ in range(2)]      # ([1]: the copy's destination as well)
            self.rows = [z(t.adpcm_bytes, torch.uint8) for _ in range(copies)]
            self.params = [IdspFileSet.file_params(f, cfg) for f in self.files]
            self.layouts = [IdspFileSet.file_layout(f, cfg) for f in self.files]
            self.infos = []
            for f, lay in zip(self.files, self.layouts):
                i = _lib.IdspInfoC()
                i.channel_count, i.sample_rate, i.sample_count = f.channels, RATE, lay.sample_count
                i.interleave_size, i.interleave = a.block_size, lay.interleave_size
                i.header_size, i.channel_info_size, i.audio_data_offset, i.audio_data_length = 0x40, 0x60, lay.header_size, lay.audio_data_size
                i.adpcm_bytes = L.vga_gcadpcm_sample_count_to_byte_count(lay.sample_count)
                assert lay.sample_count == lay.channel_sample_count    # (trimmed to the loop end: the rows are the files')
                self.infos.append(i)
            self.r = IdspFileSet.from_infos(self.infos)
            assert np.array_equal(self.r.image_offsets, s.image_offsets) and self.r.totals.adpcm_bytes == t.adpcm_bytes

        def write(self, packed):
            s = self.s
            if packed:
                s.write(self.adpcm, self.coefs, self.images[0], loop_context=self.ctx)
                return
            for f, (x, p, lay) in enumerate(zip(self.files, self.params, self.layouts)):
                c, n = int(s.first_channel[f]), lay.channel_adpcm_bytes
                check(L.vga_idsp_write_device(C.byref(p), x.channels, 1, self.adpcm.data_ptr() + int(self.ao[c]), (n + 15) // 16 * 16, n,
                                              self.coefs.data_ptr() + 32 * c, None, None, self.ctx.data_ptr() + 6 * c,
                                              self.images[1].data_ptr() + int(s.image_offsets[f]), lay.file_size, S))

        def read(self, packed):
            s = self.s
            if packed:
                self.r.read(self.images[0], self.rows[0])
                return
            for f, (i, lay) in enumerate(zip(self.infos, self.layouts)):
                c, n = int(s.first_channel[f]), lay.channel_adpcm_bytes
                check(L.vga_idsp_read_device(C.byref(i), self.images[0].data_ptr() + int(s.image_offsets[f]), lay.file_size, 1,
                                             self.rows[1].data_ptr() + int(self.ao[c]), (n + 15) // 16 * 16, S))

        def copy(self):
            check(0 if memcpy(self.images[1].data_ptr(), self.images[0].data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    class HpsSet:
        """the same files as HPS: their rows and PCM resident, the parsed headers from the block maps"""

        def __init__(self, picks):
            self.files = [_lib.HpsFileC(1 + k % 2, RATE, lens[k], 1, int(starts[k]), lens[k]) for k in picks]
            self.s = HpsFileSet(self.files)
            s, t = self.s, self.s.totals
            nch = s.channels
            self.adpcm = torch.randint(0, 256, (int(t.adpcm_bytes),), dtype=torch.uint8, device=dev)
            self.coefs = torch.randint(-2048, 2048, (nch * 16,), dtype=torch.int16, device=dev)
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            self.pcm = z(t.pcm_samples, torch.int16)
            self.images = [z(t.image_bytes, torch.uint8) for _ in range(2)]
            self.rows = [z(t.adpcm_bytes, torch.uint8)]
            parsed = []
            for f in self.files:
                lay = HpsFileSet.file_layout(f)
                blocks, p = (_lib.HpsBlockC * lay.block_count)(), HpsFileSet.file_params(f)
                check(L.vga_hps_block_map(C.byref(p), f.channels, blocks, lay.block_count))
                i, table = _lib.HpsInfoC(), (_lib.HpsBlockInfoC * lay.block_count)()
                i.sample_rate, i.channel_count, i.sample_count, i.block_count = RATE, f.channels, lay.sample_count, lay.block_count
                i.adpcm_bytes = L.vga_gcadpcm_sample_count_to_byte_count(lay.sample_count)
                assert i.adpcm_bytes == lay.channel_adpcm_bytes        # (the loop ends the file: the rows are the files')
                for b, x in zip(table, blocks):
                    b.offset, b.next_offset, b.size, b.final_nibble = x.offset, x.next_offset, x.written_size, x.end_nibble
                    b.audio_offset, b.audio_bytes, b.out_offset = x.offset + lay.block_header_size, x.channel_size, x.byte_in_index
                parsed.append((i, table))
            self.r = HpsFileSet.from_infos(parsed)
            assert np.array_equal(self.r.image_offsets, s.image_offsets) and self.r.totals.adpcm_bytes == t.adpcm_bytes

        def write(self, packed):
            self.s.write(self.adpcm, self.coefs, self.images[0], pcm=self.pcm)

        def read(self, packed):
            self.r.read(self.images[0], self.rows[0])

        def copy(self):
            check(0 if memcpy(self.images[1].data_ptr(), self.images[0].data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    def run_hps(which, st):
        t = st.s.totals
        line("write", "packed", which, timed(lambda: st.write(True)), t.image_bytes, st.s.files, "hps")
        line("read", "packed", which, timed(lambda: st.read(True)), t.image_bytes, st.s.files, "hps")
        line("copy", "hipMemcpyAsync", which, timed(st.copy), t.image_bytes, st.s.files, "hps")
        torch.cuda.synchronize()
        # every row byte went through the images and came back (the gaps between rows are not moved)
        ao = np.zeros(st.s.channels, np.int64)
        check(L.vga_gcadpcm_ragged_offsets(st.s.ragged, None, ao.ctypes.data_as(C.POINTER(C.c_int64))))
        same = all(bool(torch.equal(st.adpcm[int(o):int(o) + 4096], st.rows[0][int(o):int(o) + 4096])) for o in ao[::max(len(ao) // 64, 1)])
        print(json.dumps({"tool": "time_gc_stream_files", "format": "hps", "set": which, "rows_read_equal_rows_written": same}), flush=True)
        if not same:
            raise SystemExit("the rows read back are not the rows written")

    def describe_hps(which, st):
        items, blocks, table_bytes, _ = st.s.stats()
        ritems, _, rtable_bytes, _ = st.r.stats()
        print(json.dumps({"tool": "time_gc_stream_files", "format": "hps", "set": which, "files": st.s.files, "channels": st.s.channels,
                          "image_bytes": st.s.totals.image_bytes, "blocks": blocks, "block_table_bytes": 32 * blocks, "body_items": items,
                          "table_bytes": table_bytes, "gather_items": ritems, "read_table_bytes": rtable_bytes}), flush=True)

    def run(which, st, per_file):
        t = st.s.totals
        line("write", "packed", which, timed(lambda: st.write(True)), t.image_bytes, st.s.files)
        line("read", "packed", which, timed(lambda: st.read(True)), t.image_bytes, st.s.files)
        line("copy", "hipMemcpyAsync", which, timed(st.copy), t.image_bytes, st.s.files)
        if not per_file:
            return
        line("write", "per_file", which, timed(lambda: st.write(False)), t.image_bytes, st.s.files)
        line("read", "per_file", which, timed(lambda: st.read(False)), t.image_bytes, st.s.files)
        st.write(True)                                                 # (images[1] holds the per-file route's)
        torch.cuda.synchronize()
        same = {"images": bool(torch.equal(st.images[0], st.images[1])), "rows": bool(torch.equal(st.rows[0], st.rows[1]))}
        print(json.dumps({"tool": "time_gc_stream_files", "format": "idsp", "set": which, "packed_equals_per_file": same}), flush=True)
        if not all(same.values()):
            raise SystemExit("the routes disagree")

    def describe(which, st):
        items, wide, table_bytes, _ = st.s.stats()
        print(json.dumps({"tool": "time_gc_stream_files", "format": "idsp", "set": which, "files": st.s.files, "channels": st.s.channels,
                          "block_size": a.block_size, "image_bytes": st.s.totals.image_bytes, "audio_items": items,
                          "items_of_16_bytes": wide, "table_bytes": table_bytes}), flush=True)

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    formats = a.formats.split(",")
    if "idsp" in formats:
        sub = Set(pick, True)
        describe("subset", sub)
        run("subset", sub, True)
        sub.close()
        del sub
        torch.cuda.empty_cache()
        whole = Set(list(range(nfiles)), False)
        describe("whole", whole)
        run("whole", whole, False)
        whole.close()
        del whole
        torch.cuda.empty_cache()
    if "hps" in formats:
        for which, picks in (("subset", pick), ("whole", list(range(nfiles)))):
            st = HpsSet(picks)
            describe_hps(which, st)
            run_hps(which, st)
            st.close()
            del st
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
