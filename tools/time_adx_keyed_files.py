#!/usr/bin/env python3
"""GPU time of the keyed calls on sets of ADX files (vga_adx_write_keyed_device_v / vga_adx_read_keyed_device_v /
vga_adx_find_keys_device_v; include/vgaudio_hip_files/adx_keyed_files.h) on the file set of bench.py's ragged block: 10 008 files
of 1-120 s at 48 kHz (seed 0xBA7C4), once as mono and once as stereo files; version 4, 18-byte frames, no loop, encryption
type 8, one key for all files.  The calls only move and XOR bytes, so the rows are seeded noise made on the device: every
scale below 0x1000 (so the right key passes TestKey) and about 1 % of the frames empty.  The candidate lists are sized like
the reference's (CriAdxEncryptionKeys.cs: 10 key strings + 38 LCG parameter sets = 48 for type 8, 7 key codes for type 9):
made-up keys of the same count, the right one last -- or first, where a line says so.

    python tools/time_adx_keyed_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000] [--channels 1,2]

Device events around the calls on one stream, means, medians and the spread of --calls repeats after a warm-up of every
shape, one process; the calls of one line group are timed alternating, repeat by repeat:
  write / read      the keyed call, the unkeyed vga_adx_write_device_v / vga_adx_read_device_v of the same set, and a
                    hipMemcpyAsync of image_bytes; "ratio_to_unkeyed" is keyed mean / unkeyed mean, next to both spreads;
  general           both keyed calls and their unkeyed calls under vga_adx_files_force_general_this_thread(1): the price of
                    the extra cipher launch;
  find              the search over the whole set with the right key last and with it first, against the copy;
  per_file          on the seeded --subset only, the route that existed before: the unkeyed set call plus one
                    vga_adx_crypt_device per file, and one vga_adx_find_key_device per file, against the new calls.
The bytes of all routes are compared before anything is timed.  One JSON line per (form, set)."""
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
from tools.time_adx_files import bench_lengths, hip_memcpy_async  # noqa: E402

RATE, TYPE, NKEYS8, NKEYS9 = 48000, 8, 48, 7
RIGHT = (0x4A11, 0x5A4D, 0x6B2F)
TOOL = "time_adx_keyed_files"


def candidates():
    """NKEYS8 + NKEYS9 made-up keys, none of them RIGHT"""
    rng = np.random.default_rng(0xC0DE5)
    keys = []
    while len(keys) < NKEYS8 + NKEYS9:
        k = (int(rng.integers(0x4000, 0x8000)), int(rng.integers(0x4000, 0x8000)) | 1, int(rng.integers(0x4000, 0x8000)) | 1)
        if k != RIGHT:
            keys.append(k)
    return keys


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
    right_c = _lib.AdxKeyC(*RIGHT)
    made_up = candidates()
    keys_of = lambda ks: torch.from_numpy(np.array(ks, np.int32).reshape(-1)).to(dev)
    d_right = keys_of([RIGHT])
    d_last = keys_of(made_up[:NKEYS8 - 1] + [RIGHT] + made_up[NKEYS8:])          # keys8 with the right one last, then keys9
    d_first = keys_of([RIGHT] + made_up[:NKEYS8 - 1] + made_up[NKEYS8:])
    host_last = (_lib.AdxKeyC * NKEYS8)(*[_lib.AdxKeyC(*k) for k in made_up[:NKEYS8 - 1] + [RIGHT]])

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
                 "max_ms": round(max(m), 3), "spread": round((max(m) - min(m)) / float(np.median(m)), 3)} for m in ms]

    def line(form, which, t, nbytes, st, **more):
        print(json.dumps({"tool": TOOL, "set": which, "files": st.s.files, "channels_per_file": st.nch, "form": form, "bytes": int(nbytes), **t,
                          "gb_per_s": round(nbytes / t["mean_ms"] / 1e6, 1), **more}), flush=True)

    def ratio(x, y):
        return round(x["mean_ms"] / y["mean_ms"], 3)

    class forced:
        def __enter__(self):
            L.vga_adx_files_force_general_this_thread(1)

        def __exit__(self, *exc):
            L.vga_adx_files_force_general_this_thread(0)

    class Set:
        """files of nch channels, their rows resident; the buffers of all routes"""

        def __init__(self, picks, nch, both):
            self.nch, self.both = nch, both
            self.files = [_lib.AdxFileC(nch, _lib.AdxFileParamsC(RATE, lens[k], 0, 0, 0, 0, 18, 4, 3, 500, TYPE, 1)) for k in picks]
            self.s = AdxFileSet(self.files)
            s, t = self.s, self.s.totals
            self.lay = [AdxFileSet.file_layout(f) for f in self.files]
            g = torch.Generator(device=dev)
            g.manual_seed(0x17)
            z = lambda n, dt: torch.zeros(max(int(n), 16), dtype=dt, device=dev)
            self.audio, self.hist = z(t.audio_bytes, torch.uint8), z(s.channels, torch.int16)
            for f, lay in enumerate(self.lay):                         # seeded noise, scales below 0x1000, about 1 % empty frames
                for c in range(nch):
                    at, frames = int(s.audio_offsets[int(s.first_channel[f]) + c]), lay.frame_count
                    row = torch.randint(1, 256, (frames, 18), dtype=torch.uint8, device=dev, generator=g)
                    row[:, 0] &= 0x0F
                    row[torch.rand(frames, device=dev, generator=g) < 0.01] = 0
                    self.audio[at:at + frames * 18] = row.reshape(-1)
            self.scratch = z(t.audio_bytes, torch.uint8)               # the per-file route's encrypted copy of the rows
            self.images = [z(t.image_bytes, torch.uint8) for _ in range(3)]   # [0] keyed, [1] other routes, [2] unkeyed / copy
            self.infos = []
            for f, lay in zip(self.files, self.lay):
                i = _lib.AdxFileInfoC()
                i.header_size, i.frame_size, i.channel_count, i.sample_count, i.version = lay.header_size, 18, nch, lay.sample_count, 4
                i.audio_offset, i.samples_per_frame, i.frame_count, i.audio_bytes = lay.audio_offset, 32, lay.frame_count, lay.frame_count * 18
                i.revision = TYPE
                self.infos.append(i)
            self.r = AdxFileSet.from_infos(self.infos, [int(o) for o in s.image_offsets])
            assert list(self.r.audio_offsets) == list(s.audio_offsets) and self.r.totals.audio_bytes == t.audio_bytes
            self.rows = [z(t.audio_bytes, torch.uint8) for _ in range(2)]
            self.workspace = torch.empty(max(self.r.find_keys_workspace_bytes(NKEYS8, NKEYS9), 16), dtype=torch.uint8, device=dev)
            self.index = [torch.full((s.files,), -9, dtype=torch.int32, device=dev) for _ in range(2)]

        # ---- write
        def keyed(self, out=0):
            self.s.write_keyed_device(self.audio, self.images[out], d_right, history=self.hist)

        def keyed_general(self):
            with forced():
                self.keyed(1)

        def unkeyed(self):
            self.s.write_device(self.audio, self.images[2], history=self.hist)

        def unkeyed_general(self):
            with forced():
                self.unkeyed()

        def crypt_per_file(self, buf):
            s = self.s
            for f, lay in enumerate(self.lay):
                c, n = int(s.first_channel[f]), lay.frame_count * 18
                if n:
                    check(L.vga_adx_crypt_device(buf.data_ptr() + int(s.audio_offsets[c]), up(n, 16), n, self.nch, C.byref(right_c), TYPE, 18, S))

        def per_file(self):
            """what existed before: encrypt a copy of the rows file by file, then the unkeyed set call"""
            self.scratch.copy_(self.audio)
            self.crypt_per_file(self.scratch)
            self.s.write_device(self.scratch, self.images[1], history=self.hist)

        # ---- read
        def read_keyed(self, out=0):
            self.r.read_keyed_device(self.images[0], self.rows[out], d_right)

        def read_keyed_general(self):
            with forced():
                self.read_keyed(1)

        def read_unkeyed(self):
            self.r.read_device(self.images[0], self.rows[1])

        def read_unkeyed_general(self):
            with forced():
                self.read_unkeyed()

        def read_per_file(self):
            self.r.read_device(self.images[0], self.rows[1])
            self.crypt_per_file(self.rows[1])

        # ---- find
        def find(self, keys=None, out=0):
            keys = d_last if keys is None else keys
            check(L.vga_adx_find_keys_device_v(self.r._h, self.images[0].data_ptr(), keys.data_ptr(), NKEYS8, NKEYS9, self.index[out].data_ptr(),
                                               self.workspace.data_ptr(), self.workspace.numel(), S))

        def find_first(self):
            self.find(d_first, 1)

        def find_per_file(self):
            """one vga_adx_find_key_device per file over the rows of the unkeyed read (each returns a host value)"""
            r, got = self.r, []
            for f, i in enumerate(self.infos):
                c, idx = int(r.first_channel[f]), C.c_int(-9)
                check(L.vga_adx_find_key_device(self.rows[1].data_ptr() + int(r.audio_offsets[c]), up(max(i.audio_bytes, 1), 16), i.audio_bytes, self.nch,
                                                TYPE, 18, host_last, NKEYS8, C.byref(idx), S))
                got.append(idx.value)
            return got

        def copy(self):
            check(0 if memcpy(self.images[2].data_ptr(), self.images[0].data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def say(self, what, **same):
            torch.cuda.synchronize()
            print(json.dumps({"tool": TOOL, "set": what, "equal": same}), flush=True)
            if not all(same.values()):
                raise SystemExit("the routes disagree")

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    def run(which, st):
        t = st.s.totals
        # ---- the bytes of every route, before anything is timed
        st.keyed()
        st.unkeyed()
        st.keyed_general()
        st.say(which + ": write general", images=bool(torch.equal(st.images[0], st.images[1])),
               keyed_differs_from_unkeyed=not torch.equal(st.images[0], st.images[2]))
        st.read_keyed()
        st.say(which + ": write then read", rows_are_the_input=bool(torch.equal(st.rows[0], st.audio)))
        st.read_keyed_general()
        st.say(which + ": read general", rows=bool(torch.equal(st.rows[0], st.rows[1])))
        st.find()
        st.find_first()
        st.say(which + ": find", right_key_last=bool((st.index[0] == NKEYS8 - 1).all()), right_key_first=bool((st.index[1] == 0).all()))
        if st.both:
            st.images[1].zero_()
            st.per_file()
            st.say(which + ": write per_file", images=bool(torch.equal(st.images[0], st.images[1])))
            st.read_per_file()
            st.say(which + ": read per_file", rows=bool(torch.equal(st.rows[0], st.rows[1])))
            st.read_unkeyed()
            torch.cuda.synchronize()
            st.say(which + ": find per_file", indices=st.find_per_file() == st.index[0].cpu().tolist())
        # ---- times
        tk, tu, tc = timed([st.keyed, st.unkeyed, st.copy])
        line("write keyed", which, tk, t.image_bytes, st, ratio_to_unkeyed=ratio(tk, tu), unkeyed_spread=tu["spread"])
        line("write unkeyed", which, tu, t.image_bytes, st)
        line("hipMemcpyAsync", which, tc, t.image_bytes, st)
        tk, tu = timed([st.read_keyed, st.read_unkeyed])
        line("read keyed", which, tk, t.image_bytes, st, ratio_to_unkeyed=ratio(tk, tu), unkeyed_spread=tu["spread"])
        line("read unkeyed", which, tu, t.image_bytes, st)
        tk, tu, rk, ru = timed([st.keyed_general, st.unkeyed_general, st.read_keyed_general, st.read_unkeyed_general])
        line("write keyed general", which, tk, t.image_bytes, st, ratio_to_unkeyed=ratio(tk, tu), unkeyed_spread=tu["spread"])
        line("write unkeyed general", which, tu, t.image_bytes, st)
        line("read keyed general", which, rk, t.image_bytes, st, ratio_to_unkeyed=ratio(rk, ru), unkeyed_spread=ru["spread"])
        line("read unkeyed general", which, ru, t.image_bytes, st)
        st.keyed()                                                     # (images[0] keyed again for the search)
        tl, tf, tc = timed([st.find, st.find_first, st.copy])
        line("find right key last", which, tl, t.image_bytes, st, ratio_to_copy=ratio(tl, tc), ratio_to_right_key_first=ratio(tl, tf))
        line("find right key first", which, tf, t.image_bytes, st, ratio_to_copy=ratio(tf, tc))
        if st.both:
            tk, tp = timed([st.keyed, st.per_file])
            line("write keyed (subset)", which, tk, t.image_bytes, st)
            line("write per_file", which, tp, t.image_bytes, st, ratio_to_keyed=ratio(tp, tk))
            tk, tp = timed([st.read_keyed, st.read_per_file])
            line("read keyed (subset)", which, tk, t.image_bytes, st)
            line("read per_file", which, tp, t.image_bytes, st, ratio_to_keyed=ratio(tp, tk))
            st.read_unkeyed()
            tk, tp = timed([st.find, st.find_per_file])
            line("find (subset)", which, tk, t.image_bytes, st)
            line("find per_file", which, tp, t.image_bytes, st, ratio_to_set=ratio(tp, tk))

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    for nch in [int(c) for c in a.channels.split(",")]:
        for which, picks, both in (("subset", pick, True), ("whole", list(range(nfiles)), False)):
            st = Set(picks, nch, both)
            which = "%s x%d" % (which, nch)
            print(json.dumps({"tool": TOOL, "set": which, "files": st.s.files, "channels": st.s.channels, "image_bytes": st.s.totals.image_bytes,
                              "audio_bytes": st.s.totals.audio_bytes, "candidates": [NKEYS8, NKEYS9], "write_stats": st.s.stats(),
                              "read_stats": st.r.stats()}), flush=True)
            run(which, st)
            st.close()
            del st
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
