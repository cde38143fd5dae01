#!/usr/bin/env python3
"""GPU time of the PCM NintendoWare file sets (vga_nwstm_pcm_write_device_v / vga_nwstm_pcm_read_device_v;
include/vgaudio_hip_files/nw_pcm_files.h) on the file set of bench.py's ragged block: 10 008 files of 1-120 s at 48 kHz (seed
0xBA7C4, log-uniform, as many as hold 4096 x 60 s), even files mono and odd files stereo, no loop, at the default
configuration, once as BRSTM PCM16 (swap16) and once as BFSTM PCM8.  Both calls only move samples, so the rows are seeded
random shorts made on the device (for PCM8 with a zero low byte, so that they come back unchanged).

    python tools/time_nw_pcm_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000] [--steps brstm_pcm16,bfstm_pcm8] [--log PATH]

Without --step this is the DRIVER: it starts one child process per step, each under its own `timeout`, one after the other
and only while the one before ended well, and writes what they print to profiles/nw_pcm_files_device.log.  A step, in one
process, with device events around the calls on one stream, means, medians and the spread of --calls repeats after a warm-up
of every shape:
  set       one vga_nwstm_pcm_write_device_v call over a seeded --subset of the files and over the whole set, then one
            vga_nwstm_pcm_read_device_v call over the images it wrote;
  general   the same calls under vga_nw_pcm_files_force_general_this_thread(1), on the subset;
  per_file  what a caller with device-resident files had before, on the subset: one vga_nwstm_pcm_write_device (one
            vga_nwstm_pcm_read_device) call per file on the same buffers; timed alternating with the set call;
  copy      hipMemcpyAsync device to device of the same image bytes, in the same run: the yardstick.  "ratio_to_copy" is
            the call's mean over the copy's; "ratio_per_byte" sets the bytes each of them reads and writes against each
            other (a PCM8 call moves three bytes per image byte, the copy two).  The ratios are reported, not gated.
The bytes of all routes are compared before anything is timed, and the whole set's rows must come back from its images
unchanged.  A whole set that does not fit the free device memory is cut to the files that do, and the line says so.  One
JSON line per (route, set)."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib, nwstm  # noqa: E402
from vgaudio_amd.nwstm import NwPcmFileSet  # noqa: E402

RATE = 48000
STEP_SECONDS = 420
STEPS = {"brstm_pcm16": (nwstm.NwTarget.Revolution, nwstm.NwCodec.Pcm16Bit), "bfstm_pcm8": (nwstm.NwTarget.Cafe, nwstm.NwCodec.Pcm8Bit)}
HEAD = """# python tools/time_nw_pcm_files.py (every step names its device; one process per step, device events, means and medians of {calls} calls after
# {warmup} warm-up calls of every shape; the routes of one table alternate repeat by repeat; the bytes of all routes are compared
# first; even files mono, odd files stereo, no loop, default configuration; "general": the same call with every file forced
# into the general form; "ratio_to_copy": the call's mean over hipMemcpyAsync's of the same image bytes; "ratio_per_byte":
# the same per byte read and written)
"""


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


def drive(a):
    """one child per step, each under its own time limit, stopping at the first that fails"""
    timeout = shutil.which("timeout")
    assert timeout, "timeout (coreutils) is needed"
    os.makedirs(os.path.dirname(a.log), exist_ok=True)
    with open(a.log, "w") as log:
        log.write(HEAD.format(calls=a.calls, warmup=a.warmup))
        log.flush()
        for name in a.steps.split(","):
            cmd = [timeout, "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(a.calls),
                   "--warmup", str(a.warmup), "--files", str(a.files), "--subset", str(a.subset)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            log.write(r.stdout)
            log.flush()
            if r.returncode != 0:                                      # nothing more is started on the device
                sys.stderr.write(r.stderr[-4000:])
                log.write("# step %s ended with status %d\n" % (name, r.returncode))
                return r.returncode
    return 0


def step(a, name):
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    target, codec = STEPS[name]
    bps = 2 if codec == nwstm.NwCodec.Pcm16Bit else 1
    configuration = nwstm.BxstmConfiguration(Codec=codec)
    cfg, _ = nwstm._pcm_file_config(target, configuration)
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    channels = lambda k: 1 + k % 2
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    tool = "time_nw_pcm_files"
    print(json.dumps({"tool": tool, "step": name, "device": torch.cuda.get_device_name()}), flush=True)

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

    def line(form, which, t, st, copy=None):
        nbytes = st.s.totals.image_bytes
        moved = nbytes * (1 + 2 // bps) if copy else 2 * nbytes        # an image byte and the row bytes behind it; the copy: two
        extra = {}
        if copy:
            extra = {"ratio_to_copy": round(t["mean_ms"] / copy["mean_ms"], 2),
                     "ratio_per_byte": round(t["mean_ms"] / moved / (copy["mean_ms"] / (2 * nbytes)), 2)}
        print(json.dumps({"tool": tool, "step": name, "set": which, "files": st.s.files, "form": form, "image_bytes": int(nbytes), **t,
                          "moved_gb_per_s": round(moved / t["mean_ms"] / 1e6, 1), **extra}), flush=True)

    class forced:
        def __enter__(self):
            L.vga_nw_pcm_files_force_general_this_thread(1)

        def __exit__(self, *exc):
            L.vga_nw_pcm_files_force_general_this_thread(0)

    class Set:
        """the files, their rows resident; three buffers: the rows, the images, and one more for the other routes, the copy and
        the rows read back"""

        def __init__(self, picks):
            self.files = [_lib.NwFileC(channels(k), RATE, lens[k], 0, 0, 0) for k in picks]
            self.s = NwPcmFileSet(self.files, target, configuration)
            s, t = self.s, self.s.totals
            g = torch.Generator(device=dev)
            g.manual_seed(0x17)
            self.pcm = torch.randint(-32768, 32768, (t.pcm_samples,), dtype=torch.int16, device=dev, generator=g)
            if bps == 1:
                self.pcm &= -256                                       # DecodeSigned(EncodeSigned(x)) == x
            # zeros where no row lies (the rounding gaps, the guard), so that the rows read back compare as one buffer
            n = np.concatenate([[f.sample_count] * f.channels for f in self.files]).astype(np.int64)
            ends, pad = s.pcm_offsets + n, (-n) % 8
            gaps = np.concatenate([np.arange(e, e + p) for e, p in zip(ends[pad > 0], pad[pad > 0])] + [np.arange(t.pcm_samples - 128, t.pcm_samples)])
            self.pcm[torch.from_numpy(gaps).to(dev)] = 0
            self.images = torch.zeros(t.image_bytes, dtype=torch.uint8, device=dev)
            self.other = torch.zeros(max(t.image_bytes, 2 * t.pcm_samples) + 16, dtype=torch.uint8, device=dev)
            self.params, self.infos = [], []
            for f in self.files:                                       # the infos from the layouts: no image is downloaded for them
                N = NwPcmFileSet.file_layout(f, cfg, int(codec))
                i = _lib.NwInfoC()
                i.target, i.endianness, i.version, i.codec, i.sample_rate = N.target, N.endianness, N.version, int(codec), RATE
                i.sample_count, i.channel_count, i.interleave_size, i.samples_per_interleave = N.sample_count, f.channels, N.interleave_size, N.samples_per_interleave
                i.audio_data_offset, i.audio_data_length, i.adpcm_bytes, i.file_size = N.audio_data_offset, N.audio_data_size * f.channels, N.sample_count * bps, N.file_size
                self.infos.append(i)
                self.params.append(NwPcmFileSet.file_params(f, cfg))
            self.r = NwPcmFileSet.from_infos(self.infos, None, [int(o) for o in s.image_offsets])
            assert list(self.r.pcm_offsets) == list(s.pcm_offsets) and self.r.totals.pcm_samples == t.pcm_samples

        def rows_back(self):
            return self.other[:2 * self.s.totals.pcm_samples].view(torch.int16)

        def write(self, images=None):
            self.s.write(self.pcm, self.images if images is None else images)

        def write_general(self):
            with forced():
                self.write(self.other[:self.s.totals.image_bytes])

        def pitch(self, s, f):
            c = int(s.first_channel[f])
            return c, (int(s.pcm_offsets[c + 1]) - int(s.pcm_offsets[c])) if self.files[f].channels > 1 else self.files[f].sample_count

        def write_per_file(self):
            s = self.s
            for f, file in enumerate(self.files):
                c, pitch = self.pitch(s, f)
                check(L.vga_nwstm_pcm_write_device(C.byref(self.params[f]), int(codec), file.channels, 1, None, self.pcm.data_ptr() + 2 * int(s.pcm_offsets[c]),
                                                   0, pitch, self.other.data_ptr() + int(s.image_offsets[f]), s.image_sizes[f], S))

        def read(self):
            self.r.read(self.images, self.rows_back())

        def read_general(self):
            with forced():
                self.read()

        def read_per_file(self):
            r = self.r
            for f, i in enumerate(self.infos):
                c, pitch = self.pitch(r, f)
                check(L.vga_nwstm_pcm_read_device(C.byref(i), self.images.data_ptr() + int(r.image_offsets[f]), r.image_sizes[f], 1,
                                                  self.other.data_ptr() + 2 * int(r.pcm_offsets[c]), 0, pitch, S))

        def copy(self):
            check(0 if memcpy(self.other.data_ptr(), self.images.data_ptr(), self.s.totals.image_bytes, 3, S) == 0 else _lib.VGA_ERR_DEVICE)

        def same(self, what, kind):
            """the other route's bytes against the set call's, then cleared for the next route"""
            torch.cuda.synchronize()
            if kind == "images":
                ok = bool(torch.equal(self.other[:self.images.numel()], self.images))
            else:
                ok = bool(torch.equal(self.rows_back(), self.pcm))
            print(json.dumps({"tool": tool, "step": name, "set": what, "equal": {kind: ok}}), flush=True)
            if not ok:
                raise SystemExit("the routes disagree: " + what)
            self.other.zero_()

        def check_infos(self, count=12):
            """the infos made from the layouts are what vga_nwstm_pcm_parse reads out of the images the set wrote"""
            order = sorted(range(len(self.files)), key=lambda f: self.s.image_sizes[f])[:count]
            for f in order:
                at = int(self.s.image_offsets[f])
                image = self.images[at:at + self.s.image_sizes[f]].cpu().numpy()
                got = nwstm.parse_pcm(image.tobytes())
                for k in ("target", "endianness", "codec", "sample_count", "channel_count", "interleave_size", "audio_data_offset",
                          "audio_data_length", "adpcm_bytes"):
                    assert getattr(got, k) == getattr(self.infos[f], k), (f, k)

        def close(self):
            torch.cuda.synchronize()
            self.s.close()
            self.r.close()

    def run(which, st, both):
        st.write()
        torch.cuda.synchronize()
        st.check_infos()
        print(json.dumps({"tool": tool, "step": name, "set": which, "files": st.s.files, "channels": st.s.channels, "image_bytes": st.s.totals.image_bytes,
                          "pcm_samples": st.s.totals.pcm_samples, "write_stats": st.s.stats(), "read_stats": st.r.stats()}), flush=True)
        st.read()                                                      # the bytes of every route, before anything is timed
        st.same(which + ": read set, rows against the source", "rows")
        if both:
            st.write_general()
            st.same(which + ": write general", "images")
            st.read_general()
            st.same(which + ": read general", "rows")
            st.write_per_file()
            st.same(which + ": write per_file", "images")
            st.read_per_file()
            st.same(which + ": read per_file", "rows")
        (tc,) = timed([st.copy])
        line("hipMemcpyAsync", which, tc, st)
        if both:
            tw, tg, tf = timed([st.write, st.write_general, st.write_per_file])
            line("write per_file", which, tf, st, tc)
            line("write general", which, tg, st, tc)
            line("write set", which, tw, st, tc)
            tr, tg, tf2 = timed([st.read, st.read_general, st.read_per_file])
            line("read per_file", which, tf2, st, tc)
            line("read general", which, tg, st, tc)
            line("read set", which, tr, st, tc)
        else:
            tw, tr = timed([st.write, st.read])
            line("write set", which, tw, st, tc)
            line("read set", which, tr, st, tc)

    nfiles = len(lens)
    pick = sorted(np.random.default_rng(0x5B5E7).choice(nfiles, min(a.subset, nfiles), replace=False).tolist())
    whole = list(range(nfiles))
    # the rows, the images and a buffer of the larger of the two: cut the whole set to what fits three quarters of the free memory
    free, _ = torch.cuda.mem_get_info()
    need = lambda picks: (4 + bps) * sum(channels(k) * lens[k] for k in picks) + 20000 * len(picks)
    cut = len(whole)
    while cut > 1 and need(whole[:cut]) > 0.75 * free:
        cut = cut * 3 // 4
    if cut < len(whole):
        print(json.dumps({"tool": tool, "step": name, "set": "whole", "cut_to_files": cut, "of": len(whole), "free_bytes": int(free)}), flush=True)
    for which, picks, both in (("subset", pick, True), ("whole", whole[:cut], False)):
        st = Set(picks)
        run(which, st, both)
        st.close()
        del st
        torch.cuda.empty_cache()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=0, help="only the first N files of the set (0 = all)")
    ap.add_argument("--subset", type=int, default=1000, help="files of the seeded subset the per-file route runs on")
    ap.add_argument("--steps", default=",".join(STEPS), help="the steps, one process each")
    ap.add_argument("--step", default="", help="run this step here (what the driver starts)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "nw_pcm_files_device.log"))
    a = ap.parse_args()
    assert a.calls >= 10 or a.files, "at least 10 repetitions"
    if a.step:
        return step(a, a.step)
    return drive(a)


if __name__ == "__main__":
    sys.exit(main())
