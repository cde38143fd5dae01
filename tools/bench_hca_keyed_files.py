#!/usr/bin/env python3
"""GPU time of the keyed calls on sets of HCA files (vga_hca_find_keys_device_v / vga_hca_read_keyed_device_v;
include/vgaudio_hip_files/hca_keyed_files.h) on the file set of bench.py's ragged block: 10 008 files of 1-120 s at 48 kHz
(seed 0xBA7C4) as stereo streams of one shape class (quality High, 682-byte frames), written as type-56 images by
vga_hca_write_device_v under five keys.  The candidates are as many made-up key codes as CriHcaEncryptionKeys.cs lists (40),
the five true keys at seeded positions among them; every file's key is one of the five, picked by a seeded draw.

    python tools/bench_hca_keyed_files.py [--calls 10] [--warmup 2] [--files N] [--subset 1000]

WHAT THE FRAMES ARE.  The search reads the first ten non-empty frames of a file and nothing else, and the read only moves,
substitutes and CRCs bytes.  So the first --head-frames frames of every stream are encoded by vga_hca_encode_device_v from
seeded noise made on the device, and the rest of the stream repeats them: every frame of every image is a frame the encoder
wrote, with a valid CRC, without encoding 47 GB of PCM for a measurement that never looks at it.

Device events around the calls on one stream, means, medians and the spread of --calls repeats after a warm-up, one process; the
calls of one line group are timed alternating, repeat by repeat:
  find      the search over the whole set, against a hipMemcpyAsync of the images;
  read      the keyed read with the search's index tensor, vga_hca_read_device_v on a set created with the same keys (the same
            kernel body), and the copy;
  per_file  on the seeded --subset only: one vga_hca_find_key_device per file (host clock: the call synchronises), against
            the set search on a set of the same files.
The answers of all routes are compared before anything is timed.  One JSON line per measurement; the log belongs in
profiles/hca_keyed_files_device.log."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402
from vgaudio_amd.crihca import CriHcaKey, RaggedHca  # noqa: E402
from vgaudio_amd.hca import HcaFileSet  # noqa: E402
from tools.time_hca_files import bench_lengths, hip_memcpy_async, info_for  # noqa: E402

NCANDIDATES, NTRUE = 40, 5
TOOL = "bench_hca_keyed_files"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=0, help="only the first N files of the set (0 = all)")
    ap.add_argument("--subset", type=int, default=1000, help="files of the seeded subset the per-file route runs on")
    ap.add_argument("--head-frames", type=int, default=16)
    a = ap.parse_args()
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    n = len(lens)
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    memcpy = hip_memcpy_async()
    rng = np.random.default_rng(0x4CA56)
    keys = [CriHcaKey(int(c)) for c in rng.integers(1, 2 ** 56, NCANDIDATES)]
    true_at = sorted(int(p) for p in rng.choice(NCANDIDATES, NTRUE, replace=False))
    key_of = [true_at[int(k)] for k in rng.integers(0, NTRUE, n)]       # per file: index into the candidates
    dec = np.ascontiguousarray(np.stack([k.DecryptionTable for k in keys]), dtype=np.uint8)
    enc = np.ascontiguousarray(np.stack([k.EncryptionTable for k in keys]), dtype=np.uint8)
    d_tables = torch.from_numpy(dec.reshape(-1).copy()).to(dev)

    def timed(calls):
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

    def line(what, t, **more):
        print(json.dumps({"tool": TOOL, "what": what, **t, **more}), flush=True)

    # ---- the frames: encoded heads, repeated
    infos = [info_for(s) for s in lens]
    head_samples = a.head_frames * 1024 - 1024
    head = info_for(head_samples)
    fs, hc = head.frame_size, head.frame_count
    assert all(h.frame_size == fs and h.frame_count >= hc for h in infos)
    r = RaggedHca([head] * n)
    g = torch.Generator(device=dev)
    g.manual_seed(0x17)
    pcm = torch.randint(-6000, 6000, (max(r.totals.pcm_samples, 16),), dtype=torch.int16, device=dev, generator=g)
    heads = torch.zeros(r.totals.frame_bytes, dtype=torch.uint8, device=dev)
    estatus = torch.zeros(n, dtype=torch.int32, device=dev)
    r.encode_device(pcm, heads, estatus)
    torch.cuda.synchronize()
    assert not estatus.cpu().numpy().any()
    w = HcaFileSet([_lib.HcaFileC(h, None, 1.0, 56, 1, key_of[f]) for f, h in enumerate(infos)], tables=enc)
    t = w.totals
    frames = torch.zeros(t.frame_bytes, dtype=torch.uint8, device=dev)
    for f, h in enumerate(infos):
        src = heads[int(r.frame_offsets[f]):int(r.frame_offsets[f]) + hc * fs]
        at, nb = int(w.frame_offsets[f]), h.frame_count * fs
        frames[at:at + nb] = src.repeat((h.frame_count + hc - 1) // hc)[:nb]
    del pcm, heads
    r.close()
    images = torch.zeros(t.image_bytes, dtype=torch.uint8, device=dev)
    w.write_device(frames, images)
    torch.cuda.synchronize()
    fi = []
    for h in infos:
        i = _lib.HcaFileInfoC()
        i.hca, i.frames_offset, i.volume, i.encryption_type = h, h.header_size, 1.0, 56
        fi.append(i)
    io = [int(o) for o in w.image_offsets]
    s = HcaFileSet.from_infos(fi, image_offsets=io)
    own = HcaFileSet.from_infos(fi, image_offsets=io, keys=key_of, tables=dec)
    back, ref = (torch.zeros(s.totals.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(2))
    copy = torch.empty_like(images)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    need = s.find_keys_workspace_bytes(NCANDIDATES)
    workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)

    def find(which=s, out=index, st=status, ws=workspace):
        check(L.vga_hca_find_keys_device_v(which._h, images.data_ptr(), d_tables.data_ptr(), NCANDIDATES, -1, out.data_ptr(), st.data_ptr(),
                                           ws.data_ptr(), ws.numel(), S))

    def read_keyed():
        check(L.vga_hca_read_keyed_device_v(s._h, images.data_ptr(), d_tables.data_ptr(), NCANDIDATES, index.data_ptr(), back.data_ptr(), None,
                                            None, S))

    def read_own():
        check(L.vga_hca_read_device_v(own._h, images.data_ptr(), ref.data_ptr(), None, S))

    def copy_images():
        assert memcpy(copy.data_ptr(), images.data_ptr(), images.numel(), 3, S) == 0

    # ---- the routes agree before anything is timed
    find()
    read_keyed()
    read_own()
    torch.cuda.synchronize()
    assert index.cpu().numpy().tolist() == key_of and not status.cpu().numpy().any()
    assert torch.equal(back, ref) and torch.equal(back[:frames.numel() - 8], frames[:frames.numel() - 8])
    shape = {"files": n, "candidates": NCANDIDATES, "frame_size": fs, "image_bytes": int(t.image_bytes), "total_frames": int(t.total_frames)}
    tf, tc = timed([find, copy_images])
    line("find", tf, **shape, ratio_to_copy=round(tf["mean_ms"] / tc["mean_ms"], 3))
    line("copy_images", tc, **shape, gb_per_s=round(2 * t.image_bytes / tc["mean_ms"] / 1e6, 1))
    tk, to, tc = timed([read_keyed, read_own, copy_images])
    line("read_keyed", tk, **shape, ratio_to_create_time_keys=round(tk["mean_ms"] / to["mean_ms"], 3),
         gb_per_s=round(2 * t.image_bytes / tk["mean_ms"] / 1e6, 1))
    line("read_create_time_keys", to, **shape, gb_per_s=round(2 * t.image_bytes / to["mean_ms"] / 1e6, 1))
    line("copy_images", tc, **shape, gb_per_s=round(2 * t.image_bytes / tc["mean_ms"] / 1e6, 1))

    # ---- the seeded subset: one per-file call per file against the set search on the same files
    picks = sorted(int(p) for p in np.random.default_rng(0x5B5E7).choice(n, min(a.subset, n), replace=False))
    sub = HcaFileSet.from_infos([fi[p] for p in picks], image_offsets=[io[p] for p in picks])
    sub_index, sub_status = (torch.empty(len(picks), dtype=torch.int32, device=dev) for _ in range(2))
    sub_ws = torch.empty(max(sub.find_keys_workspace_bytes(NCANDIDATES), 16), dtype=torch.uint8, device=dev)
    found = np.zeros(len(picks), np.int32)
    u8p = C.POINTER(C.c_uint8)

    def per_file():
        for k, p in enumerate(picks):
            h, idx = infos[p], C.c_int(-1)
            check(L.vga_hca_find_key_device(C.byref(h), images.data_ptr() + io[p] + h.header_size, h.frame_count, dec.ctypes.data_as(u8p),
                                            NCANDIDATES, C.byref(idx), S))
            found[k] = idx.value

    find(sub, sub_index, sub_status, sub_ws)
    per_file()
    torch.cuda.synchronize()
    assert found.tolist() == [key_of[p] for p in picks] == sub_index.cpu().numpy().tolist()
    (ts,) = timed([lambda: find(sub, sub_index, sub_status, sub_ws)])
    for _ in range(min(a.warmup, 1)):
        per_file()
    wall = []
    for _ in range(a.calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per_file()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    tp = {"mean_ms": round(float(np.mean(wall)), 3), "median_ms": round(float(np.median(wall)), 3), "min_ms": round(min(wall), 3),
          "max_ms": round(max(wall), 3), "spread": round((max(wall) - min(wall)) / float(np.median(wall)), 3)}
    line("subset_find", ts, files=len(picks), candidates=NCANDIDATES)
    line("subset_per_file_find_key_device", tp, files=len(picks), candidates=NCANDIDATES, clock="host",
         ratio_to_set=round(tp["mean_ms"] / ts["mean_ms"], 1))
    for x in (w, s, own, sub):
        x.close()


if __name__ == "__main__":
    main()
