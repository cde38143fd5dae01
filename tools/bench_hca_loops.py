#!/usr/bin/env python3
"""GPU time of the packed HCA encode with looping streams (vga_hca_encode_loops_device_v;
include/vgaudio_hip_files/hca_ragged_loops.h) on the file set of bench.py's ragged block: 10 008 lengths of 1-120 s at 48 kHz
(seed 0xBA7C4) as stereo streams of one shape class (quality High).  In the LOOPING set every stream loops from a seeded start
in its first half to its end; the PLAIN set has the same lengths without loops, so both sets share one packed PCM buffer.

    python tools/bench_hca_loops.py [--calls 10] [--warmup 2] [--files N] [--subset 1000] [--parent-library PATH] [--log PATH]

Device events around the calls on one stream, means, medians and the spread of --calls repeats after a warm-up, one process; the
calls of one line group are timed alternating, repeat by repeat:
  set       encode_loops_device on the looping set next to encode_device on the plain set.  The looping set has more frames (a
            looping stream leads in with up to 1151 more samples and ends with 256 to 383 of post audio), so both are also
            reported per frame;
  per_file  on the seeded --subset of the looping set only: one vga_hca_encode_device call per file -- the route a looping
            file took before -- next to encode_loops_device on an object of the same files;
  parent    with --parent-library (a build of the parent commit: the same ABI without the new call): vga_hca_encode_device_v
            on the plain set through both builds, loaded side by side in this process.  The difference of the means stands
            beside the spread of the repeats; a difference inside that spread is no change.
The answers are compared before anything is timed: the subset's packed frames against the per-file calls', the plain set's
frames from both calls and both builds.  One JSON line per measurement, on stdout and appended to --log (default
profiles/hca_ragged_loops_device.log).  --files 300 is a quick trial."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402
from vgaudio_amd.crihca import RaggedHca  # noqa: E402
from tools.time_hca_files import bench_lengths  # noqa: E402

TOOL = "bench_hca_loops"


def info_for(samples, loop_start=None):
    p, h = _lib.HcaParamsC(2, 0, 0, 2, 48000, samples, 0, 0, 0), _lib.HcaInfoC()
    if loop_start is not None:
        p.looping, p.loop_start, p.loop_end = 1, loop_start, samples
    _lib.check(_lib.lib().vga_hca_encoder_initialize(C.byref(p), C.byref(h)))
    return h


def fill_pcm(pcm, torch):
    """seeded tones and noise, made on the device in pieces (no temporary as large as the buffer)"""
    g = torch.Generator(device=pcm.device).manual_seed(1)
    step = 1 << 26
    for at in range(0, pcm.numel(), step):
        n = min(step, pcm.numel() - at)
        t = torch.arange(at % (1 << 20), at % (1 << 20) + n, device=pcm.device, dtype=torch.float32)
        piece = (8000 * torch.sin(t * 0.05) + 3000 * torch.sin(t * 0.0031)).to(torch.int16)
        piece += torch.randint(-500, 500, (n,), generator=g, device=pcm.device, dtype=torch.int16)
        pcm[at:at + n] = piece


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--files", type=int, default=0, help="only the first N lengths of the set (0 = all)")
    ap.add_argument("--subset", type=int, default=1000, help="files of the seeded subset the per-file route runs on")
    ap.add_argument("--parent-library", default="", help="libvgaudio_hip.so of the parent commit, for the plain path's comparison")
    ap.add_argument("--parent-commit", default="", help="the commit --parent-library was built from (default: git's HEAD)")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "hca_ragged_loops_device.log"))
    a = ap.parse_args()
    import torch
    L, check = _lib.lib(), _lib.check
    dev = torch.device("cuda")
    lens = bench_lengths()
    if a.files:
        lens = lens[:a.files]
    ns = len(lens)
    rng = np.random.default_rng(0x100B5)
    starts = [int(rng.integers(0, n // 2)) for n in lens]
    loop_infos = [info_for(n, s) for n, s in zip(lens, starts)]
    plain_infos = [info_for(n) for n in lens]
    assert all(h.sample_count == n and h.looping for h, n in zip(loop_infos, lens))
    S = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    commit = a.parent_commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""

    def emit(**kw):
        text = json.dumps({"tool": TOOL, "library": os.path.basename(os.path.dirname(_lib.SO_PATH)) + "/" + os.path.basename(_lib.SO_PATH),
                           "parent_commit": commit or "not recorded", "device": torch.cuda.get_device_name(0), "streams": ns, **kw})
        print(text, flush=True)
        if a.log:
            with open(a.log, "a") as f:
                f.write(text + "\n")

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
                 "max_ms": round(max(m), 3)} for m in ms]

    loops, plain = RaggedHca(loop_infos), RaggedHca(plain_infos)
    assert np.array_equal(loops.pcm_row_offsets, plain.pcm_row_offsets)
    pcm = torch.empty(max(loops.totals.pcm_samples, 8), dtype=torch.int16, device=dev)
    fill_pcm(pcm, torch)
    f_loops = torch.zeros(loops.totals.frame_bytes, dtype=torch.uint8, device=dev)
    f_plain = torch.zeros(plain.totals.frame_bytes, dtype=torch.uint8, device=dev)
    f_other = torch.zeros(plain.totals.frame_bytes, dtype=torch.uint8, device=dev)
    st = torch.zeros(ns, dtype=torch.int32, device=dev)

    # ---- the answers first
    loops.encode_loops_device(pcm, f_loops, st)
    plain.encode_device(pcm, f_plain, st)
    plain.encode_loops_device(pcm, f_other, st)
    torch.cuda.synchronize()
    assert torch.equal(f_plain, f_other), "plain streams: the two calls wrote different frames"
    assert not int((st != 0).sum().item()), "status bits"
    sub = sorted(int(i) for i in np.random.default_rng(0x5AB5E7).choice(ns, min(a.subset, ns), replace=False))
    sub_obj = RaggedHca([loop_infos[i] for i in sub])
    sub_pcm = torch.empty(max(sub_obj.totals.pcm_samples, 8), dtype=torch.int16, device=dev)
    for k, i in enumerate(sub):
        for c in range(2):
            at, src, n = int(sub_obj.pcm_row_offsets[2 * k + c]), int(loops.pcm_row_offsets[2 * i + c]), lens[i]
            sub_pcm[at:at + n] = pcm[src:src + n]
    f_sub = torch.zeros(sub_obj.totals.frame_bytes, dtype=torch.uint8, device=dev)
    f_file = torch.zeros(sub_obj.totals.frame_bytes, dtype=torch.uint8, device=dev)
    st_sub = torch.zeros(len(sub), dtype=torch.int32, device=dev)

    def per_file():
        for k, i in enumerate(sub):
            h, n = loop_infos[i], lens[i]
            cp = (n + 7) // 8 * 8
            at = int(sub_obj.frame_offsets[k])
            check(L.vga_hca_encode_device(sub_pcm.data_ptr() + 2 * int(sub_obj.pcm_row_offsets[2 * k]), 2 * cp, cp, 1, n, C.byref(h),
                                          f_file.data_ptr() + at, (sub_obj.totals.frame_bytes - at) // 2 * 2, st_sub.data_ptr() + 4 * k, S))

    sub_obj.encode_loops_device(sub_pcm, f_sub, st_sub)
    per_file()
    torch.cuda.synchronize()
    assert torch.equal(f_sub[:-8], f_file[:-8]), "looping subset: the packed call and the per-file calls wrote different frames"
    first = loop_infos[sub[0]].frame_count * loop_infos[sub[0]].frame_size
    assert torch.equal(f_sub[:first], f_loops[int(loops.frame_offsets[sub[0]]):][:first]), "the subset's first stream differs from the set's"
    emit(measurement="answers", subset=len(sub), equal=True)

    # ---- the set
    lf, pf = loops.totals.total_frames, plain.totals.total_frames
    t_loops, t_plain = timed([lambda: loops.encode_loops_device(pcm, f_loops, st), lambda: plain.encode_device(pcm, f_plain, st)])
    emit(measurement="set", call="encode_loops_device", looping=True, frames=lf, ns_per_frame=round(t_loops["mean_ms"] * 1e6 / lf, 2), **t_loops)
    emit(measurement="set", call="encode_device", looping=False, frames=pf, ns_per_frame=round(t_plain["mean_ms"] * 1e6 / pf, 2), **t_plain)

    # ---- the per-file route, on the subset
    sf = sub_obj.totals.total_frames
    t_file, t_sub = timed([per_file, lambda: sub_obj.encode_loops_device(sub_pcm, f_sub, st_sub)])
    emit(measurement="per_file", call="vga_hca_encode_device per file", files=len(sub), frames=sf, **t_file)
    emit(measurement="per_file", call="encode_loops_device", files=len(sub), frames=sf, **t_sub)

    # ---- the plain path against the parent's build
    if a.parent_library:
        P = C.CDLL(a.parent_library)
        for name in ("vga_hca_ragged_create", "vga_hca_ragged_destroy", "vga_hca_encode_device_v", "vga_last_error"):
            getattr(P, name).restype, getattr(P, name).argtypes = _lib.SIGNATURES[name]
        assert not hasattr(P, "vga_hca_encode_loops_device_v"), "--parent-library has the new call: not the parent's build"
        arr = (_lib.HcaInfoC * ns)(*plain_infos)
        pr = C.c_void_p()
        rc = P.vga_hca_ragged_create(arr, ns, C.byref(pr))
        assert rc == 0, P.vga_last_error()

        def parent_call():
            rc = P.vga_hca_encode_device_v(pr, pcm.data_ptr(), f_other.data_ptr(), st.data_ptr(), S)
            assert rc == 0, P.vga_last_error()

        f_other.zero_()
        parent_call()
        torch.cuda.synchronize()
        assert torch.equal(f_plain, f_other), "plain streams: the parent's build wrote different frames"
        t_new, t_old = timed([lambda: plain.encode_device(pcm, f_plain, st), parent_call])
        emit(measurement="parent", call="vga_hca_encode_device_v", build="this", frames=pf, **t_new)
        emit(measurement="parent", call="vga_hca_encode_device_v", build="parent", frames=pf, **t_old)
        emit(measurement="parent", difference_of_means_ms=round(t_new["mean_ms"] - t_old["mean_ms"], 3),
             spread_this_ms=round(t_new["max_ms"] - t_new["min_ms"], 3), spread_parent_ms=round(t_old["max_ms"] - t_old["min_ms"], 3))
        P.vga_hca_ragged_destroy(pr)
    else:
        emit(measurement="parent", note="not measured (no --parent-library)")
    torch.cuda.synchronize()
    assert not int((st != 0).sum().item()) and not int((st_sub != 0).sum().item()), "status bits"
    for r in (loops, plain, sub_obj):
        r.close()


if __name__ == "__main__":
    main()
