#!/usr/bin/env python3
"""GPU time of the packed HCA calls (vga_hca_decode_device_v / vga_hca_encode_device_v) on streams of log-uniform lengths.

    python tools/time_hca_ragged_device.py [--set mixed|64] [--channels 1] [--quality 2] [--calls 10] [--warmup 3]
    VGAUDIO_HIP_LIBRARY=/path/to/another/libvgaudio_hip.so python tools/time_hca_ragged_device.py ...   # another build

--set mixed: the lengths of bench.py's mixed_lengths block (seed 0xBA7C4, 1-120 s log-uniform, as many as hold 4096 x 60 s:
10 008 streams); --set 64: 64 streams of 1-30 s.  One HCA shape class (48 kHz, --channels, --quality).  Three things are
timed per direction with HIP events around the calls on one stream, medians of --calls repeats after --warmup:
  packed      one *_device_v call on the packed buffers;
  equal       one vga_hca_*_device call on as many streams of equal length with the same total number of frames;
  per_stream  one vga_hca_*_device call per stream, on the packed buffers (a stream's rows are a batch of one).
A library without the packed calls (a build from before them) prints the equal and per_stream lines only.  One JSON line
per (direction, form)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vgaudio_amd import _lib  # noqa: E402


def lengths(which):
    if which == "64":
        rng = np.random.default_rng(64)
        return [int(np.exp(rng.uniform(np.log(48000.0), np.log(30 * 48000.0)))) for _ in range(64)]
    rng = np.random.default_rng(0xBA7C4)
    lens, total = [], 0
    while total < 4096 * 2_880_000:
        lens.append(int(np.exp(rng.uniform(np.log(48000.0), np.log(120 * 48000.0)))))
        total += lens[-1]
    return lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="64", choices=["mixed", "64"])
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--quality", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-stream-limit", type=int, default=0, help="time only the first N streams one by one and scale (0 = all)")
    a = ap.parse_args()
    import torch
    _lib._preload_torch_hip_runtime()
    L = C.CDLL(_lib.SO_PATH)
    have_packed = hasattr(L, "vga_hca_decode_device_v")
    names = ["vga_hca_encoder_initialize", "vga_hca_decode_workspace_bytes", "vga_hca_encode_device", "vga_hca_decode_device", "vga_last_error"]
    if have_packed:
        names += [n for n in _lib.SIGNATURES if "hca_ragged" in n and "testing" not in n] + ["vga_hca_decode_device_v", "vga_hca_encode_device_v"]
    for n in names:
        getattr(L, n).restype, getattr(L, n).argtypes = _lib.SIGNATURES[n]

    def check(rc):
        if rc:
            raise SystemExit("error %d: %s" % (rc, L.vga_last_error().decode()))

    nch, lens = a.channels, lengths(a.set)
    ns = len(lens)
    infos = (_lib.HcaInfoC * ns)()
    for s, n in enumerate(lens):
        p = _lib.HcaParamsC(a.quality, 0, 0, nch, 48000, n, 0, 0, 0)
        check(L.vga_hca_encoder_initialize(C.byref(p), C.byref(infos[s])))
    fs = infos[0].frame_size
    # the packed layout (computed here too, so that a library without the calls gets the same buffers)
    fo = np.zeros(ns, np.int64)
    ro = np.zeros(ns * nch, np.int64)
    fcur = pcur = 0
    for s in range(ns):
        fo[s] = fcur
        fcur += (infos[s].frame_count * fs + 3) // 4 * 4
        for c in range(nch):
            ro[s * nch + c] = pcur
            pcur += (lens[s] + 7) // 8 * 8
    frame_bytes, pcm_samples = fcur + 8, pcur
    total_frames = sum(h.frame_count for h in infos)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.arange(pcm_samples, device=dev, dtype=torch.float32)
    pcm = (8000 * torch.sin(t * 0.05) + 3000 * torch.sin(t * 0.0031)).to(torch.int16)
    pcm += torch.randint(-500, 500, (pcm_samples,), generator=g, device=dev, dtype=torch.int16)
    del t
    frames = torch.zeros(frame_bytes, dtype=torch.uint8, device=dev)
    out = torch.zeros(pcm_samples, dtype=torch.int16, device=dev)
    wsb = L.vga_hca_decode_workspace_bytes(C.byref(infos[0]), 1) // max(infos[0].frame_count, 1) * total_frames
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device=dev)
    status = torch.zeros(ns, dtype=torch.int32, device=dev)
    S = torch.cuda.current_stream().cuda_stream

    def timed(call, scale=1.0):
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
            ms.append(e0.elapsed_time(e1) * scale)
        return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    def line(direction, form, t, frames_done):
        print(json.dumps({"tool": "time_hca_ragged_device", "library": _lib.SO_PATH, "set": a.set, "streams": ns, "channels": nch,
                          "quality": a.quality, "direction": direction, "form": form, "frames": int(frames_done), **t,
                          "frames_per_ms": round(frames_done / t["median_ms"], 1)}), flush=True)

    def per_stream(direction, count):
        for s in range(count):
            h, n = infos[s], lens[s]
            cp = (n + 7) // 8 * 8
            room = frame_bytes - int(fo[s])
            if direction == "encode":
                check(L.vga_hca_encode_device(pcm.data_ptr() + 2 * int(ro[s * nch]), cp * nch, cp, 1, n, C.byref(h),
                                              frames.data_ptr() + int(fo[s]), room, status.data_ptr(), S))
            else:
                check(L.vga_hca_decode_device(C.byref(h), frames.data_ptr() + int(fo[s]), room, 1, out.data_ptr() + 2 * int(ro[s * nch]),
                                              cp * nch, cp, ws.data_ptr(), ws.numel(), status.data_ptr(), S))

    # equal length: as many streams, the same total number of frames
    eq_frames = max(1, round(total_frames / ns))
    eq_n = eq_frames * 1024 - 128
    ep = _lib.HcaParamsC(a.quality, 0, 0, nch, 48000, eq_n, 0, 0, 0)
    eh = _lib.HcaInfoC()
    check(L.vga_hca_encoder_initialize(C.byref(ep), C.byref(eh)))
    assert eh.frame_count == eq_frames
    e_cp = (eq_n + 7) // 8 * 8
    e_fp = (eq_frames * fs + 8 + 15) // 16 * 16
    e_pcm = pcm[:ns * nch * e_cp] if pcm_samples >= ns * nch * e_cp else pcm.repeat(2)[:ns * nch * e_cp]
    e_frames = torch.zeros(ns * e_fp, dtype=torch.uint8, device=dev)
    e_out = torch.zeros(ns * nch * e_cp, dtype=torch.int16, device=dev)
    e_ws = torch.empty(max(L.vga_hca_decode_workspace_bytes(C.byref(eh), ns), 16), dtype=torch.uint8, device=dev)

    if have_packed:
        r = C.c_void_p()
        check(L.vga_hca_ragged_create(infos, ns, C.byref(r)))
    limit = a.per_stream_limit if 0 < a.per_stream_limit < ns else ns
    lim_frames = sum(infos[s].frame_count for s in range(limit))
    for direction in ("encode", "decode"):                           # (the decoders read what the encoders wrote)
        if have_packed:
            if direction == "encode":
                call = lambda: check(L.vga_hca_encode_device_v(r, pcm.data_ptr(), frames.data_ptr(), status.data_ptr(), S))  # noqa: E731
            else:
                call = lambda: check(L.vga_hca_decode_device_v(r, frames.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), status.data_ptr(), S))  # noqa: E731
            line(direction, "packed", timed(call), total_frames)
        else:
            per_stream("encode", ns)                                  # the frames the decoders below read
        if direction == "encode":
            call = lambda: check(L.vga_hca_encode_device(e_pcm.data_ptr(), e_cp * nch, e_cp, ns, eq_n, C.byref(eh), e_frames.data_ptr(), e_fp,  # noqa: E731
                                                         status.data_ptr(), S))
        else:
            call = lambda: check(L.vga_hca_decode_device(C.byref(eh), e_frames.data_ptr(), e_fp, ns, e_out.data_ptr(), e_cp * nch, e_cp,  # noqa: E731
                                                         e_ws.data_ptr(), e_ws.numel(), status.data_ptr(), S))
        line(direction, "equal", timed(call), eq_frames * ns)
        line(direction, "per_stream", timed(lambda: per_stream(direction, limit)), lim_frames)
    torch.cuda.synchronize()
    if have_packed:
        bad = int((status != 0).sum().item())
        L.vga_hca_ragged_destroy(r)
        if bad:
            raise SystemExit("%d streams reported status bits" % bad)


if __name__ == "__main__":
    main()
