"""Times vga_nwwav_bank_read_device on a synthetic sound bank against what a caller had before it: one device-to-device
copy per channel into the same packed layout.

    python tools/bench_nwwav_bank.py [--files 8192] [--reps 30] [--out FILE]

The bank: --files wave files, 0.05 .. 5 s at 32 kHz (log-uniform, seeded), mono or stereo, 80 % GC-ADPCM and the rest
PCM16 (half of it big-endian), channel audio at arbitrary byte offsets.  The infos are filled in directly (the timing
does not depend on headers); the payload is random bytes.  Prints one JSON line: medians, spreads, bytes moved
(read + written) per second."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from vgaudio_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(2024)
    infos = (_lib.NwWavInfoC * a.files)()
    offsets = np.zeros(a.files, dtype=np.int64)
    at = 0
    src_of, bytes_of = [], []
    for f in range(a.files):
        I = infos[f]
        n = int(np.exp(rng.uniform(np.log(1600), np.log(160000))))
        gc = rng.random() < 0.8
        I.kind, I.codec, I.sample_count, I.channel_count = 2, 2 if gc else 1, n, int(rng.integers(1, 3))
        I.endianness = int(rng.integers(0, 2))
        I.channel_bytes = L.vga_gcadpcm_sample_count_to_byte_count(n) if gc else 2 * n
        offsets[f] = at
        pos = 0x80
        for c in range(I.channel_count):
            pos += int(rng.integers(0, 32))
            I.audio_offset[c] = pos
            src_of.append(at + pos)
            bytes_of.append(I.channel_bytes)
            pos += I.channel_bytes
        at += pos + int(rng.integers(0, 32))
    h = C.c_void_p()
    _lib.check(L.vga_nwwav_bank_create(infos, offsets.ctypes.data_as(C.POINTER(C.c_int64)), a.files, C.byref(h)))
    rows = L.vga_nwwav_bank_channels(h)
    codec, offs = np.zeros(rows, np.int32), np.zeros(rows, np.int64)
    _lib.check(L.vga_nwwav_bank_rows(h, None, None, codec.ctypes.data_as(C.POINTER(C.c_int)), None, offs.ctypes.data_as(C.POINTER(C.c_int64))))
    d_files = torch.randint(0, 256, (at,), dtype=torch.uint8, device="cuda")
    d_adpcm = torch.zeros(L.vga_nwwav_bank_adpcm_bytes(h), dtype=torch.uint8, device="cuda")
    d_pcm16 = torch.zeros(L.vga_nwwav_bank_pcm16_samples(h) * 2, dtype=torch.uint8, device="cuda")
    copy_out = [None, torch.zeros_like(d_pcm16), torch.zeros_like(d_adpcm)]
    stream = torch.cuda.current_stream().cuda_stream

    def bank_read():
        _lib.check(L.vga_nwwav_bank_read_device(h, d_files.data_ptr(), d_adpcm.data_ptr(), d_pcm16.data_ptr(), None, stream))

    views = [(copy_out[codec[r]][offs[r] * (2 if codec[r] == 1 else 1):][:bytes_of[r]], d_files[src_of[r]:src_of[r] + bytes_of[r]])
             for r in range(rows)]

    def copies():                                        # one device-to-device copy per channel (no byte swap, no padding)
        for dst, src in views:
            dst.copy_(src, non_blocking=True)

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        ms.sort()
        return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], p10_ms=ms[len(ms) // 10], p90_ms=ms[-1 - len(ms) // 10])

    audio = int(sum(bytes_of))
    res = dict(files=a.files, rows=rows, audio_bytes=audio, source_bytes=at, reps=a.reps, bank_read=timed(bank_read),
               copy_per_channel=timed(copies))
    res["bank_read"]["gbytes_per_s_read_plus_written"] = 2 * audio / res["bank_read"]["median_ms"] / 1e6
    res["copy_per_channel"]["gbytes_per_s_read_plus_written"] = 2 * audio / res["copy_per_channel"]["median_ms"] / 1e6
    le = [r for r in range(rows) if codec[r] == 2]        # same bytes where no swap is involved
    res["gc_rows_equal"] = bool(all(torch.equal(d_adpcm[offs[r]:offs[r] + bytes_of[r]], copy_out[2][offs[r]:offs[r] + bytes_of[r]])
                                    for r in le[:200]))
    L.vga_nwwav_bank_destroy(h)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
