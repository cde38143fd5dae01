"""The files of tests/test_adx_files_host.py and tests/test_gpu_adx_files.py (include/vgaudio_hip/adx_files.h): cases written as
(channels, samples, looping, loop start, loop end, frame size, version, type, trim, rate), the loop the format's BEFORE
alignment; the alignment samples are computed as CriAdxFormat.cs:59-62 computes them.  Plus a model of the set's layout built
from the per-file vga_adx_file_layout_for and the rounding the header states, and of which form a file takes."""
import ctypes as C

from vgaudio_amd import _lib

D = (18, 4, 3, 1, 48000)                                     # frame size, version, type, trim, rate unless a case says otherwise

CASES = [
    (1, 1, 0, 0, 0, 18, 4, 3, 1, 48000),                     # mono version-4 header with its extra 4 bytes
    (2, 32, 0, 0, 0, 18, 4, 3, 1, 44100),                    # one full frame
    (2, 33, 0, 0, 0, 18, 3, 3, 1, 32000),
    (2, 0, 0, 0, 0) + D,                                     # 58-byte file: the header fields end at 56, "(c)CRI" and the footer overlap them
    (3, 0, 0, 0, 0, 18, 3, 3, 1, 48000),
    (1, 200, 1, 5, 150) + D,                                 # alignment 59, 10 frames asked, rows hold 9
    (2, 200, 1, 5, 150) + D,
    (2, 200, 1, 32, 190, 18, 4, 3, 1, 22050),                # alignment 0
    (2, 200, 1, 5, 60) + D,                                  # 6 frames asked, rows hold 8 (truncation)
    (2, 200, 1, 5, 60, 18, 4, 3, 0, 48000),                  # the same with trim off
    (1, 200, 1, 33, 200, 18, 3, 3, 1, 48000),                # version-3 alignment bytes
    (2, 200, 1, 40, 200, 18, 3, 2, 1, 48000),                # Fixed: high-pass written as 0
    (255, 32, 0, 0, 0) + D,                                  # header overrun overwritten by audio
    (255, 40, 1, 3, 40, 18, 4, 4, 1, 48000),
    (3, 100, 1, 7, 90, 19, 4, 3, 1, 48000),
    (2, 1000, 0, 0, 0, 255, 3, 3, 1, 48000),
    (4, 100, 0, 0, 0, 36, 4, 3, 1, 48000),
    (8, 3000, 1, 1000, 2900) + D,
    # for the span form
    (2, 448 * 32 + 1, 0, 0, 0) + D,                          # one span (448 frames of two channels) plus one frame
    (113, 9 * 32, 0, 0, 0) + D,                              # a span of 8 frames
    (114, 64, 0, 0, 0) + D,                                  # one channel too many: the general form
]
REFUSED = {                                                  # name -> (case, code, the per-file call refuses it too)
    "header_does_not_fit": ((20, 0, 0, 0, 0) + D, -4, True),
    "frame_size_3": ((2, 100, 0, 0, 0, 3, 4, 3, 1, 48000), -4, False),      # no room for the footer: the set's own refusal
    "frame_size_2": ((2, 100, 0, 0, 0, 2, 4, 3, 1, 48000), -1, True),
    "frame_size_256": ((2, 100, 0, 0, 0, 256, 4, 3, 1, 48000), -1, True),
    "channels_0": ((0, 100, 0, 0, 0) + D, -1, True),
    "channels_256": ((256, 100, 0, 0, 0) + D, -1, True),
    "negative_samples": ((2, -1, 0, 0, 0) + D, -2, True),
    "too_large": ((255, 0x7FFFFF00, 0, 0, 0) + D, -2, True),
}
SPAN_FRAME, SPAN_BYTES, SPAN_MAX_CHANNELS, CHUNK_GRANULES, GUARD = 18, 16384, 113, 2048, 256


def up(v, m):
    return (v + m - 1) // m * m


def alignment_of(case):
    nch, n, looping, ls, le, fs = case[:6]
    spf = (fs - 2) * 2
    multiple = spf * 2 if nch == 1 else spf
    start = ls if looping else 0
    return 0 if multiple <= 0 else up(start, multiple) - start                   # CriAdxFormat.cs:59-62


def adx_file(case):
    """the _lib.AdxFileC of a case: CriAdxFormat's aligned counts, as AdxWriter hands them on"""
    nch, n, looping, ls, le, fs, version, type_, trim, rate = case
    a = alignment_of(case)
    return _lib.AdxFileC(nch, _lib.AdxFileParamsC(rate, n + a if n >= 0 else n, looping, ls + a if looping else 0, le + a if looping else 0,
                                                  a, fs, version, type_, 500, 0, trim))


def files_of(cases):
    return [adx_file(c) for c in cases]


def file_layout(f):
    lay = _lib.AdxFileLayoutC()
    return _lib.lib().vga_adx_file_layout_for(C.byref(f.params), f.channels, C.byref(lay)), lay


def row_bytes(f):
    fs = f.params.frame_size
    return -(-f.params.sample_count // ((fs - 2) * 2)) * fs


def explicit_offsets(files, residue=4, gap=40):
    """row offsets that are multiples of 4 and, with residue 4, never of 16: the rows in reverse order, gaps between them"""
    rows = [row_bytes(f) for f in files for _ in range(f.channels)]
    offs, at = [0] * len(rows), residue
    for c in reversed(range(len(rows))):
        offs[c] = at
        at = up(at + rows[c] + gap, 16) + residue
    return offs


def granule_of(*values):
    bits = 0
    for v in values:
        bits |= v
    for g in (16, 8, 4, 2):
        if bits % g == 0:
            return g
    return 1


def model(files, audio_offsets=None):
    """the set's layout and every file's form from the per-file layout and the stated rounding"""
    m = {"first_channel": [], "audio_off": [], "image_off": [], "image_size": [], "layouts": [], "span": [], "granule": [], "copy_frames": [],
         "header_end": []}
    ch = audio_at = image_at = end = 0
    for f in files:
        rc, lay = file_layout(f)
        assert rc == 0
        p, nch, rows = f.params, f.channels, row_bytes(f)
        m["first_channel"].append(ch)
        offs = []
        for i in range(nch):
            if audio_offsets is None:
                offs.append(audio_at)
                audio_at += up(rows, 16)
            else:
                offs.append(audio_offsets[ch + i])
            if rows:
                end = max(end, offs[-1] + rows)
        m["audio_off"] += offs
        m["image_off"].append(image_at)
        m["image_size"].append(lay.file_size)
        m["layouts"].append(lay)
        used = [o for o in offs if rows]
        m["span"].append(p.frame_size == SPAN_FRAME and nch <= SPAN_MAX_CHANNELS and all(o % 16 == 0 for o in used))
        m["granule"].append(granule_of(image_at + lay.audio_offset, *(used + ([p.frame_size] if nch > 1 else []))))
        m["copy_frames"].append(min(rows // p.frame_size, lay.frame_count))
        m["header_end"].append(max(lay.audio_offset, 20 + (4 + 4 * nch + (4 if nch == 1 else 0) if p.version == 4 else 0) + 24))
        image_at += up(lay.file_size, 16)
        ch += nch
    m["channels"] = ch
    m["audio_bytes"] = (audio_at if audio_offsets is None else end) + GUARD
    m["image_bytes"] = image_at + GUARD
    return m


def span_frames(nch):
    return SPAN_BYTES // (SPAN_FRAME * nch) // 8 * 8


def info_of(f, lay):
    """the vga_adx_file_info vga_adx_parse fills for the image of file f, as far as the set reads it"""
    i = _lib.AdxFileInfoC()
    fs = f.params.frame_size
    i.header_size, i.frame_size, i.channel_count, i.sample_count = lay.header_size, fs, f.channels, lay.sample_count
    i.version, i.sample_rate, i.audio_offset = f.params.version, f.params.sample_rate, lay.audio_offset
    i.samples_per_frame, i.frame_count, i.audio_bytes = (fs - 2) * 2, lay.frame_count, lay.frame_count * fs
    for c in range(f.channels):
        i.history[c][0] = i.history[c][1] = (c * 37 + 11) % 65536 - 32768
    return i


def odd_image_offsets(sizes, start=3, step=5):
    """images at odd byte offsets, every residue of 16 among them"""
    offs, at = [], start
    for k, size in enumerate(sizes):
        offs.append(at)
        at = at + size + 1 + (k * step) % 16
    return offs
