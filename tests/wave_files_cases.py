"""The files of tests/test_wave_files_host.py and tests/test_gpu_wave_files.py (include/vgaudio_hip_files/wave_files.h): one
mixed set written as (channels, bits, samples, loop or None), the sample counts around every file's own span F, which is read
from the items hook and never written down here; seeded noise for the rows; the images from the oracle's WaveWriter (16-bit) or
from a small model of WaveWriter with BitDepth 8 (8-bit); two more images for the read side only (a data chunk that declares
more bytes than are present, a chunk in front of `data`); and a model of the set's layout from the rounding the header
states."""
import ctypes as C
import struct

import numpy as np

from vgaudio_amd import _lib
from vgaudio_amd.wave import WaveFileSet

HEADER_ITEM, TILE, GENERAL = 0, 1, 2
ROW_ROUND, GUARD_SAMPLES, GUARD_BYTES, SPAN_BYTES, CHUNK_BYTES = 8, 128, 256, 16384, 2048 * 16
CHANNELS = (1, 2, 3, 6, 8, 33, 255)
MASKS = {4: 0x33, 5: 0x133, 6: 0x633, 7: 0x1f3, 8: 0x6f3}
SUBTYPE_PCM = bytes([0x01, 0x00, 0x00, 0x00, 0x00, 0x00, 0x10, 0x00, 0x80, 0x00, 0x00, 0xAA, 0x00, 0x38, 0x9B, 0x71])


def up(v, m):
    return (v + m - 1) // m * m


def wave_file(nch, bits, n, loop=None, rate=44100):
    looping = loop is not None
    return _lib.WaveFileC(nch, bits, _lib.WaveParamsC(rate, n, int(looping), loop[0] if looping else 0, loop[1] if looping else 0))


def form_and_span(nch, bits):
    """(form, F) of a file of this shape, from the items hook"""
    items = [i for i in WaveFileSet.write_items([wave_file(nch, bits, 1)]) if i.form != HEADER_ITEM]
    assert items and len({(i.form, i.span) for i in items}) == 1
    return items[0].form, items[0].span


def first_general_channels(bits):
    """the smallest channel count whose file leaves the TILE form, found with the items hook"""
    lo, hi = 1, 0x7FFF                                         # lo: tile, hi: general
    assert form_and_span(lo, bits)[0] == TILE and form_and_span(hi, bits)[0] == GENERAL
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if form_and_span(mid, bits)[0] == TILE:
            lo = mid
        else:
            hi = mid
    return hi


_cases = []


def cases():
    """(channels, bits, samples, loop): computed once"""
    if _cases:
        return _cases
    out = [(1, 16, 0, None), (2, 16, 1, (0, 1)), (2, 16, 7, None), (1, 16, 8, None), (2, 8, 9, (2, 9)), (2, 8, 0, None)]
    for k, nch in enumerate(CHANNELS):
        for j, count in enumerate(("F-1", "F", "F+1", "2F+3")):
            bits = 16 if (j + k) % 2 == 0 else 8
            form, span = form_and_span(nch, bits)
            assert form == TILE and span > 0 and span % 8 == 0
            n = {"F-1": span - 1, "F": span, "F+1": span + 1, "2F+3": 2 * span + 3}[count]
            out.append((nch, bits, n, (n // 3, n - 1) if (j + 2 * k) % 3 == 0 else None))
    out.append((first_general_channels(16), 16, 9, None))
    out.append((first_general_channels(8), 8, 17, (3, 16)))
    _cases.extend(out)
    return _cases


def files_of(the_cases):
    return [wave_file(*c) for c in the_cases]


def pcm8_encode(row):
    return (((np.asarray(row, np.int16).astype(np.int32) + 0x8000) >> 8) & 0xFF).astype(np.uint8)      # Pcm8Codec.Encode


def pcm8_decode(b):
    return ((np.asarray(b, np.uint8).astype(np.int32) - 0x80) << 8).astype(np.int16)                   # Pcm8Codec.Decode


def wave8(rows, rate, looping=False, loop_start=0, loop_end=0):
    """WaveWriter.cs (:56-129) with BitDepth 8 from int16 rows, written out with struct"""
    nch, n = len(rows), len(rows[0])
    fmt_size = 40 if nch > 2 else 16
    data = nch * n
    riff = 4 + 8 + fmt_size + 8 + data + (8 + 0x3c if looping else 0)
    out = b"RIFF" + struct.pack("<i", riff) + b"WAVE"
    out += b"fmt " + struct.pack("<iHHiiHH", fmt_size, 0xFFFE if nch > 2 else 1, nch, rate, rate * nch, nch, 8)
    if nch > 2:
        out += struct.pack("<HHI", 22, 8, MASKS.get(nch, ((1 << (nch & 31)) - 1) & 0xFFFFFFFF)) + SUBTYPE_PCM
    if looping:
        out += b"smpl" + struct.pack("<i", 0x3c) + struct.pack("<7i", *[0] * 7) + struct.pack("<i", 1)
        out += struct.pack("<3i", 0, 0, 0) + struct.pack("<4i", loop_start, loop_end, 0, 0)
    out += b"data" + struct.pack("<i", data)
    if n:
        out += np.stack([pcm8_encode(r) for r in rows]).T.tobytes()
    return out


_reference = []


def reference():
    """(cases, files, rows, images): seeded noise and the image of every file, computed once and never changed.  rows: one
    int16 array per row of the set; images: one uint8 array per file."""
    if _reference:
        return _reference[0]
    from oracle import pyoracle as po
    the_cases = cases()
    rng = np.random.default_rng(0x3A7EF11E)
    rows, images = [], []
    for nch, bits, n, loop in the_cases:
        mine = [rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(nch)]
        looping = loop is not None
        ls, le = loop if looping else (0, 0)
        if bits == 16:
            rc, image = po.wave_write(mine, 44100, looping, ls, le)
            assert rc == 0
        else:
            image = np.frombuffer(wave8(mine, 44100, looping, ls, le), np.uint8).copy()
        rows += mine
        images.append(np.asarray(image, np.uint8))
    for a in rows + images:
        a.setflags(write=False)
    _reference.append((the_cases, files_of(the_cases), rows, images))
    return _reference[0]


def row_as_read(row, bits):
    """what the reader gives back for a row that went through a file of this depth"""
    return np.asarray(row, np.int16) if bits == 16 else pcm8_decode(pcm8_encode(row))


def read_side():
    """(images, rows): the reference's images that hold samples (WaveReader refuses the others: RiffParser never reaches a data
    chunk whose header ends the file) and three more for the read side only -- a 16-bit stereo file cut so that 3 data bytes
    remain (no samples), one whose data chunk declares 7 bytes more than are present, and a 3-channel file with a LIST chunk in
    front of `data` -- with the rows a reader takes out of each"""
    the_cases, files, rows, images = reference()
    out_images, out_rows, c = [], [], 0
    for (nch, bits, n, loop), image in zip(the_cases, images):
        if n:
            out_images.append(image)
            out_rows.append([row_as_read(r, bits) for r in rows[c:c + nch]])
        c += nch
    from oracle import pyoracle as po
    rng = np.random.default_rng(0x7A11)
    stereo = [rng.integers(-32768, 32768, 100).astype(np.int16) for _ in range(2)]
    rc, image = po.wave_write(stereo, 22050)
    assert rc == 0
    out_images.append(np.asarray(image[:-397], np.uint8).copy())                            # 3 of 400 data bytes: no samples
    out_rows.append([r[:0] for r in stereo])
    out_images.append(np.asarray(image[:-7], np.uint8).copy())                              # 393 of 400 data bytes: 98 samples
    out_rows.append([r[:98] for r in stereo])
    three = [rng.integers(-32768, 32768, 50).astype(np.int16) for _ in range(3)]
    rc, image = po.wave_write(three, 32000, True, 5, 45)
    assert rc == 0
    raw = bytes(image)
    at = raw.index(b"data")
    extra = b"LIST" + struct.pack("<i", 26) + bytes(range(26))
    raw = raw[:4] + struct.pack("<i", len(raw) + len(extra) - 8) + raw[8:at] + extra + raw[at:]
    out_images.append(np.frombuffer(raw, np.uint8).copy())
    out_rows.append(three)
    return out_images, out_rows


def parse(image):
    info = _lib.WaveInfoC()
    data = np.ascontiguousarray(image, dtype=np.uint8)
    _lib.check(_lib.lib().vga_wave_parse(data.ctypes.data_as(C.POINTER(C.c_uint8)), len(data), C.byref(info)))
    return info


def model(sample_counts, image_sizes, pcm_offsets=None, image_offsets=None):
    """the set's layout from the rounding the header states.  sample_counts: per file, a list with one count per row"""
    m = {"first_channel": [], "pcm_off": [], "image_off": []}
    ch = pcm_at = image_at = pcm_end = image_end = 0
    for f, (counts, size) in enumerate(zip(sample_counts, image_sizes)):
        m["first_channel"].append(ch)
        for n in counts:
            if pcm_offsets is None:
                at = pcm_at
                pcm_at += up(n, ROW_ROUND)
            else:
                at = pcm_offsets[ch]
            if n:
                pcm_end = max(pcm_end, at + n)
            m["pcm_off"].append(at)
            ch += 1
        at = image_at if image_offsets is None else image_offsets[f]
        m["image_off"].append(at)
        image_at = up(at + size, 16)
        image_end = max(image_end, image_at)
    m["channels"] = ch
    m["pcm_samples"] = (pcm_at if pcm_offsets is None else pcm_end) + GUARD_SAMPLES
    m["image_bytes"] = image_end + GUARD_BYTES
    return m


def counts_of(files):
    return [[f.params.sample_count] * f.channels for f in files]


def explicit_pcm_offsets(counts, start=3, gap=5):
    """one offset per row at odd and even sample boundaries: the rows in reverse order with gaps between them"""
    flat = [n for per in counts for n in per]
    offs, at = [0] * len(flat), start
    for c in reversed(range(len(flat))):
        offs[c] = at
        at += flat[c] + gap + c % 4
    return offs


def image_offsets_at(sizes, residue, gap=3):
    """every image at an offset of this residue mod 16, a gap between two images"""
    offs, at = [], residue
    for size in sizes:
        offs.append(at)
        at = up(at + size + gap, 16) + residue
    return offs
