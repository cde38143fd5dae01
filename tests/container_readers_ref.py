"""An independent `struct` restatement of the DSP, ADX and HCA file layouts the readers take (Containers/Dsp/DspReader.cs,
Containers/Adx/AdxReader.cs, Containers/Hca/HcaReader.cs), used to build headers the product writers never produce: a
channel count of 0, loop blocks cut off by a small HeaderSize, negative header sizes, dec / ath / vbr / comm chunks,
old versions.  Everything is big-endian."""
import struct

import numpy as np


def gc_bytes(samples):
    """SampleCountToByteCount (GcAdpcmMath.cs)"""
    frames, extra = divmod(samples, 14)
    return frames * 8 + (0 if extra == 0 else (extra + 1) // 2 + 1)


def gc_nibbles(samples):
    frames, extra = divmod(samples, 14)
    return frames * 16 + (0 if extra == 0 else extra + 2)


def gc_nibble_to_sample(nibble):
    frames, extra = divmod(nibble, 16)
    return frames * 14 + max(extra - 2, 0)


def next_multiple(v, m):
    return v if m <= 0 or v % m == 0 else v + m - v % m


# ---------------------------------------------------------------- DSP
def dsp_channel_header(sample_count, rate, looping=False, fmt=0, start_addr=2, end_addr=0, cur_addr=2, nibble_count=None,
                       coefs=None, gain=0, start_ctx=(0, 0, 0), loop_ctx=(0, 0, 0), channel_field=0, fpi=0):
    """one 0x60-byte header (DspReader.ReadHeader :57-85 reads these offsets)"""
    h = bytearray(0x60)
    nibbles = gc_nibbles(sample_count) if nibble_count is None else nibble_count
    struct.pack_into(">iiihhiii", h, 0, sample_count, nibbles, rate, 1 if looping else 0, fmt, start_addr, end_addr, cur_addr)
    coefs = list(coefs) if coefs is not None else [0] * 16
    struct.pack_into(">16h", h, 0x1c, *coefs)
    struct.pack_into(">h3h3h", h, 0x3c, gain, *start_ctx, *loop_ctx)
    struct.pack_into(">hh", h, 0x4a, channel_field, fpi)
    return bytes(h)


def dsp_interleave(rows, interleave):
    """Interleave(rows, interleave, outputSize = GetNextMultiple(bytes, 8)) for equally long rows"""
    size = next_multiple(len(rows[0]), 8)
    padded = [bytes(r) + bytes(size - len(r)) for r in rows]
    out = bytearray()
    for b in range(0, size, interleave):
        for r in padded:
            out += r[b:b + interleave]
    return bytes(out)


# ---------------------------------------------------------------- ADX
def adx_header(header_size, nch, sample_count, frame_size=18, type_=3, bit_depth=4, rate=48000, highpass=500, version=4,
               revision=0, history=None, inserted=0, loop_count=0, loop=(0, 0, 0, 0, 0), write_loop=True):
    """AdxReader.ReadHeader (:71-114) field by field; returns header_size + 4 bytes (the audio follows)"""
    h = bytearray(struct.pack(">Hhbbbbiihbb", 0x8000, header_size, type_, frame_size, bit_depth, nch, rate, sample_count,
                              highpass, version, revision))
    if version >= 4:
        h += bytes(4)
        hist = history if history is not None else [(0, 0)] * nch
        for a, b in hist:
            h += struct.pack(">hh", a, b)
        if nch == 1:
            h += bytes(4)
    if write_loop:
        h += struct.pack(">hh", inserted, loop_count) + struct.pack(">5i", *loop)
    size = max(header_size + 4, 0)
    h = h[:size] + bytes(max(size - len(h), 0))
    if size >= 6:
        h[size - 6:size] = b"(c)CRI"
    return bytes(h)


def adx_interleave(rows, frame_size):
    n = len(rows[0]) // frame_size
    out = bytearray()
    for k in range(n):
        for r in rows:
            out += bytes(r[k * frame_size:(k + 1) * frame_size])
    return bytes(out)


# ---------------------------------------------------------------- HCA
def _id(name, mask):
    b = name.encode("ascii").ljust(4, b"\0")
    return bytes(c | 0x80 if mask and c else c for c in b)


def hca_fmt(nch, rate, frame_count, inserted=0, appended=0, mask=False):
    return _id("fmt", mask) + struct.pack(">B", nch) + struct.pack(">I", rate)[1:] + struct.pack(">ihh", frame_count, inserted, appended)


def hca_comp(frame_size, min_res=1, max_res=15, tracks=1, config=0, total=128, base=128, stereo=0, per_hfr=0, r1=0, r2=0,
             mask=False):
    return _id("comp", mask) + struct.pack(">h10B", frame_size, min_res, max_res, tracks, config, total, base, stereo, per_hfr, r1, r2)


def hca_dec(frame_size, min_res, max_res, total_minus1, base_minus1, tracks, config, stereo_type, mask=False):
    return _id("dec", mask) + struct.pack(">h6B", frame_size, min_res, max_res, total_minus1, base_minus1, tracks << 4 | config,
                                          stereo_type)


def hca_loop(start_frame, end_frame, pre, post, mask=False):
    return _id("loop", mask) + struct.pack(">iihh", start_frame, end_frame, pre, post)


def hca_ath(kind, mask=False):
    return _id("ath", mask) + struct.pack(">h", kind)


def hca_ciph(kind, mask=False):
    return _id("ciph", mask) + struct.pack(">h", kind)


def hca_rva(volume, mask=False):
    return _id("rva", mask) + struct.pack(">f", volume)


def hca_vbr(max_frame, noise, mask=False):
    return _id("vbr", mask) + struct.pack(">hh", max_frame, noise)


def hca_comm(text, mask=False):
    return _id("comm", mask) + b"\0" + text + b"\0"


def hca_pad(mask=False):
    return _id("pad", mask)


def hca_image(chunks, frames, header_size=None, version=0x0200, mask=False):
    """'HCA\\0' version header_size, the chunks, zero padding to header_size - 2, a CRC-16 slot, then the frames"""
    body = b"".join(chunks)
    hs = header_size if header_size is not None else next_multiple(8 + len(body) + 2, 32)
    h = bytearray(_id("HCA", mask) + struct.pack(">hh", version, hs) + body)
    h += bytes(max(hs - len(h), 0))
    return bytes(h[:max(hs, len(h))]) + bytes(frames)


def _crc16_table():
    out = []
    for b in range(256):
        crc = b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x8005) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
        out.append(crc)
    return out


_CRC16 = _crc16_table()


def crc16(data):
    """Crc16(0x8005).Compute: MSB first, initial value 0"""
    crc = 0
    for b in bytes(data):
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16[(crc >> 8) ^ b]
    return crc


def bad_crc_frames(frames):
    """frames whose last two bytes are not the CRC-16 of the others"""
    return sum(crc16(f[:-2]) != (int(f[-2]) << 8 | int(f[-1])) for f in frames)


def hca_frames(frame_count, frame_size, rng, good_crc=True):
    """frames of random bytes behind a 0xFFFF sync word, each with its CRC-16"""
    out = np.zeros((frame_count, frame_size), dtype=np.uint8)
    for k in range(frame_count):
        body = bytes([0xFF, 0xFF]) + rng.integers(0, 256, frame_size - 4, dtype=np.uint8).tobytes()
        c = crc16(body) if good_crc else crc16(body) ^ 1
        out[k] = np.frombuffer(body + struct.pack(">H", c), dtype=np.uint8)
    return out
