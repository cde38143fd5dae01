"""The files of tests/test_hca_files_host.py and tests/test_gpu_hca_files.py (include/vgaudio_hip/hca_files.h): cases written as
(frame size, frame count, channels, looping, volume, comment length or None, header size mod 16, encrypted ids, key), the infos
built from vga_hca_encoder_initialize with frame_size, frame_count, comment_length and header_size replaced (the container
does not look inside a frame, so random bytes with a valid CRC-16 serve as frames).  Plus the keys of one set, a model of the
set's layout from the rounding the header states, and what the oracle writes and reads for every file."""
import ctypes as C

import numpy as np

from vgaudio_amd import _lib

SPAN_BYTES, MAX_SPAN_FRAME, SLACK, GUARD = 16384, 4096, 8, 256
NONE, TYPE1, TYPE0, KEY_A, KEY_B = -1, 0, 1, 2, 3            # `key`: index into KEYS
KEYS = [(1, 0), (0, 0), (56, 0xCC55463930DBE1AB), (56, 0x0123456789ABCDEF)]     # (key type, key code); type 0 is the identity table


def span_frames(fs):
    return max(1, SPAN_BYTES // fs)


CASES = [
    # fs, frames, nch, loop, volume, comment, header % 16, ids, key
    (8, span_frames(8) - 1, 1, 0, 1.0, None, 0, 0, NONE),     # the parser's minimum: a lane per frame; one less than a span
    (8, span_frames(8), 1, 0, 1.0, None, 1, 1, KEY_A),        # exactly one span
    (8, span_frames(8) + 1, 2, 0, 0.5, 3, 2, 0, TYPE1),       # one more
    (9, 5, 1, 1, 1.0, 0, 3, 0, TYPE1),                        # (an empty comment is the pad chunk)
    (341, span_frames(341), 2, 0, 1.0, 17, 4, 1, KEY_A),
    (341, span_frames(341) - 1, 2, 1, 2.0, None, 7, 0, NONE),
    (341, span_frames(341) + 1, 2, 0, 1.0, 40, 8, 1, KEY_B),
    (682, 0, 2, 0, 1.0, None, 15, 0, NONE),                   # no frames: a header alone
    (682, 0, 2, 0, 1.0, None, 0, 1, KEY_A),
    (682, 1, 2, 0, 1.0, None, 0, 0, TYPE0),                   # the identity table: the CRC is refreshed all the same
    (682, 30, 2, 1, 0.25, 255, 0, 1, KEY_A),
    (683, span_frames(683) + 1, 2, 0, 1.0, None, 1, 0, NONE),
    (683, 7, 1, 0, 1.0, 1, 2, 1, TYPE0),
    (4095, span_frames(4095) + 1, 2, 0, 1.0, None, 3, 1, KEY_B),
    (4096, span_frames(4096), 2, 0, 1.0, None, 4, 0, TYPE1),  # the largest frame of the span form (and of vga_hca_crypt_device)
    (4096, span_frames(4096) - 1, 2, 0, 1.0, 9, 7, 0, NONE),
    (4097, span_frames(4097), 2, 0, 1.0, None, 8, 1, KEY_A),  # one byte more: the general form, one item
    (4097, span_frames(4097) + 1, 2, 1, 1.0, None, 15, 0, NONE),
    (32767, 2, 2, 0, 1.0, None, 0, 1, KEY_B),
    (32767, 2, 1, 0, 3.0, 2, 5, 0, NONE),
]
# (file, frame) whose stored bytes are damaged: the first, a middle and the last frame of three files, keyed and unkeyed,
# one frame on each side of a span's edge, and a general file's
BAD_FRAMES = [(1, 0), (1, 1000), (1, 2047), (5, 0), (5, 20), (5, 46), (10, 0), (10, 23), (10, 24), (10, 29), (2, 2047), (2, 2048),
              (17, 1), (18, 1)]


def up(v, m):
    return (v + m - 1) // m * m


def needed_header(loop, volume, comment):
    """the chunks and the CRC; a reader takes "pad" for a chunk only with a zero byte behind its three letters"""
    return 8 + 16 + 16 + (16 if loop else 0) + 6 + (8 if volume != 1.0 else 0) + (5 + comment + 1 if comment else 3 + 1) + 2


def comment_of(case):
    n = case[5]
    return None if n is None else "".join(chr(ord("a") + i % 26) for i in range(n))


def info_of(case):
    fs, fc, nch, loop, volume, comment, residue = case[:7]
    p = _lib.HcaParamsC(2, 0, 0, nch, 48000 if nch == 2 else 44100, 5000, loop, 1000 if loop else 0, 4000 if loop else 0)
    h = _lib.HcaInfoC()
    _lib.check(_lib.lib().vga_hca_encoder_initialize(C.byref(p), C.byref(h)))
    need = needed_header(loop, volume, comment or 0)
    h.header_size = need + (residue - need) % 16
    h.frame_size, h.frame_count, h.comment_length = fs, fc, comment or 0
    h.sample_count = fc * 1024 - h.inserted_samples if fc else 0
    if loop:
        h.loop_start_frame, h.loop_end_frame = 0, max(fc - 1, 0)
    return h


def enc_type_of(case):
    return KEYS[case[8]][0] if case[8] >= 0 else 0


def hca_file(case):
    c = comment_of(case)
    return _lib.HcaFileC(info_of(case), None if c is None else c.encode(), case[4], enc_type_of(case), case[7], case[8])


def files_of(cases):
    return [hca_file(c) for c in cases]


def key_tables():
    """(decryption tables, encryption tables), [len(KEYS), 256] each, from the library's vga_hca_key_tables"""
    dec, enc = np.zeros((len(KEYS), 256), np.uint8), np.zeros((len(KEYS), 256), np.uint8)
    for k, (kind, code) in enumerate(KEYS):
        _lib.check(_lib.lib().vga_hca_key_tables(kind, code, dec[k].ctypes.data_as(_lib.u8p), enc[k].ctypes.data_as(_lib.u8p)))
    return dec, enc


def model(files, frame_offsets=None):
    """the layout the header states"""
    sizes = [f.hca.header_size + f.hca.frame_count * f.hca.frame_size for f in files]
    streams = [f.hca.frame_count * f.hca.frame_size for f in files]
    image_off, at = [], 0
    for s in sizes:
        image_off.append(at)
        at += up(s, 16)
    if frame_offsets is None:
        frame_off, fat = [], 0
        for b in streams:
            frame_off.append(fat)
            fat += up(b, 4)
        end = fat
    else:
        frame_off = [int(o) for o in frame_offsets]
        end = max([o + up(b, 4) for o, b in zip(frame_off, streams) if b] + [0])
    return dict(image_off=image_off, image_size=sizes, image_bytes=at + GUARD, frame_off=frame_off, stream_bytes=streams,
                frame_bytes=end + SLACK, total_frames=sum(f.hca.frame_count for f in files),
                span=[f.hca.frame_size <= MAX_SPAN_FRAME for f in files])


def explicit_frame_offsets(files, gap=0):
    """the streams in reverse order with gaps, at offsets whose residues mod 16 run through 0, 4, 8, 12"""
    offs, at = [0] * len(files), 32
    for k, f in enumerate(reversed(range(len(files)))):
        at = up(at, 16) + 4 * (k % 4)
        offs[f] = at
        at += up(files[f].hca.frame_count * files[f].hca.frame_size, 4) + gap
    return offs


def odd_image_offsets(sizes):
    """images at byte offsets whose residues mod 16 run through 1, 2, 3, 5, 8, 15, with gaps"""
    offs, at = [], 0
    for k, s in enumerate(sizes):
        at = up(at, 16) + 16 + (1, 2, 3, 5, 8, 15)[k % 6]
        offs.append(at)
        at += s + 5
    return offs


# ---------------------------------------------------------------- the oracle's side
def oracle_info(h):
    from oracle import pyoracle as po
    return po.HcaInfo.from_buffer_copy(bytes(h))


def identity():
    return np.arange(256, dtype=np.uint8)


def valid_frames(seed, fs, fc):
    """random frames with the CRC-16 the oracle's CryptFrame leaves under the identity table"""
    from oracle import pyoracle as po
    raw = np.random.default_rng(seed).integers(0, 256, fs * fc, dtype=np.uint8)
    return po.hca_crypt(raw, fs, identity()) if fc else raw


def damage(frames, fs, frame):
    frames[frame * fs + (frame * 7) % (fs - 2)] ^= 0x5A


def input_frames(cases, bad=()):
    """one flat array of frames per case, the frames of `bad` damaged"""
    out = [valid_frames(1000 + i, c[0], c[1]) for i, c in enumerate(cases)]
    for f, k in bad:
        damage(out[f], cases[f][0], k)
    return out


def bad_count(frames, fs):
    """frames whose last two bytes are not the oracle's CRC-16 of the bytes before them"""
    from oracle import pyoracle as po
    if len(frames) == 0:
        return 0
    a, b = np.asarray(frames).reshape(-1, fs), po.hca_crypt(frames, fs, identity()).reshape(-1, fs)
    return int((a[:, -2:] != b[:, -2:]).any(axis=1).sum())


def oracle_image(case, frames, enc_tables):
    """crypt with the file's table (if it has a key), then HcaWriter: (rc, image)"""
    from oracle import pyoracle as po
    fs, key = case[0], case[8]
    body = po.hca_crypt(frames, fs, enc_tables[key]) if key >= 0 and len(frames) else np.asarray(frames, dtype=np.uint8)
    return po.hcafile_write(oracle_info(info_of(case)), body, comment_of(case), case[4], enc_type_of(case), bool(case[7]))


def oracle_read(image, frames_offset, fs, fc, dec_table):
    """(frames as delivered, bad-CRC count): HcaReader's frames, CRC as stored, then CryptFrame if there is a key"""
    from oracle import pyoracle as po
    stored = np.asarray(image[frames_offset:frames_offset + fs * fc], dtype=np.uint8)
    out = po.hca_crypt(stored, fs, dec_table) if dec_table is not None and fc else stored.copy()
    return out, bad_count(stored, fs)
