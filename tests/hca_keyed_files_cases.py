"""The files, keys and candidate lists of tests/test_hca_keyed_files_host.py and tests/test_gpu_hca_keyed_files.py
(include/vgaudio_hip_files/hca_keyed_files.h), and what the CPU oracle says about them.  Every stream is at most 14 frames,
mono and stereo, two qualities; hand-made frames are random bytes behind a valid sync word (frames are any bytes to these
calls).  Every expectation comes from the oracle alone (po.hca_encode, po.hca_crypt, po.hca_key_tables, po.hca_find_key,
po.hcafile_write), so the table is self-consistent without a GPU; it is computed once and never changed."""
import functools

import numpy as np

from oracle import pyoracle as po
from vgaudio_amd import synth

KEY_BLOCK = 64                                   # candidates per work item
STAGE_MAX_FRAME = 2048                           # the largest first tested frame the search stages in LDS
STAGE_REST_BYTES = 9216                          # the later tested frames are staged when together they are no longer
NCODES, NSINGLE = 130, 16
_rng = np.random.default_rng(20260)
CODES = [int(c) for c in _rng.integers(1, 2 ** 56, NCODES)]

# candidate lists: name -> indices into CODES (the candidates are d_tables[0 .. nkeys) in that order)
LISTS = {
    "main": list(range(12)),
    "n1": [0],
    "n63": list(range(63)),
    "n64": list(range(64)),
    "n65": list(range(65)),
    "n130": list(range(130)),
    "none": [],
}

# (name, channels, quality, frames, encryption type, index of the key into CODES or None, what is done to the stream)
FILES = [
    ("type0", 2, "High", 6, 0, None, ""),
    ("type1", 2, "Low", 6, 1, None, ""),
    ("first", 2, "High", 14, 56, 0, ""),
    ("middle", 1, "Low", 12, 56, 5, ""),
    ("last", 2, "Low", 12, 56, 11, ""),
    ("absent", 1, "High", 11, 56, 100, ""),
    ("silent", 2, "Low", 12, 56, 3, "silent"),
    ("silent3", 2, "High", 14, 56, 4, "silent3"),
    ("short_tail", 2, "High", 7, 56, 6, "silent3"),
    ("no_frames", 2, "High", 0, 56, 7, ""),
    ("damage10", 2, "Low", 14, 56, 8, "damage9"),
    ("damage11", 2, "Low", 14, 56, 8, "damage10"),
    ("sync_with_key", 2, "High", 12, 56, 2, "sync2"),
    ("sync_without_key", 2, "High", 12, 56, 101, "sync2"),
    ("random_a", 2, "Low", 1, 56, None, "random@3005"),              # one frame: wrong keys pass (two of CODES do)
    ("random_b", 2, "Low", 2, 56, None, "random@3005+lead"),         # a first frame EVERY key passes, then random_a's
    ("random_c", 2, "Low", 11, 56, None, "random+lead"),             # ... then ten random frames: every candidate walks on
    ("random_8", 1, "Low", 5, 56, None, "random:8"),
    ("random_2049", 2, "Low", 4, 56, None, "random:2049"),
    ("random_32767", 2, "Low", 3, 56, None, "random:32767"),
    ("random_4096", 2, "High", 3, 56, None, "random:4096"),
    ("random_4097", 2, "High", 3, 56, None, "random:4097"),
    ("key129", 1, "Low", 10, 56, 129, ""),
    ("key63", 2, "Low", 10, 56, 63, ""),
    ("key64", 1, "High", 10, 56, 64, ""),
    # every candidate passes the first frame and walks the later ones: read from global memory (3 x 32767 bytes), staged at
    # the limit (9 x 1024 = STAGE_REST_BYTES) and one step past it (9 x 1025)
    ("lead_32767", 2, "Low", 4, 56, None, "random:32767+lead"),
    ("lead_1024", 2, "Low", 10, 56, None, "random:1024+lead"),
    ("lead_1025", 2, "Low", 10, 56, None, "random:1025+lead"),
]
NAMES = [f[0] for f in FILES]


def index_of(name):
    return NAMES.index(name)


def first_non_empty(frames):
    """FindFirstNonEmptyFrame (CriHcaEncryption.cs:65-88) and the number of frames TestKey reads, in Python"""
    fc = len(frames)
    first = next((j for j in range(fc) if frames[j, 2:frames.shape[1] - 2].any()), 0)
    return first, min(10, fc - first)


_CRC = []


def bad_crc_frames(frames):
    """the frames whose last two bytes are not the CRC-16 (polynomial 0x8005, MSB first, from 0) of the bytes in front, in Python"""
    if not _CRC:
        for b in range(256):
            c = b << 8
            for _ in range(8):
                c = ((c << 1) ^ (0x8005 if c & 0x8000 else 0)) & 0xFFFF
            _CRC.append(c)
    bad = 0
    for fr in np.asarray(frames, np.uint8).tolist():
        c = 0
        for b in fr[:-2]:
            c = ((c << 8) ^ _CRC[(c >> 8) ^ b]) & 0xFFFF
        bad += c != (fr[-2] << 8 | fr[-1])
    return bad


def copy_info(info):
    return po.HcaInfo.from_buffer_copy(info)


def _stream(n, nch, quality, frame_count, what, enc_table):
    """(oracle info, plain frames, frames as they lie in the image)"""
    rng = np.random.default_rng(1000 + n)
    samples = 1024 * max(frame_count, 1) - 300
    pcm = synth.generate(nch, samples) if what != "silent" else np.zeros((nch, samples), np.int16)
    rc, info, frames = po.hca_encode(pcm, po.hca_params(nch, samples, quality=quality))
    assert rc == 0
    if frame_count == 0:
        info = copy_info(info)
        info.frame_count = 0
        frames = frames[:0]
    assert info.frame_count == frame_count and len(frames) == frame_count, (n, info.frame_count)
    if what == "silent3":
        rc, _, quiet = po.hca_encode(np.zeros((nch, samples), np.int16), po.hca_params(nch, samples, quality=quality))
        assert rc == 0 and quiet.shape == frames.shape
        frames = frames.copy()
        frames[:3] = quiet[:3]
    if what.startswith("random"):
        info = copy_info(info)
        lead = what.endswith("+lead")
        what = what[:-5] if lead else what
        if "@" in what:
            what, seed = what.split("@")
            rng = np.random.default_rng(int(seed))
        if ":" in what:
            info.frame_size = int(what.split(":")[1])
        frames = rng.integers(0, 256, (frame_count - lead, info.frame_size)).astype(np.uint8)
        frames[:, :2] = 0xFF
        frames[:, 2] &= 0x0F                                           # small noise levels: more frames survive
        if lead:
            # noise level 0 and no scale factors under every key (0x00 is a fixed point of every table), but not an EMPTY
            # frame to FindFirstNonEmptyFrame: every candidate passes it and walks the frames behind it
            first = np.random.default_rng(7).integers(1, 256, (1, info.frame_size)).astype(np.uint8)
            first[0, :2], first[0, 2:16] = 0xFF, 0                      # (past the bits skipped between the channels' headers)
            frames = np.concatenate([first, frames])
        return info, frames, frames.copy()                             # any bytes: stored as they are
    plain = np.ascontiguousarray(frames)
    enc = plain.copy()
    if enc_table is not None and frame_count:
        enc = po.hca_crypt(plain, info.frame_size, enc_table).reshape(plain.shape)
    if what.startswith("damage"):
        enc[int(what[6:]), 6:70] ^= 0x5A
    if what == "sync2":
        enc[2, 0] = 0x00                                               # 0x00 and 0xFF are fixed points of every table
    return info, plain, enc


def verdict(r):
    """what po.hca_find_key returns -> (index, status) of the set call"""
    return (r, 0) if r >= 0 else ((-1, 1) if r == -1 else (-1, 2))


@functools.lru_cache(maxsize=None)
def table():
    from vgaudio_amd import hca
    dec, enc = np.zeros((NCODES, 256), np.uint8), np.zeros((NCODES, 256), np.uint8)
    for k, code in enumerate(CODES):
        rc, dec[k], enc[k] = po.hca_key_tables(56, code)
        assert rc == 0
    rc, dec1, enc1 = po.hca_key_tables(1)
    assert rc == 0
    t = {"dec": dec, "enc": enc, "dec1": dec1, "oinfo": [], "plain": [], "stored": [], "datas": [], "infos": [], "types": [], "first": []}
    for n, (name, nch, quality, frame_count, etype, key, what) in enumerate(FILES):
        enc_table = enc1 if etype == 1 else (enc[key] if key is not None else None)
        info, plain, stored = _stream(n, nch, quality, frame_count, what, enc_table)
        rc, image = po.hcafile_write(info, stored, encryption_type=etype, encrypted_ids=etype != 0)
        assert rc == 0, (name, rc)
        t["oinfo"].append(info)
        t["plain"].append(plain)
        t["stored"].append(stored)
        t["datas"].append(image.tobytes())
        parsed = hca.parse(image.tobytes())
        assert parsed.encryption_type == etype and parsed.hca.frame_size == info.frame_size and parsed.hca.frame_count == frame_count
        t["infos"].append(parsed)
        t["types"].append(etype)
        t["first"].append(first_non_empty(stored))
    # the candidates (of the first NSINGLE) that pass the FIRST tested frame alone: the ones that walk the later frames
    t["first_frame_passes"] = []
    for n, stored in enumerate(t["stored"]):
        first, ntest = t["first"][n]
        one = copy_info(t["oinfo"][n])
        one.frame_count = 1
        t["first_frame_passes"].append([k for k in range(NSINGLE) if t["types"][n] == 56 and ntest > 0
                                        and po.hca_find_key(one, stored[first:first + 1], dec[k][None, :]) == 0])
    t["bad_crc"] = [bad_crc_frames(stored) for stored in t["stored"]]   # of the frames as they lie in the image
    # what the search must give: name of the list -> [(index, status)] per file, the type-1 files given `type1_index`
    t["found"] = {}
    for name, codes in LISTS.items():
        tabs = dec[codes] if codes else np.zeros((0, 256), np.uint8)
        row = []
        for n, etype in enumerate(t["types"]):
            if etype != 56:
                row.append((len(codes) if etype == 1 else -1, 0))
            elif not codes:
                row.append((-1, 1))
            else:
                row.append(verdict(po.hca_find_key(t["oinfo"][n], t["stored"][n], tabs)))
        t["found"][name] = row
    # every candidate singly: file -> [oracle's answer over the one-key list]: 0 passes, -1 fails, -3 wrong sync word
    # (the first NSINGLE candidates; all of them on the two files made for wrong keys that pass)
    t["single"] = {n: [po.hca_find_key(t["oinfo"][n], t["stored"][n], dec[k][None, :])
                       for k in range(NCODES if NAMES[n] in ("random_a", "random_b") else NSINGLE)]
                   for n, etype in enumerate(t["types"]) if etype == 56}
    return t


def find_items_model(types, nkeys):
    return [(f, k, min(KEY_BLOCK, nkeys - k)) for f, e in enumerate(types) if e == 56 for k in range(0, nkeys, KEY_BLOCK)]


def workspace_model(nfiles, nkeys):
    return 8 * nfiles + (nfiles * nkeys + 3) // 4 * 4


def read_key_indices():
    """per-file table indices of the keyed read tests over d_tables = dec[0 .. 130) + the type-1 table: the file's own key, the
    type-1 table for the type-1 file, -1 for type 0, and for the hand-made files -1, >= ntables, and two valid ones"""
    out = []
    for name, _, _, _, etype, key, _ in FILES:
        out.append(NCODES if etype == 1 else (key if key is not None else -1))
    out[index_of("random_a")] = NCODES + 1                              # == ntables: moved unkeyed, status 1
    out[index_of("random_b")] = NCODES + 40
    out[index_of("random_4096")] = 9
    out[index_of("random_4097")] = 10
    out[index_of("random_32767")] = 11
    out[index_of("random_8")] = 12
    out[index_of("no_frames")] = -7
    return out
