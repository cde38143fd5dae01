"""The files, keys and candidate lists of tests/test_adx_keyed_files_host.py and tests/test_gpu_adx_keyed_files.py
(include/vgaudio_hip_files/adx_keyed_files.h), and what the CPU oracle says about them: the shapes of tests/adx_files_cases.py
under encryption types 8 and 9 (one at 0 with a key, one at 5), files for the span boundaries, one of more than 2^16 slots,
hand-made rows (rows are any bytes to these calls) and tiny files.  Every expectation here comes from the oracle alone
(po.adxfile_write, po.adxfile_read, po.adx_crypt, po.adx_test_key), so the table is self-consistent without a GPU; it is
computed once and never changed."""
import numpy as np

import adx_files_cases as ac
from oracle import pyoracle as po

D = ac.D
FIND_SPAN_SLOTS, CIPHER_CHUNK_SLOTS = 1024, 2048

# name -> (seed, mult, inc)
KEYS = {
    "plain": (0x4A11, 0x5A4D, 0x6B2F),
    "twin": (0x4B2E, 0x5A4D, 0x6B2F),                         # "plain" up to the seed (same top three seed bits)
    "high_seed": (0x9C31, 0x4E35, 0x5B17),                    # a seed of 0x8000 or above: slot 0 uses it unmasked
    "even_mult": (0x1234, 0x4E36, 0x0101),
    "mult0": (0x2222, 0, 0x1357),
    "inc0": (0x3333, 0x4E35, 0),
    "nine_a": (0x0A51, 0x1B45, 0x0C2D),
    "nine_b": (0x8F13, 0x0D09, 0x1E6B),                       # high seed under type 9
    "nine_c": (0x1F13, 0x0D09, 0x1E6B),                       # "nine_b" up to the seed
}
KEYS8 = ["twin", "high_seed", "even_mult", "mult0", "inc0", "plain"]
KEYS9 = ["nine_c", "nine_b", "nine_a"]
ALL_KEYS = KEYS8 + KEYS9                                     # d_keys of the write and read tests: an index names one of these

# candidate lists of the search: name -> (keys of revision 8, keys of every other non-zero revision)
FIND_LISTS = {
    "forward": (KEYS8, KEYS9),                                # "plain" and "nine_a" are tried last
    "reverse": (KEYS8[::-1], KEYS9[::-1]),                    # ... first
    "absent": ([k for k in KEYS8 if k != "plain"], [k for k in KEYS9 if k != "nine_a"]),
    "empty9": (KEYS8, []),
}


def _files():
    """(case of adx_files_cases, encryption type, key name, kind of rows)"""
    out, n8, n9 = [], 0, 0
    for i, c in enumerate(ac.CASES):
        if i % 2 == 0:
            out.append((c, 8, KEYS8[n8 % len(KEYS8)], "low"))
            n8 += 1
        else:
            out.append((c, 9, KEYS9[n9 % len(KEYS9)], "low"))
            n9 += 1
    out[1] = (ac.CASES[1], 0, "plain", "low")                 # type 0 with a key: XOR only, and the search answers -1
    out[2] = (ac.CASES[2], 5, "nine_b", "low")                # any other value: XOR only, searched like type 9
    out += [
        ((2, (448 * 2 + 1) * 32, 0, 0, 0) + D, 8, "high_seed", "holes"),      # stereo, 448 * k + 1 frames: three spans
        ((1, 2000 * 32, 0, 0, 0) + D, 9, "nine_a", "holes"),                  # mono: spans of 904 frames
        ((113, 17 * 32, 0, 0, 0) + D, 8, "inc0", "holes"),                    # spans of 8 frames, the last one short
        ((114, 20 * 32, 0, 0, 0) + D, 9, "nine_b", "holes"),                  # the general form
        ((2, 33000 * 32, 0, 0, 0) + D, 8, "plain", "holes"),                  # 66 000 slots: past the LCG's period twice
        ((3, 40 * 34, 0, 0, 0, 19, 4, 3, 1, 48000), 8, "even_mult", "holes"),
        ((2, 30 * 506, 0, 0, 0, 255, 3, 3, 1, 48000), 9, "nine_c", "holes"),
        ((4, 2100 * 68, 0, 0, 0, 36, 4, 3, 1, 48000), 8, "mult0", "holes"),   # more than one chunk of the cipher pass
        ((2, 200, 1, 5, 150) + D, 9, "nine_a", "noise"),                      # looping: more frames asked than the rows hold
        ((2, 200, 1, 5, 60) + D, 8, "plain", "noise"),                        # ... and fewer
        ((1, 64, 0, 0, 0) + D, 8, "plain", "low"),                            # a two-frame file
        ((2, 32, 0, 0, 0) + D, 8, "plain", "one_frame"),                      # one non-empty frame: "twin" fits by chance
        ((2, 100 * 32, 0, 0, 0) + D, 8, "mult0", "zeros"),                    # every candidate passes, the first wins
        ((2, 1200 * 32, 0, 0, 0) + D, 9, "nine_b", "noise"),                  # scales of any value: no candidate fits
    ]
    return out


FILES = _files()


def okey(name):
    return po.AdxKey(*KEYS[name])


def hole_slots(f):
    """slots of all-zero frames: slot 0, the middle, the last frame of the first span and the first of the next (or of the
    first chunk of the search, where that is earlier), and the file's last; and of non-empty frames with a zero scale"""
    nch, frames = f.channels, ac.row_bytes(f) // f.params.frame_size
    total = nch * frames
    span = ac.span_frames(nch) * nch if nch <= ac.SPAN_MAX_CHANNELS else CIPHER_CHUNK_SLOTS
    empty = {0, total // 2, span - 1, span, FIND_SPAN_SLOTS - 1, FIND_SPAN_SLOTS, total - 1}
    zero_scale = {1, total // 2 + 1, span + 1, total - 2}
    return sorted(s for s in empty if 0 <= s < total), sorted(s for s in zero_scale - empty if 0 <= s < total)


def make_rows(f, kind, rng):
    n, fs, nch = ac.row_bytes(f), f.params.frame_size, f.channels
    rows = [rng.integers(1, 256, n, dtype=np.uint8) for _ in range(nch)]
    if kind == "zeros":
        rows = [np.zeros(n, np.uint8) for _ in range(nch)]
    if kind != "noise":
        for r in rows:
            r[0::fs] &= 0x0F                                   # every scale below 0x1000
    if kind == "one_frame":
        rows[0][0] |= 0x08
        rows[1][:] = 0
    if kind == "holes":
        empty, zero_scale = hole_slots(f)
        for s in empty:
            rows[s % nch][(s // nch) * fs:(s // nch + 1) * fs] = 0
        for s in zero_scale:
            rows[s % nch][(s // nch) * fs:(s // nch) * fs + 2] = 0
    return rows


def oracle_params(p):
    return po.adxfile_params(p.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end, p.alignment_samples, p.frame_size, p.version,
                             p.type, p.highpass_frequency, p.encryption_type, p.trim_file)


def keyed_file(case, encryption_type):
    f = ac.adx_file(case)
    f.params.encryption_type = encryption_type
    return f


def crypt(rows, key_name, encryption_type, frame_size):
    if key_name is None or len(rows[0]) == 0:
        return [np.array(r, copy=True) for r in rows]
    return po.adx_crypt(rows, okey(key_name), encryption_type, frame_size)


def image_of(f, rows, hist, key_name):
    """the oracle's AdxWriter with that key (None: no key)"""
    src = crypt(rows, key_name, f.params.encryption_type, f.params.frame_size)
    rc, image = po.adxfile_write(src if len(rows[0]) else [np.zeros(1, np.uint8)[:0]] * f.channels, hist, oracle_params(f.params))
    assert rc == 0
    return image


_table = {}


def table():
    """files, rows, histories; per file the oracle's keyed and unkeyed image; per file of the READ set (the keyed images) the
    parsed header's numbers, the rows the oracle's reader takes out, those rows decrypted, and per candidate list the
    search's answer as an index into keys8 + keys9"""
    if _table:
        return _table
    from vgaudio_amd import adx
    rng = np.random.default_rng(0xADC0DE)
    files = [keyed_file(c, t) for c, t, _, _ in FILES]
    rows, hist, keyed, plain = [], [], [], []
    for f, (_, _, key, kind) in zip(files, FILES):
        mine = make_rows(f, kind, rng)
        h = rng.integers(-32768, 32768, f.channels).astype(np.int16)
        rows.append(mine)
        hist.append(h)
        keyed.append(image_of(f, mine, h, key))
        plain.append(image_of(f, mine, h, None))
    infos, enc_rows, dec_rows = [], [], []
    for image, f, (_, _, key, _) in zip(keyed, files, FILES):
        info = adx.parse(image.tobytes())
        rc, h, hh, chans = po.adxfile_read(image.tobytes())
        assert rc == 0 and info.revision == f.params.encryption_type
        chans = [np.array(c[:info.audio_bytes], copy=True) for c in chans]
        infos.append(info)
        enc_rows.append(chans)
        dec_rows.append(crypt(chans, key, info.revision, info.frame_size))
    found = {}
    for name, (k8, k9) in FIND_LISTS.items():
        answers = []
        for info, chans in zip(infos, enc_rows):
            sub, base = (k8, 0) if info.revision == 8 else (k9, len(k8))
            hit = -1
            if info.revision != 0:
                for i, k in enumerate(sub):
                    if info.audio_bytes == 0 or po.adx_test_key(chans, okey(k), info.revision, info.frame_size):
                        hit = base + i
                        break
            answers.append(hit)
        found[name] = answers
    for group in rows + enc_rows + dec_rows:
        for a in group:
            a.setflags(write=False)
    for a in keyed + plain:
        a.setflags(write=False)
    _table.update(files=files, rows=rows, hist=hist, keyed=keyed, plain=plain, infos=infos, enc_rows=enc_rows, dec_rows=dec_rows, found=found)
    return _table


def key_index_sets():
    """name -> (one index into ALL_KEYS per file or None, the status the call must write per file); an index that names no key
    (negative, or == nkeys) moves the file unkeyed"""
    own = [ALL_KEYS.index(k) for _, _, k, _ in FILES]
    mixed = [(-1 if i % 3 == 1 else len(ALL_KEYS) if i % 7 == 3 else v) for i, v in enumerate(own)]
    return {"own": own, "null": None, "mixed": mixed}


def key_of_index(i):
    return ALL_KEYS[i] if 0 <= i < len(ALL_KEYS) else None


def find_items_model(infos):
    out = []
    for f, i in enumerate(infos):
        total = i.frame_count * i.channel_count
        for first in range(0, total, FIND_SPAN_SLOTS):
            out.append((f, first, min(FIND_SPAN_SLOTS, total - first)))
    return out


def workspace_model(nfiles, n8, n9):
    return nfiles * ((n8 + n9 + 31) // 32) * 4
