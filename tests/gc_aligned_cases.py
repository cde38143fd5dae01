"""What tests/test_gc_aligned_host.py and tests/test_gpu_gc_aligned.py share: the files of the set, a model of the packed layout
of include/vgaudio_hip/gc_files_aligned.h built from the PER-FILE size call of the library (vga_gcadpcm_channel_layout_for) and
the rounding rules the header states, the per-channel numbers of GcAdpcmAlignment.cs:29-39 computed here, and the oracle's
side of every channel (po.gc_build_channel), computed once."""
import ctypes as C

import numpy as np

from oracle import pyoracle as po
from vgaudio_amd import _lib

RATE = 32000
# (channels, samples, loop start, loop end, alignment multiple, samples per seek entry), looping
LOOPING = [
    (1, 2, 1, 2, 4, 14),               # keeps no frame, histories 0, loop of length 1 wrapped four times
    (2, 28, 1, 14, 14, 14),            # loop end on a frame boundary: head 0; output row (27) shorter than input (28)
    (2, 29, 2, 20, 4, 14),
    (3, 15, 1, 15, 8, 5),              # seek entries inside the re-encoded tail
    (2, 100, 15, 57, 14, 14),          # loop ends before the data: aligned count 70 < 100
    (2, 130, 99, 100, 28, 14),         # loop of length 1 far in
    (1, 57, 30, 40, 7, 0),             # no seek table
    (1, 100, 50, 100, 64, 14),         # aligned count 114 > 100: output row longer than input
    (2, 43, 14, 43, 14, 28),           # already aligned: copied through
    (2, 13, 0, 13, 14, 14),            # loop start 0: default context
    (1, 40, 13, 27, 14, 14),           # aligned count a multiple of 14
    (1, 30000, 1, 30000, 0x3800, 0x3800),   # the default multiple: a tail of 14 347 samples, tail 8 mod 16 into its row
    (6, 43, 15, 43, 2, 28),            # a tail of 2 samples, six channels
    (1, 16, 1, 3, 2, 2),               # spacing 2
]
# The ragged encoder cuts a channel into time pieces of at least 3584 frames (plan_encode_pieces: MIN_PIECE_FRAMES) and the
# tail of 14 347 samples (1025 frames) is one piece.  Two pieces need 7168 frames = 100 339 samples or more; a tail is at most
# multiple + 12 samples (loop start 1 mod the multiple, loop end 13 mod 14), so 100 327 is the smallest multiple whose tail
# spans two pieces: this file's tail is 13 + 100 326 = 100 339 samples, and it keeps no frame.  Its 100 325 samples are the
# fewest with which the aligned loop start (100 327) still lies inside the original data, as the loop context needs; its PCM
# is the 30 000 samples of its channel, repeated.
TWO_PIECE_MULTIPLE = 100327
TWO_PIECES = (1, 100325, 1, 13, TWO_PIECE_MULTIPLE, 0x3800)
MIN_PIECE_FRAMES = 3584
# (channels, samples), not looping, spacing 14
PLAIN = [(2, 0), (1, 1), (255, 15)]
# rc -2 from po.gc_build_channel WITH a context (the aligned loop start lies past the original data): the call-time refusals
CTX_REFUSED = [(2, 14, 1, 14, 14, 14), (1, 100, 15, 100, 0x3800, 0x3800), (2, 100, 99, 100, 28, 14)]

CHUNK = 1024                                                           # samples, granules and entries of one work item (gc_aligned_host.hpp)


def looping(t):
    nch, n, ls, le, multiple, spacing = t
    return (nch, n, 1, ls, le, spacing, multiple)


def plain(t):
    return (t[0], t[1], 0, 0, 0, 14, 0)


# the set, as (channels, samples, looping, loop start, loop end, spacing, alignment): the files that do not loop between the others
SET = ([looping(t) for t in LOOPING[:2]] + [plain(PLAIN[0])] + [looping(t) for t in LOOPING[2:8]] + [plain(PLAIN[1])] +
       [looping(t) for t in LOOPING[8:]] + [looping(TWO_PIECES), plain(PLAIN[2])])
REFUSED_SET = [looping(t) for t in CTX_REFUSED]
NEEDS = [f for f in SET if f[6] and f[3] % f[6]]                      # every file of it needs alignment
BIG = [(2, 5_000_000, 1, 28, 4_000_000, 14, 0x3800), (255, 15, 1, 1, 15, 14, 0x3800), (1, 3_000_001, 1, 1, 3_000_001, 0x3800, 0x3800),
       (3, 70_001, 1, 14, 70_000, 1, 0)]


def gc_file(channels, samples, looping_, loop_start, loop_end, spacing, alignment=0, rate=RATE):
    return _lib.GcFileC(channels, rate, _lib.GcChannelParamsC(samples, looping_, loop_start, loop_end, alignment, spacing))


def files_of(tuples):
    return [gc_file(*t) for t in tuples]


def byte_count(samples):
    return _lib.lib().vga_gcadpcm_sample_count_to_byte_count(samples)


def up(v, m):
    return (v + m - 1) // m * m


def channel_layout(f):
    lay = _lib.GcChannelLayoutC()
    assert _lib.lib().vga_gcadpcm_channel_layout_for(C.byref(f.channel), C.byref(lay)) == 0
    return lay


def alignment_numbers(f):
    """GcAdpcmAlignment.cs:29-39 for one file, computed here: the AlignRow numbers of each of its channels"""
    p = f.channel
    ls, le, m, n = p.loop_start, p.loop_end, p.loop_alignment_multiple, p.sample_count
    needed = m != 0 and ls % m != 0
    if not needed:
        return {"needed": False, "loop_start_aligned": ls, "out_samples": n, "bytes_to_keep": byte_count(n), "samples_to_keep": n,
                "samples_to_encode": 0, "head": 0, "loop_start": ls, "loop_length": le - ls}
    aligned = ls + (m - ls % m)                                        # :29 GetNextMultiple
    count = le + (aligned - ls)                                        # :30-31
    frames = le // 14                                                  # :33
    return {"needed": True, "loop_start_aligned": aligned, "out_samples": count, "bytes_to_keep": frames * 8, "samples_to_keep": frames * 14,
            "samples_to_encode": count - frames * 14, "head": le - frames * 14, "loop_start": ls, "loop_length": le - ls}


def model(files, scratch_bytes=None):
    """files: GcFileC; the packed layout as a dict.  scratch_bytes: the encoder's scratch for n channels (None: not modelled)"""
    m = {"first_channel": [], "counts": [], "out_counts": [], "tail_counts": [], "entries": [], "seek_off": [], "rows": []}
    seek_at = 0
    for f in files:
        lay, a = channel_layout(f), alignment_numbers(f)
        assert (bool(lay.alignment_needed), lay.loop_start_aligned, lay.sample_count_aligned) == (a["needed"], a["loop_start_aligned"], a["out_samples"])
        m["first_channel"].append(len(m["counts"]))
        for _ in range(f.channels):
            m["counts"].append(f.channel.sample_count)
            m["out_counts"].append(lay.sample_count_aligned)
            if a["needed"]:
                m["tail_counts"].append(a["samples_to_encode"])
            m["entries"].append(lay.seek_table_entries)
            m["seek_off"].append(seek_at)
            m["rows"].append(a)
            seek_at += up(2 * lay.seek_table_entries, 8)
    for key, counts in (("in", m["counts"]), ("out", m["out_counts"]), ("tail", m["tail_counts"])):
        pcm_at = adpcm_at = 0
        m[key + "_pcm_off"], m[key + "_adpcm_off"] = [], []
        for n in counts:                                               # rows: 8 samples / 16 bytes (vga_gcadpcm_ragged_create)
            m[key + "_pcm_off"].append(pcm_at)
            m[key + "_adpcm_off"].append(adpcm_at)
            pcm_at += up(n, 8)
            adpcm_at += up(byte_count(n), 16)
        m[key + "_pcm_samples"], m[key + "_adpcm_bytes"] = pcm_at + 128, adpcm_at + 256
    m["seek_shorts"] = seek_at
    nt = len(m["tail_counts"])
    ws = m["in_pcm_samples"] * 2 if files else 0                       # the plain decode; then the tail batch, coefficients, histories, scratch
    if nt:
        ws += up(m["tail_pcm_samples"] * 2, 16) + up(m["tail_adpcm_bytes"], 16) + nt * 32 + 2 * up(nt * 2, 16)
        m["scratch_at"] = ws
        if scratch_bytes is not None:
            ws += up(scratch_bytes(nt), 16)
    m["workspace"] = ws
    return m


def item_range(keep, total, y):
    """[start, end) and granule of an assemble work item of a row of `total` bytes that keeps `keep`"""
    gran = 4 << (y >> 30)
    start = (y & 0x3FFFFFFF) << 2
    part_end = keep if start < keep else total
    return start, min(start + CHUNK * gran, part_end), gran


def emulate_gather(pcm, row):
    """the gather kernel's index arithmetic over one AlignRow, on the decoded PCM of the input row: (new_pcm, hist1, hist2)"""
    keep, head, ls, ll = row["samples_to_keep"], row["head"], row["loop_start"], row["loop_length"]
    out = np.zeros(row["samples_to_encode"], np.int16)
    for i in range(out.size):
        out[i] = pcm[keep + i] if i < head else pcm[ls + (i - head) % ll]
    return out, (int(pcm[keep - 1]) if keep >= 1 else 0), (int(pcm[keep - 2]) if keep >= 2 else 0)


# ---------------------------------------------------------------- the oracle's side, computed once per list of files
_pcm = []
_ref = {}


def source_pcm():
    if not _pcm:
        _pcm.append(po.synth_generate(64, 30000, first_channel=40))
    return _pcm[0]


def reference(tuples):
    """per file, per channel: the input (pcm, coefs, adpcm) and po.gc_build_channel's (rc, out adpcm, pcm, seek, ctx); the running
    channel index counts over `tuples`"""
    key = tuple(tuples)
    if key not in _ref:
        out, c = [], 0
        for nch, n, looping_, ls, le, spacing, multiple in tuples:
            p = po.gc_channel_params(n, bool(looping_), ls, le, multiple, spacing)
            chans = []
            for i in range(nch):
                x = np.resize(source_pcm()[(c + i) % 64], n) if n > 30000 else source_pcm()[(c + i) % 64, :n]
                coefs = po.gc_calculate_coefficients(x)
                adpcm = po.gc_encode(x, coefs)
                rc, lay, a, dec, seek, ctx = po.gc_build_channel(adpcm, coefs, p)
                chans.append({"x": x, "coefs": coefs, "adpcm": adpcm, "rc": rc, "out": a.copy(), "pcm": dec.copy(), "seek": seek.copy(),
                              "ctx": ctx.copy(), "plain": po.gc_decode(adpcm, coefs, n)})
            out.append(chans)
            c += nch
        _ref[key] = out
    return _ref[key]
