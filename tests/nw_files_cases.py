"""What tests/test_nw_files_host.py and tests/test_gpu_nw_files.py share: the files and configurations of the sets, a model of the
packed layout of include/vgaudio_hip/nw_files.h built from the PER-FILE size call of the library (vga_nwstm_layout_for) and the
rounding rules the header states, and the oracle's side of every channel (gc_aligned_cases.reference: the oracle's encode and
po.gc_build_channel with each file's layout.channel), computed once."""
import ctypes as C

import numpy as np

import gc_aligned_cases as ga
import nwstm_ref
from vgaudio_amd import _lib

RATE = 32000
RSTM, CSTM, FSTM = 0, 1, 2
# (channels, samples, looping, loop start, loop end): the loop the format's, before the writer aligns it
SMALL = [
    (1, 1, 0, 0, 0),
    (2, 28, 0, 0, 0),
    (3, 15, 0, 0, 0),
    (2, 100, 1, 15, 57),               # alignment 14: aligned count 70 < 100, the output row is shorter than the input row
    (2, 57, 0, 0, 0),                  # a file that does not loop between two that do
    (2, 100, 1, 14, 57),               # alignment 14: no re-encode, rows of 100 samples for 57 in the file: the interleave truncates
    (255, 15, 0, 0, 0),                # the largest channel info, 128 default tracks, the last one mono
    (1, 100, 1, 50, 100),              # alignment 64: aligned count 114
    (2, 0, 0, 0, 0),                   # no samples: headers, an empty seek table and an empty DATA block
]
# the default configuration's files: three blocks of 16-byte granules with a short last block padded to 0x20, and
# gc_aligned_cases' file whose tail is re-encoded under the default alignment
BIG = [(2, 2 * 14336 + 5, 0, 0, 0), (1, 30000, 1, 1, 30000), (1, 1, 0, 0, 0), (2, 0, 0, 0, 0)]

V = lambda major, minor: major << 24 | minor << 16


def config(target, spi=0, spe=0, align=0, track=0, seek=0, version=0, endianness=-1):
    return _lib.NwFileConfigC(target, spi, spe, align, track, seek, version, endianness)


# name -> (configuration, files).  Interleaves: 14 samples (8-byte granules), 28 (16-byte granules), the default.
CONFIGS = {
    "rstm": (config(RSTM, 14, 14, 14), SMALL),
    "rstm-short": (config(RSTM, 28, 5, 64, 1, 1), SMALL),        # short tracks, short seek table: zero fill past the source entries
    "rstm-default": (config(RSTM), BIG),
    "cstm-2.0": (config(CSTM, 14, 14, 14, version=V(2, 0)), SMALL),
    "cstm-2.1": (config(CSTM, 28, 14, 64, version=V(2, 1)), SMALL),
    "cstm-2.2-big": (config(CSTM, 14, 5, 64, version=V(2, 2), endianness=1), SMALL),
    "cstm-2.3": (config(CSTM, 0, 14, 14, version=V(2, 3)), SMALL),
    "fstm-0.2": (config(FSTM, 28, 14, 14, version=V(0, 2)), SMALL),
    "fstm-0.3-little": (config(FSTM, 14, 14, 64, version=V(0, 3), endianness=0), SMALL),
    "fstm-0.4": (config(FSTM, 14, 5, 14, version=V(0, 4)), SMALL),
    "fstm-0.5": (config(FSTM, 0, 0, 64, version=V(0, 5)), SMALL),
    "fstm-default": (config(FSTM), BIG),
}
CHUNK = 1024                                                           # granules / shorts of one work item


def nw_file(channels, samples, looping=0, loop_start=0, loop_end=0, rate=RATE):
    return _lib.NwFileC(channels, rate, samples, looping, loop_start, loop_end)


def files_of(tuples):
    return [nw_file(*t) for t in tuples]


def params_of(f, cfg):
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count = cfg.target, f.sample_rate, f.sample_count
    p.looping, p.loop_start, p.loop_end = f.looping, f.loop_start, f.loop_end
    p.samples_per_interleave, p.samples_per_seek_table_entry = cfg.samples_per_interleave, cfg.samples_per_seek_table_entry
    p.loop_point_alignment, p.track_type, p.seek_table_type = cfg.loop_point_alignment, cfg.track_type, cfg.seek_table_type
    p.version, p.endianness = cfg.version, cfg.endianness
    return p


def file_layout(f, cfg):
    """(rc, vga_nwstm_layout) of the per-file call"""
    lay, p = _lib.NwLayoutC(), params_of(f, cfg)
    return _lib.lib().vga_nwstm_layout_for(C.byref(p), f.channels, C.byref(lay)), lay


up = ga.up
byte_count = ga.byte_count


def model(files, cfg):
    """the packed layout as a dict, from the per-file layouts and the header's rounding rules"""
    m = {"first_channel": [], "counts": [], "entries": [], "seek_off": [], "adpcm_off": [], "image_off": [], "image_size": [], "layouts": []}
    seek_at = adpcm_at = pcm_at = image_at = 0
    for f in files:
        rc, lay = file_layout(f, cfg)
        assert rc == 0
        m["layouts"].append(lay)
        m["first_channel"].append(len(m["counts"]))
        for _ in range(f.channels):
            m["counts"].append(lay.channel_sample_count)
            m["entries"].append(lay.channel_seek_entries)
            m["seek_off"].append(seek_at)
            m["adpcm_off"].append(adpcm_at)
            seek_at += up(2 * lay.channel_seek_entries, 8)
            adpcm_at += up(lay.channel_adpcm_bytes, 16)                # rows: 8 samples / 16 bytes (vga_gcadpcm_ragged_create)
            pcm_at += up(lay.channel_sample_count, 8)
        assert lay.channel_adpcm_bytes == byte_count(lay.channel_sample_count)
        m["image_off"].append(image_at)
        m["image_size"].append(lay.file_size)
        image_at += up(lay.file_size, 16)
    m["seek_shorts"], m["adpcm_bytes"], m["pcm_samples"], m["image_bytes"] = seek_at, adpcm_at + 256, pcm_at + 128, image_at + 256
    return m


def gc_tuples(files, cfg):
    """gc_aligned_cases' tuples (channels, samples, looping, loop start, loop end, spacing, alignment) of the files: layout.channel"""
    out = []
    for f in files:
        ch = file_layout(f, cfg)[1].channel
        out.append((f.channels, ch.sample_count, ch.looping, ch.loop_start, ch.loop_end, ch.samples_per_seek_table_entry,
                    ch.loop_alignment_multiple))
    return out


def audio_item_range(geom, y):
    """[start, end) and granule of a writer's audio item over a file's audio region; geom: (input, interleave, output, channels)"""
    _, il, out, nch = geom
    gran = 16 if y >> 31 else 8
    start = (y & 0x7FFFFFFF) << 3
    total = out * nch
    boundary = (-(-out // il) - 1) * il * nch
    part_end = boundary if start < boundary else total
    return start, min(start + CHUNK * gran, part_end), gran


def reader_item_range(out, y):
    gran = 16 if y >> 31 else 8
    start = (y & 0x7FFFFFFF) << 3
    return start, min(start + CHUNK * gran, out), gran


def reference_image(f, cfg, lay, chans, gain=None, start=None, loop=None):
    """tests/nwstm_ref.build_image (the restatement of the reference's writers) for one file from the oracle's channels; None:
    the defaults of the device call's NULL pointers"""
    nch = f.channels
    adpcm = [bytes(c["out"]) for c in chans]
    coefs = [[int(v) for v in c["coefs"]] for c in chans]
    gain = [0] * nch if gain is None else gain
    start = [[a[0] if a else 0, 0, 0] for a in adpcm] if start is None else start
    loop = [[0, 0, 0]] * nch if loop is None else loop
    seek = [[int(v) for v in c["seek"]] for c in chans]
    spi = cfg.samples_per_interleave or nwstm_ref.DEFAULT
    spe = cfg.samples_per_seek_table_entry or nwstm_ref.DEFAULT
    version = None if cfg.target == RSTM else (cfg.version or None)
    big = None if cfg.endianness < 0 else bool(cfg.endianness)
    return nwstm_ref.build_image(cfg.target, f.sample_rate, nch, adpcm, coefs, gain, start, loop, seek, bool(lay.looping), lay.loop_start,
                                 lay.loop_end, lay.sample_count, spi, spe, bool(cfg.track_type), bool(cfg.seek_table_type), version, big)
