"""What tests/test_gc_files_host.py and tests/test_gpu_gc_files.py share: the set of twelve files, the configurations, and a
model of the packed layout of include/vgaudio_hip/gc_files.h built from the PER-FILE size calls of the library
(vga_gcadpcm_channel_layout_for, vga_dsp_layout_for) and the rounding rules the headers state."""
import ctypes as C

from vgaudio_amd import _lib

RATE = 32000
# (channels, samples, looping, loop start, loop end, samples per seek entry): the smallest shapes at which each branch can go wrong
FILES = [
    (1, 1, 0, 0, 0, 14),
    (2, 13, 0, 0, 0, 14),
    (2, 14, 1, 0, 14, 14),
    (3, 15, 1, 1, 15, 14),
    (2, 29, 1, 2, 20, 14),
    (6, 43, 1, 14, 43, 28),
    (2, 100, 1, 15, 57, 14),
    (1, 57, 1, 30, 40, 0x3800),
    (2, 0, 0, 0, 0, 14),
    (2, 100, 1, 15, 57, 0),
    (1, 100, 1, 15, 57, 14),
    (255, 15, 0, 0, 0, 14),
]
# (samples per interleave, loop point alignment); each runs with trim_file 1 and 0
CONFIGS = {"blocks8": (14, 1), "blocks16": (28, 1), "oneblock": (0x3800, 1), "align4": (0x3800, 4)}
CHUNK_GRANULES = 1024                                                  # granules of one audio work item (gc_files_host.hpp)
CHUNK_ENTRIES = 1024


def gc_file(channels, samples, looping, loop_start, loop_end, spacing, alignment=0, rate=RATE):
    return _lib.GcFileC(channels, rate, _lib.GcChannelParamsC(samples, looping, loop_start, loop_end, alignment, spacing))


def config(samples_per_interleave, alignment, trim):
    return _lib.DspFileConfigC(samples_per_interleave, alignment, trim)


def byte_count(samples):
    return _lib.lib().vga_gcadpcm_sample_count_to_byte_count(samples)


def up(v, m):
    return (v + m - 1) // m * m


def dsp_layout(f, cfg):
    """vga_dsp_layout_for of one file under the set's configuration: (rc, DspLayoutC)"""
    ch = f.channel
    p = _lib.DspParamsC(f.sample_rate, ch.sample_count, ch.looping, ch.loop_start, ch.loop_end, cfg.samples_per_interleave,
                        cfg.loop_point_alignment, cfg.trim_file)
    out = _lib.DspLayoutC()
    return _lib.lib().vga_dsp_layout_for(C.byref(p), f.channels, C.byref(out)), out


def model(files, cfg=None):
    """files: GcFileC; the packed layout as a dict"""
    m = {"first_channel": [], "counts": [], "entries": [], "pcm_off": [], "adpcm_off": [], "seek_off": [], "image_off": [],
         "image_size": [], "geom": []}
    pcm_at = adpcm_at = seek_at = image_at = 0
    for f in files:
        lay = _lib.GcChannelLayoutC()
        assert _lib.lib().vga_gcadpcm_channel_layout_for(C.byref(f.channel), C.byref(lay)) == 0 and not lay.alignment_needed
        m["first_channel"].append(len(m["counts"]))
        n = f.channel.sample_count
        for _ in range(f.channels):
            m["counts"].append(n)
            m["entries"].append(lay.seek_table_entries)
            m["pcm_off"].append(pcm_at)
            m["adpcm_off"].append(adpcm_at)
            m["seek_off"].append(seek_at)
            pcm_at += up(n, 8)                                         # rows: 8 samples / 16 bytes (vga_gcadpcm_ragged_create)
            adpcm_at += up(byte_count(n), 16)
            seek_at += up(2 * lay.seek_table_entries, 8)
        if cfg is not None:
            rc, d = dsp_layout(f, cfg)
            assert rc == 0
            m["image_off"].append(image_at)
            m["image_size"].append(d.file_size)
            image_at += up(d.file_size, 16)
            mono = f.channels == 1
            m["geom"].append({"input": byte_count(n), "output": d.audio_data_size, "channels": f.channels,
                              "interleave": up(max(byte_count(n), 1), 16) if mono else d.bytes_per_interleave, "layout": d})
    m["pcm_samples"], m["adpcm_bytes"], m["seek_shorts"] = pcm_at + 128, adpcm_at + 256, seek_at
    m["image_bytes"] = image_at + 256 if cfg is not None else 0
    m["workspace"] = (pcm_at + 128) * 2 if files else 0
    return m


def writer_granules(g):
    """(full blocks, last block): the granule the geometry allows.  A 16-byte granule needs every run it copies to start on a
    16-byte boundary on both sides: blocks of a multiple of 16 bytes and, in the last block, rows a multiple of 16 apart; a
    single channel is one run from a 16-byte boundary to a 16-byte boundary"""
    if g["channels"] == 1:
        return 16, 16
    out_blocks = -(-g["output"] // g["interleave"]) if g["output"] else 0
    last_out = g["output"] - (out_blocks - 1) * g["interleave"] if out_blocks else 0
    full = 16 if g["interleave"] % 16 == 0 else 8
    return full, 16 if full == 16 and last_out % 16 == 0 else 8


def item_range(g, y, reader=False):
    """[start, end) and granule of an audio work item of a file of geometry g"""
    gran = 16 if y >> 31 else 8
    start = (y & 0x7FFFFFFF) << 3
    if reader:
        part_end = g["output"]
    else:
        total = g["output"] * g["channels"]
        out_blocks = -(-g["output"] // g["interleave"])
        boundary = (out_blocks - 1) * g["interleave"] * g["channels"]
        part_end = boundary if start < boundary else total
    return start, min(start + CHUNK_GRANULES * gran, part_end), gran
