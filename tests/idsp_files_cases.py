"""What tests/test_idsp_files_host.py and tests/test_gpu_idsp_files.py share: the files and configurations of the sets (the
smallest shapes at which each branch can go wrong), a model of the packed layout of include/vgaudio_hip_files/idsp_files.h built
from tests/gc_containers_ref.idsp_layout (the restatement of IdspWriter's size math) and the rounding rules the header states,
and the rows, tables and reference images of a set, computed once."""
import ctypes as C
import functools

import numpy as np

import gc_containers_ref as gr
from vgaudio_amd import _lib

RATE = 32000
CHUNK = 1024                                                           # granules of one work item
# (channels, samples, looping, loop start, loop end): the loop the format's, before the writer aligns it
FILES = [
    (1, 1, 0, 0, 0),                   # shorter than one frame
    (2, 100, 1, 15, 57),               # the loop start needs alignment under every block size but 0
    (2, 100, 1, 28, 57),               # on the multiple of 8 and 0x10: no re-encode; trimmed, the rows are longer than the audio
    (4, 57, 0, 0, 0),
    (5, 15, 0, 0, 0),
    (6, 300, 1, 0, 300),
    (8, 29, 0, 0, 0),                  # 18 bytes: the last block of a row is shorter than an interleave of 8 or 0x10
    (16, 14, 0, 0, 0),
    (255, 15, 0, 0, 0),                # the largest header
    (1, 40000, 1, 100, 39000),         # several work items
    # no samples: a header and no audio (refused with block size 0).  It loops over nothing so that its end address is
    # SampleToNibble(0): without a loop it is SampleToNibble(-1), which C# (and the library) truncate to 1 and
    # gc_containers_ref's floor division makes -1
    (2, 0, 1, 0, 0),
]
# name -> (block size, trim, files)
CONFIGS = {
    "b0": (0, 1, FILES[:-1]),          # not interleaved: one block, 8-byte granules where the frames are odd
    "b0-keep": (0, 0, FILES[:-1]),
    "b8": (8, 1, FILES),               # 8-byte granules throughout
    "b16": (0x10, 1, FILES),           # the reference's default
    "b16-keep": (0x10, 0, FILES),
    "b4000": (0x4000, 1, FILES),       # every row is shorter than one block; alignment to 28672 samples
}


def config(block_size, trim=1):
    return _lib.IdspFileConfigC(block_size, trim)


def config_of(name):
    return config(*CONFIGS[name][:2])


def idsp_file(channels, samples, looping=0, loop_start=0, loop_end=0, rate=RATE):
    return _lib.IdspFileC(channels, rate, samples, looping, loop_start, loop_end)


def files_of(tuples):
    return [idsp_file(*t) for t in tuples]


def params_of(f, cfg):
    return _lib.IdspParamsC(f.sample_rate, f.sample_count, f.looping, f.loop_start, f.loop_end, cfg.block_size, cfg.trim_file)


def file_layout(f, cfg):
    """(rc, vga_idsp_layout) of the per-file call"""
    lay, p = _lib.IdspLayoutC(), params_of(f, cfg)
    return _lib.lib().vga_idsp_layout_for(C.byref(p), f.channels, C.byref(lay)), lay


def up(v, m):
    return -(-v // m) * m


def ref_layout(f, cfg):
    return gr.idsp_layout(f.channels, f.sample_count, bool(f.looping), f.loop_start, f.loop_end, cfg.block_size, bool(cfg.trim_file))


def model(files, cfg):
    """the packed layout as a dict, from gc_containers_ref's layouts and the header's rounding rules"""
    m = {"first_channel": [], "counts": [], "adpcm_off": [], "pcm_off": [], "image_off": [], "image_size": [], "layouts": []}
    adpcm_at = pcm_at = image_at = 0
    for f in files:
        lay = ref_layout(f, cfg)
        m["layouts"].append(lay)
        m["first_channel"].append(len(m["counts"]))
        for _ in range(f.channels):
            m["counts"].append(lay["channel_sample_count"])
            m["adpcm_off"].append(adpcm_at)
            m["pcm_off"].append(pcm_at)
            adpcm_at += up(gr.bytes_of(lay["channel_sample_count"]), 16)   # rows: 8 samples / 16 bytes (vga_gcadpcm_ragged_create)
            pcm_at += up(lay["channel_sample_count"], 8)
        m["image_off"].append(image_at)
        m["image_size"].append(lay["file_size"])
        image_at += up(lay["file_size"], 16)
    m["adpcm_bytes"], m["pcm_samples"], m["image_bytes"] = adpcm_at + 256, pcm_at + 128, image_at + 256
    return m


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the aligned rows of every channel of a set (any bytes: the writer moves them), the per-channel tables, and per file the
    image gc_containers_ref.idsp_image makes of them with the tables given and with the defaults of the NULL pointers.
    Computed once; callers do not modify it."""
    block, trim, tuples = CONFIGS[name]
    cfg, files = config(block, trim), files_of(tuples)
    m = model(files, cfg)
    nch = len(m["counts"])
    rng = np.random.default_rng(11)
    rows = [rng.integers(0, 256, gr.bytes_of(n), dtype=np.uint8) for n in m["counts"]]
    coefs = rng.integers(-32768, 32768, (nch, 16)).astype(np.int16)
    gain = rng.integers(-3000, 3000, nch).astype(np.int16)
    start = rng.integers(-30000, 30000, (nch, 3)).astype(np.int16)
    loop = rng.integers(-30000, 30000, (nch, 3)).astype(np.int16)
    given, nulls, c = [], [], 0
    for f, lay in zip(files, m["layouts"]):
        k = f.channels
        a = [bytes(r) for r in rows[c:c + k]]
        args = (bool(f.looping), f.loop_start, f.loop_end, f.sample_count, block, bool(trim))
        given.append(gr.idsp_image(f.sample_rate, a, coefs[c:c + k].tolist(), gain[c:c + k].tolist(), start[c:c + k].tolist(),
                                   loop[c:c + k].tolist(), *args))
        nulls.append(gr.idsp_image(f.sample_rate, a, coefs[c:c + k].tolist(), [0] * k, [[r[0] if r else 0, 0, 0] for r in a],
                                   [[0, 0, 0]] * k, *args))
        c += k
    return {"cfg": cfg, "files": files, "model": m, "rows": rows, "coefs": coefs, "gain": gain, "start": start, "loop": loop,
            "given": given, "nulls": nulls}


def parse(image):
    """vga_idsp_parse of one image (bytes or a uint8 array)"""
    buf = np.frombuffer(bytes(image), dtype=np.uint8)
    info = _lib.IdspInfoC()
    _lib.check(_lib.lib().vga_idsp_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info)))
    return info


def foreign_image(nch, il, length, samples, pad=0, seed=3):
    """an IDSP file no writer here makes: `length` bytes per channel in blocks of `il` (any numbers), `pad` bytes between the
    channel infos and the audio; returns (bytes, the per-channel rows gc_containers_ref.idsp_parse reads out of it)"""
    import struct
    rng = np.random.default_rng(seed)
    audio_offset = 0x40 + 0x60 * nch + pad
    out = bytearray(audio_offset + nch * length)
    struct.pack_into(">4siiiiiiiiiii", out, 0, b"IDSP", 0, nch, RATE, samples, 0, 0, il, 0x40, 0x60, audio_offset, length)
    for c in range(nch):
        struct.pack_into(">iiihhiii16hh3h3h", out, 0x40 + 0x60 * c, samples, gr.sample_count_to_nibble_count(samples), RATE, 0, 0, 2,
                         gr.sample_to_nibble(max(samples - 1, 0)), 2, *[int(v) for v in rng.integers(-2048, 2048, 16)], c, 1 + c, 2, 3, 0, 0, 0)
    out[audio_offset:] = rng.integers(0, 256, nch * length, dtype=np.uint8).tobytes()
    return bytes(out), gr.idsp_parse(bytes(out))["audio"]
