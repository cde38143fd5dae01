"""What tests/test_hps_files_host.py and tests/test_gpu_hps_files.py share: the files of the set (the smallest shapes at which
the block map can go wrong), a model of the packed layout of include/vgaudio_hip_files/hps_files.h built from
tests/gc_containers_ref.hps_layout (the restatement of HpsWriter's SetupWriter and CreateBlockMap) and the rounding rules the
header states, and the rows, tables and reference images of the set, computed once.

One block holds 0x20000 / nch' nibbles (nch' the padded channel size times the channels): 114 688 samples mono, 14 336 for 8
channels, 7 168 for 16 and 504 for 253, so files of several blocks stay small with 8 or more channels.  HPS cannot write 255
channels (255 % 4 == 3, refused): 253 is the largest count a set covers, and 255 stands among the refusals."""
import ctypes as C
import functools

import numpy as np

import gc_containers_ref as gr
from vgaudio_amd import _lib

RATE = 32000
CHUNK_BYTES = 16384                                                    # of one work item of 16-byte granules
CHUNK_BYTES1 = 1024                                                    # of one work item of the general form of the gather
# name -> (channels, samples, looping, loop start, loop end): the loop the format's, before the writer aligns it
FILES = {
    "short": (1, 5, 0, 0, 0),                  # shorter than one frame; one block only
    "full": (8, 14336, 0, 0, 0),               # exactly one full block
    "full+1": (8, 14337, 0, 0, 0),             # ... plus one sample: a last block of 3 nibbles (odd), min(left, ...) = left
    "blocks": (16, 7168 * 3 + 500, 0, 0, 0),   # four blocks without a loop: three full ones, then what is left
    "loop0": (8, 50000, 1, 0, 50000),          # a loop in block 0: every block comes from the even re-division
    "later": (8, 40000, 1, 28000, 40000),      # a loop in block 1 that the re-encode moves to 28672: the loop block is 2
    "on": (16, 30000, 1, 7168 * 2, 30000),     # a loop start already on the multiple, in a later block
    "align2": (2, 100, 1, 10, 90),             # the alignment of two channels: 57344 samples, a second block of a few bytes
    "wide": (253, 1200, 0, 0, 0),              # the largest channel count: blocks of 504 samples
    "four": (4, 300, 0, 0, 0),
    "five": (5, 1000, 0, 0, 0),
    "six": (6, 777, 1, 0, 777),
    "mono": (1, 120000, 1, 1000, 120000),      # mono over two blocks after its alignment (233 688 samples): several work items
}
ORDER = list(FILES)


def hps_file(channels, samples, looping=0, loop_start=0, loop_end=0, rate=RATE):
    return _lib.HpsFileC(channels, rate, samples, looping, loop_start, loop_end)


def files_of(tuples):
    return [hps_file(*t) for t in tuples]


def the_files():
    return files_of(FILES[k] for k in ORDER)


def params_of(f):
    return _lib.HpsParamsC(f.sample_rate, f.sample_count, f.looping, f.loop_start, f.loop_end)


def file_layout(f):
    """(rc, vga_hps_layout) of the per-file call"""
    lay, p = _lib.HpsLayoutC(), params_of(f)
    return _lib.lib().vga_hps_layout_for(C.byref(p), f.channels, C.byref(lay)), lay


def block_map(f):
    rc, lay = file_layout(f)
    assert rc == 0
    blocks, p = (_lib.HpsBlockC * lay.block_count)(), params_of(f)
    assert _lib.lib().vga_hps_block_map(C.byref(p), f.channels, blocks, lay.block_count) == 0
    return lay, list(blocks)


def up(v, m):
    return -(-v // m) * m


def ref_layout(f):
    lay = gr.hps_layout(f.channels, f.sample_count, bool(f.looping), f.loop_start, f.loop_end)
    lay["channel_sample_count"] = gr.aligned_loop(bool(f.looping), f.loop_start, f.loop_end, f.sample_count, lay["alignment"])[3]
    lay["block_header_size"] = up(12 + 8 * f.channels, 0x20)
    return lay


def model(files):
    """the packed layout as a dict, from gc_containers_ref's layouts and the header's rounding rules"""
    m = {"first_channel": [], "counts": [], "adpcm_off": [], "pcm_off": [], "image_off": [], "image_size": [], "first_block": [],
         "layouts": []}
    adpcm_at = pcm_at = image_at = blocks = 0
    for f in files:
        lay = ref_layout(f)
        m["layouts"].append(lay)
        m["first_channel"].append(len(m["counts"]))
        m["first_block"].append(blocks)
        blocks += len(lay["blocks"])
        for _ in range(f.channels):
            m["counts"].append(lay["channel_sample_count"])
            m["adpcm_off"].append(adpcm_at)
            m["pcm_off"].append(pcm_at)
            adpcm_at += up(gr.bytes_of(lay["channel_sample_count"]), 16)   # rows: 8 samples / 16 bytes (vga_gcadpcm_ragged_create)
            pcm_at += up(lay["channel_sample_count"], 8)
        m["image_off"].append(image_at)
        m["image_size"].append(lay["file_size"])
        image_at += up(lay["file_size"], 16)
    m["adpcm_bytes"], m["pcm_samples"], m["image_bytes"], m["blocks"] = adpcm_at + 256, pcm_at + 128, image_at + 256, blocks
    return m


@functools.lru_cache(maxsize=None)
def inputs():
    """the aligned rows of every channel of the set (any bytes: the writer moves them), the PCM rows, the per-channel tables, and
    per file the image gc_containers_ref.hps_image makes of them with the tables given and with the defaults of the NULL
    pointers.  Computed once; callers do not modify it."""
    files = the_files()
    m = model(files)
    nch = len(m["counts"])
    rng = np.random.default_rng(12)
    rows = [rng.integers(0, 256, gr.bytes_of(n), dtype=np.uint8) for n in m["counts"]]
    pcm = [rng.integers(-32768, 32768, n).astype(np.int16) for n in m["counts"]]
    coefs = rng.integers(-32768, 32768, (nch, 16)).astype(np.int16)
    gain = rng.integers(-3000, 3000, nch).astype(np.int16)
    start = rng.integers(-30000, 30000, (nch, 3)).astype(np.int16)
    given, nulls, c = [], [], 0
    for f in files:
        k = f.channels
        a = [bytes(r) for r in rows[c:c + k]]
        args = (bool(f.looping), f.loop_start, f.loop_end, f.sample_count)
        given.append(gr.hps_image(f.sample_rate, a, coefs[c:c + k].tolist(), gain[c:c + k].tolist(), start[c:c + k].tolist(),
                                  pcm[c:c + k], *args))
        nulls.append(gr.hps_image(f.sample_rate, a, coefs[c:c + k].tolist(), [0] * k, [[r[0], 0, 0] for r in a], None, *args))
        c += k
    return {"files": files, "model": m, "rows": rows, "pcm": pcm, "coefs": coefs, "gain": gain, "start": start, "given": given,
            "nulls": nulls}


def parse(image):
    """vga_hps_parse of one image (bytes or a uint8 array): (info, block table)"""
    buf = np.frombuffer(bytes(image), dtype=np.uint8)
    info = _lib.HpsInfoC()
    _lib.check(_lib.lib().vga_hps_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), None, 0))
    blocks = (_lib.HpsBlockInfoC * max(info.block_count, 1))()
    _lib.check(_lib.lib().vga_hps_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), blocks, info.block_count))
    return info, blocks


def foreign_image(nch, sizes, stride_pad=0, seed=3):
    """an HPS file no writer here makes: blocks of sizes[i] nibbles per channel (any numbers, so that block audio lands on odd
    row offsets) whose channels lie next_multiple(bytes, 0x20) + stride_pad apart; returns (bytes, the per-channel rows
    gc_containers_ref.hps_parse reads out of it)"""
    import struct
    rng = np.random.default_rng(seed)
    header = up(max(0x80, 0x10 + 0x38 * nch), 0x20)
    nbytes = sum((s + 1) // 2 for s in sizes)
    samples = next(s for s in range(nbytes * 2) if gr.bytes_of(s) == nbytes)       # the rows are the header's sample count's
    out = bytearray(header)
    struct.pack_into(">8sii", out, 0, b" HALPST\0", RATE, nch)
    for c in range(nch):
        struct.pack_into(">iiii16hh3h", out, 16 + 0x38 * c, 0x10000, 2, gr.sample_to_nibble(samples - 1), 2,
                         *[int(v) for v in rng.integers(-2048, 2048, 16)], c, 1 + c, 2, 3)
    for i, size in enumerate(sizes):
        n = (size + 1) // 2
        stride = up(n, 0x20) + stride_pad
        at = len(out)
        block_header = up(12 + 8 * nch, 0x20)
        body = rng.integers(0, 256, stride * nch, dtype=np.uint8).tobytes()
        nxt = at + block_header + len(body) if i + 1 < len(sizes) else -1
        head = bytearray(block_header)
        struct.pack_into(">iii", head, 0, stride * nch, size - 1, nxt)
        out += head + body
    return bytes(out), gr.hps_parse(bytes(out))["audio"]
