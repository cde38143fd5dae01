"""The files of tests/test_nw_pcm_files_host.py and tests/test_gpu_nw_pcm_files.py (include/vgaudio_hip_files/nw_pcm_files.h):
the cases as (channels, samples, looping, loop start, loop end) at the smallest shapes at which the addressing can go wrong, the
configurations by name, seeded noise for the rows, the images from tests/nwstm_pcm_ref.py's restatement of the reference's
writers, and the model of the set's layout (tests/wave_files_cases.py's: the rounding rules are the same)."""
import ctypes as C

import numpy as np

import nwstm_pcm_ref as ref
from vgaudio_amd import _lib
from wave_files_cases import explicit_pcm_offsets, image_offsets_at, model, up  # noqa: F401  (the same rounding rules)

HEADER_ITEM, VECTOR, GENERAL = 0, 1, 2
COPY, SWAP16, PCM8_CONV = 0, 1, 2
PCM8, PCM16 = ref.PCM8, ref.PCM16
RSTM, CSTM, FSTM = ref.RSTM, ref.CSTM, ref.FSTM
LITTLE, BIG_ENDIAN = 0, 1
CHUNK_BYTES = 1024 * 16
RATE = 32000

# (channels, samples, looping, loop start, loop end)
SMALL = [(1, 1, 0, 0, 0), (2, 28, 0, 0, 0), (3, 15, 0, 0, 0),
         (2, 100, 1, 15, 57),                                 # the row holds 100 samples, the file stores 57: the cut falls inside a block
         (2, 57, 0, 0, 0),                                    # between two looping files
         (1, 100, 1, 50, 100),
         (255, 15, 0, 0, 0),                                  # the largest channel info: 128 default tracks, the last one mono
         (2, 0, 0, 0, 0)]                                     # headers and an empty DATA block
LONG = (2, 70001, 1, 7, 69990)                                # spans more than one work item
MID = (1, 2500, 0, 0, 0)                                      # more than two interleaves of 1001 samples


def big(codec):
    """two whole blocks at the default interleave plus a short last block padded to 0x20"""
    return [(2, 2 * 4096 + 5, 0, 0, 0) if codec == PCM16 else (2, 2 * 8192 + 3, 0, 0, 0), (1, 1, 0, 0, 0), (2, 0, 0, 0, 0)]


# name -> (target, codec, endianness or None, packed version or 0, samples per interleave or 0, cases)
CONFIGS = {
    "rstm16_i8": (RSTM, PCM16, None, 0, 8, SMALL),
    "rstm8_i16": (RSTM, PCM8, None, 0, 16, SMALL),
    "rstm16_i5": (RSTM, PCM16, None, 0, 5, SMALL + [LONG]),
    "rstm16_default": (RSTM, PCM16, None, 0, 0, big(PCM16) + [LONG]),
    "rstm8_default": (RSTM, PCM8, None, 0, 0, big(PCM8)),
    "cstm16_le_i16": (CSTM, PCM16, LITTLE, 0x02010000, 16, SMALL),
    "cstm8_le_i32": (CSTM, PCM8, LITTLE, 0x02010000, 32, SMALL),
    "cstm16_be_i8": (CSTM, PCM16, BIG_ENDIAN, 0x02010000, 8, SMALL),
    "cstm8_be_i1001": (CSTM, PCM8, BIG_ENDIAN, 0x02010000, 1001, SMALL + [MID, LONG]),
    "cstm16_le_default": (CSTM, PCM16, LITTLE, 0x02010000, 0, big(PCM16) + [LONG]),
    "fstm16_be_default": (FSTM, PCM16, BIG_ENDIAN, 0x00030000, 0, big(PCM16)),
    "fstm8_be_default": (FSTM, PCM8, BIG_ENDIAN, 0x00030000, 0, big(PCM8) + [LONG]),
    "fstm16_le_i5": (FSTM, PCM16, LITTLE, 0x00030000, 5, SMALL + [LONG]),
    "fstm8_le_i16": (FSTM, PCM8, LITTLE, 0x00030000, 16, SMALL),
}
REFUSED_VERSIONS = {"cstm_2_3": (CSTM, 0x02030000), "fstm_0_4": (FSTM, 0x00040000)}


def config_c(name):
    """(vga_nw_file_config, codec) of a named configuration"""
    target, codec, endian, version, spi, _ = CONFIGS[name]
    return _lib.NwFileConfigC(target, spi, 0, 0, 0, 0, version, -1 if endian is None else endian), codec


def files_of(cases):
    return [_lib.NwFileC(nch, RATE, n, looping, ls, le) for nch, n, looping, ls, le in cases]


def counts_of(cases):
    return [[c[1]] * c[0] for c in cases]


def big_endian(name):
    target, _, endian, _, _, _ = CONFIGS[name]
    return target == RSTM or (endian == BIG_ENDIAN if endian is not None else target == FSTM)


def conv_of(name):
    return PCM8_CONV if CONFIGS[name][1] == PCM8 else SWAP16 if big_endian(name) else COPY


_rows, _images = {}, {}


def rows_of(cases):
    """seeded noise, one int16 array per row of the cases, computed once per list and never changed"""
    key = tuple(cases)
    if key not in _rows:
        rng = np.random.default_rng(0x9C3F + len(cases))
        rows = [rng.integers(-32768, 32768, n).astype(np.int16) for nch, n, _, _, _ in cases for _ in range(nch)]
        for r in rows:
            r.setflags(write=False)
        _rows[key] = rows
    return _rows[key]


def reference(name):
    """(cases, rows, images) of a named configuration: the image of every file from the restatement of the reference's writers,
    computed once and never changed"""
    target, codec, endian, version, spi, cases = CONFIGS[name]
    rows = rows_of(cases)
    if name not in _images:
        images, c = [], 0
        for nch, n, looping, ls, le in cases:
            mine = rows[c:c + nch]
            stored = mine if codec == PCM16 else [ref.encode_signed(r) for r in mine]
            raw = ref.build_image(target, codec, RATE, stored, bool(looping), ls, le, spi or None, version=version or None,
                                  big=big_endian(name))
            images.append(np.frombuffer(bytes(raw), np.uint8))
            c += nch
        _images[name] = images
    return cases, rows, _images[name]


def row_as_read(row, codec, stored):
    """what a reader gives for a row that went through a file that stores `stored` samples of it"""
    row = np.asarray(row, np.int16)[:stored]
    return row if codec == PCM16 else ref.decode_signed(ref.encode_signed(row))


def parse(image):
    info = _lib.NwInfoC()
    data = np.ascontiguousarray(image, dtype=np.uint8)
    _lib.check(_lib.lib().vga_nwstm_pcm_parse(data.ctypes.data_as(C.POINTER(C.c_uint8)), len(data), C.byref(info)))
    return info


def mixed_read_side():
    """(images, codecs): BRSTM PCM16, BCSTM PCM8 and BFSTM PCM16 little-endian files for ONE set for reading"""
    images, codecs = [], []
    for name in ("rstm16_i8", "cstm8_le_i32", "fstm16_le_i5", "rstm16_default", "fstm8_be_default"):
        _, _, mine = reference(name)
        images += mine
        codecs += [CONFIGS[name][1]] * len(mine)
    return images, codecs
