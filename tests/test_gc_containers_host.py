"""HPS, IDSP and GENH size math and parsing (host only, no GPU): vga_hps_layout_for / vga_hps_block_map and
vga_idsp_layout_for against known answers and the independent restatement in gc_containers_ref.py; the parsers on
restatement-built images and on broken ones."""
import ctypes as C
import random
import struct

import numpy as np
import pytest

import gc_containers_ref as ref
from vgaudio_amd import _lib

OK, ARG, RANGE, DATA, OP = 0, -1, -2, -3, -4


def hps_layout(nch, n, looping=False, ls=0, le=0):
    p = _lib.HpsParamsC(48000, n, int(looping), ls, le)
    L = _lib.HpsLayoutC()
    rc = _lib.lib().vga_hps_layout_for(C.byref(p), nch, C.byref(L))
    if rc:
        return rc, L, []
    blocks = (_lib.HpsBlockC * L.block_count)()
    assert _lib.lib().vga_hps_block_map(C.byref(p), nch, blocks, L.block_count) == OK
    return rc, L, [{k: getattr(b, k) for k, _ in _lib.HpsBlockC._fields_} for b in blocks]


def idsp_layout(nch, n, looping=False, ls=0, le=0, block_size=0x10, trim=True):
    p = _lib.IdspParamsC(48000, n, int(looping), ls, le, block_size, int(trim))
    L = _lib.IdspLayoutC()
    return _lib.lib().vga_idsp_layout_for(C.byref(p), nch, C.byref(L)), L


# ---------------------------------------------------------------- HPS layout
# hand-derived from HpsWriter.cs:22-47,114-185: 48 000 samples, no loop
HPS_KAT = [
    # nch, header, channel size, alignment, blocks, file size
    # 48 000 samples = 3428 frames + 8 samples = 27 429 bytes = 54 858 nibbles per channel
    (1, 0x80, 0x10000, 114688, 1, 0x80 + 0x20 + 27456),
    (2, 0x80, 0x8000, 57344, 1, 0x80 + 0x20 + 2 * 27456),
    # 2 blocks of 32 768 + 22 090 nibbles; block headers of 4 + 8 * 4 -> 0x40 bytes
    (4, 0x100, 0x4000, 28672, 2, 0x100 + 2 * 0x40 + 4 * 0x4000 + 4 * 11072),
]


@pytest.mark.parametrize("nch,header,cs,align,nblocks,size", HPS_KAT)
def test_hps_layout_known_answers(nch, header, cs, align, nblocks, size):
    rc, L, blocks = hps_layout(nch, 48000)
    assert rc == OK
    assert (L.header_size, L.channel_size, L.alignment, L.block_count, L.file_size) == (header, cs, align, nblocks, size)
    assert blocks[0]["offset"] == header and blocks[-1]["next_offset"] == -1
    assert L.channel_adpcm_bytes == ref.bytes_of(48000) == 27429


CASES = [
    # samples, looping, loop start, loop end
    (1, False, 0, 0),
    (14, False, 0, 0),
    (48000, False, 0, 0),
    (48000, True, 0, 48000),                 # loop in the first block
    (48000, True, 1234, 40000),              # a loop that needs alignment
    (300000, True, 280000, 300000),          # loop in the last block (after alignment)
    (300000, True, 14336, 299999),
]


@pytest.mark.parametrize("nch", [1, 2, 4, 5, 8, 254])
@pytest.mark.parametrize("n,looping,ls,le", CASES)
def test_hps_layout_against_restatement(nch, n, looping, ls, le):
    rc, L, blocks = hps_layout(nch, n, looping, ls, le)
    assert rc == OK
    R = ref.hps_layout(nch, n, looping, ls, le)
    assert (L.header_size, L.channel_size, L.alignment, L.loop_start, L.loop_end, L.sample_count, L.loop_block,
            L.file_size) == (R["header_size"], R["channel_size"], R["alignment"], R["loop_start"], R["loop_end"],
                             R["sample_count"], R["loop_block"], R["file_size"])
    assert blocks == R["blocks"]
    assert L.alignment_needed == int(bool(looping and ls % L.alignment))
    assert L.block_header_size == ref.next_multiple(12 + 8 * nch, 0x20)


def test_hps_exactly_one_block_and_one_block_plus_a_frame():
    # 2 channels: 0x8000 bytes = 0x10000 nibbles = 57344 samples per channel per block
    _, L, blocks = hps_layout(2, 57344)
    assert L.block_count == 1 and blocks[0]["channel_size"] == 0x8000 and blocks[0]["end_nibble"] == 0xffff
    _, L, blocks = hps_layout(2, 57344 + 14)
    assert L.block_count == 2 and blocks[1]["channel_size"] == 8 and blocks[1]["start_sample"] == 57344


def test_hps_loop_points_back_to_the_loop_block():
    _, L, blocks = hps_layout(2, 300000, True, 114688, 300000)
    assert L.loop_block == 2 and L.alignment_needed == 0
    assert blocks[-1]["next_offset"] == blocks[2]["offset"]
    assert blocks[2]["start_sample"] == 114688


@pytest.mark.parametrize("nch", [3, 7, 11, 255])
def test_hps_channel_counts_the_reference_cannot_write(nch):
    rc, L, _ = hps_layout(nch, 48000)
    assert rc == (OP if nch % 4 == 3 else OK)
    if nch % 4 == 3 and nch < 255:
        assert "overrun" in _lib.lib().vga_last_error().decode()
        # the restatement's BinaryWriter over byte[FileSize] indeed runs off the end
        rows = [bytes(ref.bytes_of(48000))] * nch
        with pytest.raises(ref.CannotWrite):
            ref.hps_image(48000, rows, [[0] * 16] * nch, [0] * nch, [[0, 0, 0]] * nch, None, unaligned_count=48000)


def test_hps_layout_errors():
    assert hps_layout(0, 100)[0] == ARG
    assert hps_layout(256, 100)[0] == OP
    assert hps_layout(2, 0)[0] == RANGE                   # no block: blocks[0] of an empty map
    assert hps_layout(2, 100, True, 50, 200)[0] == RANGE
    assert hps_layout(2, 100, True, 60, 50)[0] == RANGE
    p = _lib.HpsParamsC(48000, 48000, 0, 0, 0)
    assert _lib.lib().vga_hps_block_map(C.byref(p), 2, None, 0) == ARG


# ---------------------------------------------------------------- IDSP layout
# IdspTests.IdspAlignsLoopToBlock (IdspTests.cs:20-36)
@pytest.mark.parametrize("loops,start_in,end_in,start_out,end_out,block_size", [
    (True, 1234, 2000, 1260, 2026, 0x10),
    (True, 1248, 2014, 1260, 2026, 0x10),
    (True, 1234, 2000, 1274, 2040, 0x38),
    (True, 1274, 2040, 1274, 2040, 0x38),
    (False, 0, 0, 0, 0, 0x10),
])
def test_idsp_aligns_loop_to_block(loops, start_in, end_in, start_out, end_out, block_size):
    rc, L = idsp_layout(2, 48000, loops, start_in, end_in, block_size)
    assert rc == OK
    assert (L.loop_start, L.loop_end) == (start_out, end_out)


@pytest.mark.parametrize("nch", [1, 2, 3, 8])
@pytest.mark.parametrize("block_size", [0, 0x10, 0x38, 0x800])
@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("n,looping,ls,le", [(48000, False, 0, 0), (48000, True, 1234, 40000), (48000, True, 14 * 100, 47000),
                                             (1, False, 0, 0)])
def test_idsp_layout_against_restatement(nch, block_size, trim, n, looping, ls, le):
    rc, L = idsp_layout(nch, n, looping, ls, le, block_size, trim)
    assert rc == OK
    R = ref.idsp_layout(nch, n, looping, ls, le, block_size, trim)
    got = dict(loop_start=L.loop_start, loop_end=L.loop_end, sample_count=L.sample_count,
               channel_sample_count=L.channel_sample_count, audio_data_size=L.audio_data_size, interleave=L.interleave_size,
               header_size=L.header_size, file_size=L.file_size, start_addr=L.start_addr, end_addr=L.end_addr)
    assert got == R


def test_idsp_layout_errors():
    assert idsp_layout(2, 100, block_size=-8)[0] == RANGE
    assert idsp_layout(2, 100, block_size=12)[0] == RANGE
    assert idsp_layout(2, 0, block_size=0)[0] == OP       # Interleave divides by the zero interleave
    assert idsp_layout(256, 100)[0] == OP
    assert idsp_layout(2, 100, True, 10, 200)[0] == RANGE


def test_idsp_configuration_block_size_setter():
    from vgaudio_amd.idsp import IdspConfiguration
    assert IdspConfiguration().BlockSize == 0x10
    for bad in (-8, 4, 0x11):
        with pytest.raises(_lib.ArgumentOutOfRangeError):
            IdspConfiguration(BlockSize=bad)
    c = IdspConfiguration(BlockSize=0)
    c.RecalculateLoopContext = False
    assert c.BlockSize == 0


# ---------------------------------------------------------------- parsing
def rows(nch, nbytes, seed):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(nbytes)) for _ in range(nch)]


def coefs(nch, seed):
    rng = random.Random(seed)
    return [[rng.randrange(-32768, 32768) for _ in range(16)] for _ in range(nch)]


def hps_file(nch, n, looping=False, ls=0, le=0, seed=1):
    R = ref.hps_layout(nch, n, looping, ls, le)
    adpcm = rows(nch, ref.bytes_of(R["sample_count"]), seed)
    hist = [np.arange(R["sample_count"], dtype=np.int16) * (c + 1) for c in range(nch)]
    return ref.hps_image(44100, adpcm, coefs(nch, seed), [c * 3 for c in range(nch)], [[adpcm[c][0], 5, -6] for c in range(nch)],
                         hist, looping, ls, le, n)


def hps_parse(data):
    buf = np.frombuffer(data, dtype=np.uint8)
    info = _lib.HpsInfoC()
    rc = _lib.lib().vga_hps_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), None, 0)
    if rc:
        return rc, info, []
    blocks = (_lib.HpsBlockInfoC * info.block_count)()
    assert _lib.lib().vga_hps_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), blocks, info.block_count) == OK
    return rc, info, list(blocks)


@pytest.mark.parametrize("nch,n,looping,ls,le", [(1, 1, False, 0, 0), (2, 48000, False, 0, 0), (2, 300000, True, 1234, 290000),
                                                 (5, 100000, True, 22960, 100000), (8, 60000, True, 0, 60000)])
def test_hps_parse_matches_restatement(nch, n, looping, ls, le):
    data = hps_file(nch, n, looping, ls, le)
    rc, I, blocks = hps_parse(data)
    assert rc == OK
    R = ref.hps_parse(data)
    assert (I.sample_rate, I.channel_count, I.sample_count, I.looping, I.loop_start) == (
        R["sample_rate"], nch, R["sample_count"], int(R["looping"]), R["loop_start"])
    assert I.block_count == len(R["blocks"]) and I.adpcm_bytes == len(R["audio"][0])
    for c in range(nch):
        assert list(I.coefs[c]) == R["channels"][c]["coefs"] and I.gain[c] == R["channels"][c]["gain"]
        assert list(I.start_context[c]) == R["channels"][c]["start"]
        assert list(I.loop_context[c]) == list(R["loop_context"][c])
    for b, rb in zip(blocks, R["blocks"]):
        assert (b.offset, b.next_offset, b.size, b.final_nibble, b.audio_offset) == (
            rb["offset"], rb["next"], rb["size"], rb["final"], rb["audio_start"])


def test_hps_parse_errors():
    good = hps_file(2, 100000)
    assert hps_parse(b"x" * len(good))[0] == DATA                           # magic
    bad = bytearray(good)
    struct.pack_into(">i", bad, 16 + 0x38 + 8, struct.unpack_from(">i", bad, 16 + 8)[0] - 32)
    assert hps_parse(bytes(bad))[0] == DATA                                  # differing sample counts
    bad = bytearray(good)
    struct.pack_into(">i", bad, 12, 0)
    assert hps_parse(bytes(bad))[0] == DATA                                  # no channels
    bad = bytearray(good)
    struct.pack_into(">i", bad, 12, 256)
    assert hps_parse(bytes(bad))[0] == OP
    # a chain that points backwards mid-file: the walk stops, the audio falls short of the sample count
    _, _, blocks = hps_parse(good)
    assert len(blocks) >= 2
    bad = bytearray(good)
    struct.pack_into(">i", bad, blocks[0].offset + 8, 0x40)
    assert hps_parse(bytes(bad))[0] == DATA


def test_hps_parse_every_truncation_fails_cleanly():
    data = hps_file(2, 3000, True, 0, 3000)
    _, _, blocks = hps_parse(data)
    last = blocks[-1]
    end = last.audio_offset + last.size // 2 + last.audio_bytes     # the last byte HpsReader reads; padding follows
    assert end < len(data)
    for cut in range(len(data)):
        rc = hps_parse(data[:cut])[0]
        assert rc == (DATA if cut < end else OK), cut


def idsp_file(nch, n, looping=False, ls=0, le=0, block_size=0x10, trim=True, seed=2):
    R = ref.idsp_layout(nch, n, looping, ls, le, block_size, trim)
    adpcm = rows(nch, ref.bytes_of(R["channel_sample_count"]), seed)
    return ref.idsp_image(32000, adpcm, coefs(nch, seed), [7] * nch, [[adpcm[c][0], 1, 2] for c in range(nch)],
                          [[3, 4, 5]] * nch, looping, ls, le, n, block_size, trim)


def idsp_parse(data):
    buf = np.frombuffer(data, dtype=np.uint8)
    info = _lib.IdspInfoC()
    return _lib.lib().vga_idsp_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info)), info


@pytest.mark.parametrize("nch,block_size,looping,trim", [(1, 0, False, True), (2, 0x10, True, True), (3, 0x38, True, False),
                                                         (8, 0x800, False, False)])
def test_idsp_parse_matches_restatement(nch, block_size, looping, trim):
    data = idsp_file(nch, 20000, looping, 1000, 19000, block_size, trim)
    rc, I = idsp_parse(data)
    assert rc == OK
    R = ref.idsp_parse(data)
    for k in ("channel_count", "sample_rate", "sample_count", "loop_start", "loop_end", "interleave_size", "header_size",
              "channel_info_size", "audio_data_offset", "audio_data_length"):
        assert getattr(I, k) == R[k], k
    assert I.looping == int(R["looping"]) and I.adpcm_bytes == len(R["audio"][0])
    for c in range(nch):
        ch = R["channels"][c]
        assert list(I.coefs[c]) == ch["coefs"] and I.gain[c] == ch["gain"]
        assert list(I.start_context[c]) == ch["start"] and list(I.loop_context[c]) == ch["loop"]
        assert I.channel_sample_count[c] == ch["sample_count"] and I.end_address[c] == ch["end_address"]


def test_idsp_parse_errors():
    good = idsp_file(2, 5000)
    assert idsp_parse(b"IDSQ" + good[4:])[0] == DATA
    for cut in range(0, len(good), 7):
        assert idsp_parse(good[:cut])[0] == DATA, cut
    bad = bytearray(good)
    struct.pack_into(">i", bad, 8, 0)
    assert idsp_parse(bytes(bad))[0] == DATA
    struct.pack_into(">i", bad, 8, 256)
    assert idsp_parse(bytes(bad))[0] == OP
    bad = bytearray(good)
    struct.pack_into(">i", bad, 0x1c, 0)                                     # interleave 0 -> AudioDataLength
    assert idsp_parse(bytes(bad))[0] == OK
    struct.pack_into(">i", bad, 0x2c, 0)                                     # ... which is 0 as well
    assert idsp_parse(bytes(bad))[0] == DATA
    # the BlockSize setter rejects what the header may hold (ReadWithConfig -> GetConfiguration)
    from vgaudio_amd.idsp import IdspConfiguration
    for v in (-16, 12):
        with pytest.raises(_lib.ArgumentOutOfRangeError):
            IdspConfiguration(BlockSize=v)


def genh_parse(data):
    buf = np.frombuffer(data, dtype=np.uint8)
    info = _lib.GenhInfoC()
    return _lib.lib().vga_genh_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info)), info


@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("coef_type", [0, 1, 2, 3])
def test_genh_parse_matches_restatement(nch, coef_type):
    co = coefs(nch, 5)
    data = ref.genh_image(22050, rows(nch, ref.bytes_of(3000), 5), co, 0x8000 if nch == 1 else 0x20, 14, 3000, coef_type)
    rc, I = genh_parse(data)
    assert rc == OK
    R = ref.genh_parse(data)
    assert (I.channel_count, I.interleave, I.sample_rate, I.loop_start, I.loop_end, I.sample_count, I.looping) == (
        nch, R["interleave"], 22050, 14, 3000, 3000, 1)
    assert [list(I.coefs[c]) for c in range(nch)] == R["coefs"] == co
    assert I.adpcm_bytes == ref.bytes_of(3000)


def test_genh_parse_errors():
    co = coefs(2, 6)
    good = ref.genh_image(22050, rows(2, ref.bytes_of(3000), 6), co, 0x20)
    assert genh_parse(good)[0] == OK
    assert genh_parse(b"GENX" + good[4:])[0] == DATA
    for nch in (0, 3):
        bad = bytearray(good)
        struct.pack_into("<i", bad, 4, nch)
        assert genh_parse(bytes(bad))[0] == DATA
    assert genh_parse(ref.genh_image(22050, rows(1, 100, 1), co[:1], 0x20, header_size=0x300, audio_offset=0x200))[0] == DATA
    bad = bytearray(good)
    struct.pack_into("<i", bad, 8, 0)                                        # interleave 0
    assert genh_parse(bytes(bad))[0] == DATA
    for cut in range(0, len(good), 5):
        assert genh_parse(good[:cut])[0] == DATA, cut
