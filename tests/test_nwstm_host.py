"""NintendoWare stream size math and parsing (host only, no GPU): vga_nwstm_layout_for against known answers and the
independent restatement in nwstm_ref.py, vga_nwstm_parse on restatement-built images and on broken ones."""
import ctypes as C
import itertools
import random
import struct

import numpy as np
import pytest

import nwstm_ref as ref
from vgaudio_amd import _lib

RSTM, CSTM, FSTM = 0, 1, 2
VERSIONS = {CSTM: [0x02000000, 0x02010000, 0x02020000, 0x02030000], FSTM: [0x00020000, 0x00030000, 0x00040000, 0x00050000]}


def layout(target, nch, n, **kw):
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = target, 48000, n, -1
    for k, v in kw.items():
        setattr(p, k, v)
    L = _lib.NwLayoutC()
    rc = _lib.lib().vga_nwstm_layout_for(C.byref(p), nch, C.byref(L))
    return rc, L


# hand-derived from the cited formulas: 48 000 samples, no loop, default settings
KAT = [
    # target, nch, version, head/info block, seek block, data block offset, file size
    (RSTM, 1, 0, 192, 32, 288, 27776),
    (RSTM, 2, 0, 256, 64, 384, 55328),
    (CSTM, 2, 0x02010000, 288, 64, 416, 55360),
    (FSTM, 2, 0x00030000, 256, 64, 384, 55328),
    (FSTM, 2, 0x00040000, 256, 64, 384, 55328),
]


@pytest.mark.parametrize("target,nch,version,head,seek,data_off,file_size", KAT)
def test_layout_known_answers(target, nch, version, head, seek, data_off, file_size):
    rc, L = layout(target, nch, 48000, version=version)
    assert rc == 0
    assert (L.interleave_count, L.last_block_samples, L.last_block_size_without_padding, L.last_block_size) == (4, 4992, 2853, 2880)
    assert L.audio_data_size == 27456
    assert (L.head_block_size, L.seek_block_size, L.data_block_offset, L.file_size) == (head, seek, data_off, file_size)
    assert L.audio_data_offset == data_off + 0x20


def test_layout_version_flags_and_words():
    rc, L = layout(CSTM, 2, 48000)
    assert rc == 0 and L.version == 0x02010000 and (L.include_track_info, L.include_region_info, L.include_unaligned_loop) == (1, 1, 0)
    assert L.version_word == 0x201 << 16
    rc, L = layout(FSTM, 2, 48000)
    assert rc == 0 and L.version == 0x00030000 and (L.include_track_info, L.include_region_info, L.include_unaligned_loop) == (0, 1, 0)
    assert L.version_word == 3 << 16 and L.endianness == 1
    assert layout(FSTM, 2, 48000, version=0x00040000)[1].version_word == 4 << 16
    assert layout(CSTM, 2, 48000, version=0x02000000)[1].version_word == 0x200 << 16
    assert layout(CSTM, 2, 48000, version=0x02020000)[1].version_word == 0x202 << 16
    assert layout(CSTM, 2, 48000)[1].endianness == 0
    assert layout(CSTM, 2, 48000, endianness=1)[1].endianness == 1


def test_layout_validation():
    assert layout(RSTM, 2, 1000, samples_per_interleave=15)[0] == _lib.VGA_ERR_OUT_OF_RANGE
    assert layout(RSTM, 2, 1000, samples_per_interleave=-14)[0] == _lib.VGA_ERR_OUT_OF_RANGE
    assert layout(RSTM, 2, 1000, samples_per_seek_table_entry=1)[0] == _lib.VGA_ERR_OUT_OF_RANGE
    assert layout(FSTM, 2, 1000, keep_seek_table=1)[0] == _lib.VGA_ERR_ARGUMENT
    assert layout(FSTM, 2, 1000, keep_loop_context=1)[0] == _lib.VGA_ERR_ARGUMENT
    assert layout(FSTM, 2, 1000, looping=1, loop_start=10, loop_end=2000)[0] == _lib.VGA_ERR_OUT_OF_RANGE
    assert layout(FSTM, 2, 1000, version=0x02010000)[0] == _lib.VGA_ERR_OUT_OF_RANGE
    assert layout(3, 2, 1000)[0] == _lib.VGA_ERR_ARGUMENT
    assert layout(RSTM, 0, 1000)[0] == _lib.VGA_ERR_ARGUMENT


def test_layout_loop_alignment():
    """BrstmLoopAlignmentIsSet: loop 1288..16288 with alignment 700 -> 1400 / 16400"""
    for target in (RSTM, CSTM, FSTM):
        rc, L = layout(target, 2, 20000, looping=1, loop_start=1288, loop_end=16288, loop_point_alignment=700)
        assert rc == 0 and L.alignment_needed == 1
        assert (L.loop_start, L.loop_end, L.sample_count, L.channel_sample_count) == (1400, 16400, 16400, 16400)
        assert L.channel.loop_alignment_multiple == 700 and (L.channel.loop_start, L.channel.loop_end) == (1288, 16288)


LENGTHS = [1, 13, 14 * 64 * 3, 14336 * 2, 48000, 100003]


@pytest.mark.parametrize("target", [RSTM, CSTM, FSTM])
def test_layout_grid_matches_restatement(target):
    versions = VERSIONS.get(target, [0])
    cases = itertools.product([14, 14 * 64, 14336], [2, 100, 14336], [0, 1], [0, 1], versions, LENGTHS, [1, 2, 3, 8])
    for spi, spe, tshort, sshort, version, n, nch in cases:
        if target != RSTM and (tshort or sshort):
            continue
        rc, L = layout(target, nch, n, samples_per_interleave=spi, samples_per_seek_table_entry=spe, track_type=tshort,
                       seek_table_type=sshort, version=version)
        assert rc == 0
        R = ref.layout(target, nch, n, spi=spi, spe=spe, track_short=bool(tshort), seek_short=bool(sshort),
                       version=version or None)
        got = dict(sample_count=L.sample_count, audio_data_size=L.audio_data_size, interleave_size=L.interleave_size,
                   interleave_count=L.interleave_count, last_block_samples=L.last_block_samples,
                   last_block_size_without_padding=L.last_block_size_without_padding, last_block_size=L.last_block_size,
                   seek_table_entry_count=L.seek_table_entry_count, h1=L.head1_size, h2=L.head2_size, h3=L.head3_size,
                   head_block_size=L.head_block_size, seek_block_size=L.seek_block_size,
                   data_block_offset=L.data_block_offset, data_block_size=L.data_block_size,
                   audio_data_offset=L.audio_data_offset, file_size=L.file_size)
        assert got == R, (spi, spe, tshort, sshort, hex(version), n, nch)


def random_image(rng, target, nch, n, looping=False, loop_start=0, loop_end=0, version=None, big=None, spi=ref.DEFAULT,
                 spe=ref.DEFAULT, track_short=False, seek_short=False, tracks=None):
    """a restatement-built image over random payload (the parser does not look at what the audio means)"""
    sc = loop_end if looping else n
    ch_bytes = ref.bytes_of(n)
    adpcm = [bytes(rng.getrandbits(8) for _ in range(ch_bytes)) for _ in range(nch)]
    coefs = [[rng.randint(-32768, 32767) for _ in range(16)] for _ in range(nch)]
    gain = [rng.randint(-32768, 32767) for _ in range(nch)]
    start = [[rng.randint(0, 255), rng.randint(-32768, 32767), rng.randint(-32768, 32767)] for _ in range(nch)]
    loopc = [[rng.randint(0, 255), rng.randint(-32768, 32767), rng.randint(-32768, 32767)] for _ in range(nch)]
    seek = [[rng.randint(-32768, 32767) for _ in range(2 * -(-n // spe))] for _ in range(nch)]
    img = ref.build_image(target, 32000, nch, adpcm, coefs, gain, start, loopc, seek, looping, loop_start, loop_end, n,
                          spi=spi, spe=spe, track_short=track_short, seek_short=seek_short, version=version, big=big,
                          tracks=tracks)
    return img, dict(adpcm=adpcm, coefs=coefs, gain=gain, start=start, loop=loopc if looping else start, sc=sc)


def parse(img):
    info = _lib.NwInfoC()
    buf = np.frombuffer(img, dtype=np.uint8)
    rc = _lib.lib().vga_nwstm_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info))
    return rc, info


PARSE_CASES = [
    dict(target=RSTM, nch=1, n=48000),
    dict(target=RSTM, nch=2, n=30001, looping=True, loop_start=1400, loop_end=20000),
    dict(target=RSTM, nch=3, n=5000, track_short=True, seek_short=True, spi=14 * 64, spe=100),
    dict(target=CSTM, nch=2, n=48000),
    dict(target=CSTM, nch=5, n=777, version=0x02000000),
    dict(target=CSTM, nch=2, n=20000, version=0x02030000, looping=True, loop_start=14336, loop_end=20000),
    dict(target=CSTM, nch=2, n=3000, big=True, version=0x02020000),
    dict(target=FSTM, nch=2, n=48000),
    dict(target=FSTM, nch=1, n=14, version=0x00020000),
    dict(target=FSTM, nch=4, n=40000, version=0x00040000, looping=True, loop_start=0, loop_end=39000),
    dict(target=FSTM, nch=2, n=9999, version=0x00050000, big=False),
    dict(target=RSTM, nch=2, n=4000, tracks=[dict(channel_count=2, left=1, right=0, volume=3, panning=9)]),
]


@pytest.mark.parametrize("case", PARSE_CASES, ids=lambda c: "%s-%dch-%d" % ("RCF"[c["target"]], c["nch"], c["n"]))
def test_parse_restatement_images(case):
    rng = random.Random(case["n"] * 31 + case["nch"])
    img, src = random_image(rng, **case)
    R = ref.parse_image(img)
    rc, I = parse(img)
    assert rc == 0, _lib.lib().vga_last_error()
    nch = case["nch"]
    assert (I.target, I.channel_count, I.codec, I.sample_rate) == (case["target"], nch, 2, 32000)
    assert (I.looping, I.loop_start, I.sample_count) == (int(case.get("looping", False)), case.get("loop_start", 0), src["sc"])
    assert (I.interleave_size, I.interleave_count, I.samples_per_interleave) == (R["interleave_size"], R["interleave_count"], R["spi"])
    assert (I.last_block_size_without_padding, I.last_block_samples, I.last_block_size) == (R["lbs_nopad"], R["lb_samples"], R["lbs"])
    assert I.samples_per_seek_table_entry == R["spe"]
    assert (I.audio_data_offset, I.audio_data_length) == (R["audio_offset"], R["audio_length"])
    assert I.endianness == int(R["big"]) and I.file_size == len(img)
    if case["target"] == RSTM:
        assert I.track_type == int(case.get("track_short", False)) and I.seek_table_type == int(case.get("seek_short", False))
    if case["target"] != RSTM:
        # the file carries GetVersion(Type) << 16, not the configured version (BCFstmWriter.cs:147-169)
        rc, L = layout(case["target"], nch, case["n"], version=case.get("version", 0))
        assert I.version == L.version_word
    for c in range(nch):
        assert list(I.coefs[c]) == src["coefs"][c] == R["channels"][c]["coefs"]
        assert list(I.start_context[c]) == [struct.unpack("h", struct.pack("H", v & 0xffff))[0] for v in src["start"][c]]
        assert list(I.loop_context[c]) == [struct.unpack("h", struct.pack("H", v & 0xffff))[0] for v in src["loop"][c]]
        if case["target"] == RSTM:
            assert I.gain[c] == src["gain"][c]
    tracks = [dict(channel_count=t.channel_count, left=t.left, right=t.right, volume=t.volume, panning=t.panning)
              for t in I.tracks[:I.track_count]]
    assert tracks == R["tracks"]
    assert I.seek_entries * 4 * nch <= len(img) - I.seek_table_offset
    # the stored seek table, read the library's way, equals the restatement's
    for c in range(nch):
        e = "<>"[I.seek_big_endian]
        got = [struct.unpack_from(e + "h", img, I.seek_table_offset + (k // 2 * nch + c) * 4 + 2 * (k % 2))[0]
               for k in range(2 * I.seek_entries)]
        assert got == R["seek_raw"][c][:2 * I.seek_entries]


def _err(img):
    return parse(bytes(img))[0]


def test_parse_errors():
    rng = random.Random(5)
    rstm, _ = random_image(rng, RSTM, 2, 3000)
    fstm, _ = random_image(rng, FSTM, 2, 3000)
    cstm, _ = random_image(rng, CSTM, 2, 3000)
    assert parse(rstm)[0] == 0 and parse(fstm)[0] == 0 and parse(cstm)[0] == 0
    for img in (rstm, fstm, cstm):
        assert _err(img[:len(img) - 1]) == _lib.VGA_ERR_INVALID_DATA               # shorter than stated
        assert _err(img[:40]) == _lib.VGA_ERR_INVALID_DATA
        assert _err(b"XXXX" + img[4:]) == _lib.VGA_ERR_INVALID_DATA                  # bad magic
        assert _err(img[:4] + img[5:6] + img[4:5] + img[6:]) == _lib.VGA_ERR_INVALID_DATA or img[:4] != b"RSTM"
    assert _err(rstm[:4] + b"\xff\xfe" + rstm[6:]) == _lib.VGA_ERR_INVALID_DATA     # BRSTM is big-endian only
    assert _err(fstm[:4] + b"\x00\x00" + fstm[6:]) == _lib.VGA_ERR_INVALID_DATA     # no byte order mark
    # a swapped BOM makes every field read the other way round: the block table no longer describes the file
    assert _err(fstm[:4] + fstm[5:6] + fstm[4:5] + fstm[6:]) == _lib.VGA_ERR_INVALID_DATA
    # block sizes that disagree: the INFO / HEAD header's size against the block table
    for img in (rstm, fstm):
        bad = bytearray(img)
        head = 0x40
        bad[head + 7] ^= 0x20
        assert _err(bad) == _lib.VGA_ERR_INVALID_DATA
    # PCM16 codec byte
    for img in (rstm, fstm):
        I = parse(img)[1]
        R = ref.parse_image(img)
        bad = bytearray(img)
        si = 0x40 + 8 + struct.unpack_from(">i" if R["big"] else "<i", img, 0x40 + 8 + 4)[0]
        assert bad[si] == 2
        bad[si] = 1
        assert _err(bad) == _lib.VGA_ERR_INVALID_OP
        assert "PCM16" in _lib.lib().vga_last_error().decode()
        del I
    for magic in (b"CWAV", b"FWAV", b"CSTP", b"FSTP"):
        assert _err(magic + fstm[4:]) == _lib.VGA_ERR_INVALID_OP
        assert magic.decode() in _lib.lib().vga_last_error().decode()


def test_parse_random_truncations_never_read_past_the_end():
    rng = random.Random(11)
    img, _ = random_image(rng, CSTM, 3, 2000)
    for cut in sorted(rng.sample(range(len(img)), 40)):
        rc = _err(img[:cut])
        assert rc == _lib.VGA_ERR_INVALID_DATA
