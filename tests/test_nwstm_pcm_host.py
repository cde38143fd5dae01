"""PCM8 / PCM16 NintendoWare streams, host side (no GPU): vga_nwstm_pcm_layout_for against the restatement in
nwstm_pcm_ref.py over a grid, vga_nwstm_pcm_parse on restatement-built images, and the refusals."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nwstm_pcm_ref as ref
from vgaudio_amd import _lib
from vgaudio_amd.nwstm import BxstmConfiguration, NwCodec

RSTM, CSTM, FSTM = 0, 1, 2
VERSIONS = {RSTM: [0], CSTM: [0, 0x02000000, 0x02010000, 0x02020000, 0x02030000],
            FSTM: [0, 0x00020000, 0x00030000, 0x00040000, 0x00050000]}


def layout(target, codec, nch, n, **kw):
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = target, 48000, n, -1
    for k, v in kw.items():
        setattr(p, k, v)
    L = _lib.NwLayoutC()
    return _lib.lib().vga_nwstm_pcm_layout_for(C.byref(p), codec, nch, C.byref(L)), L


def parse(data):
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.NwInfoC()
    return _lib.lib().vga_nwstm_pcm_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info)), info


@pytest.mark.parametrize("target,codec", list(itertools.product([RSTM, CSTM, FSTM], [ref.PCM8, ref.PCM16])))
def test_layout_matches_restatement(target, codec):
    for nch, spi, looping, version, endian in itertools.product(
            [1, 2, 8, 255], [0, 1, 3, 4097, 8192, 0x3800], [False, True], VERSIONS[target], [-1, 0, 1]):
        n = 48001
        rc, L = layout(target, codec, nch, n, samples_per_interleave=spi, looping=int(looping),
                       loop_start=777 if looping else 0, loop_end=30001 if looping else 0, version=version,
                       endianness=endian)
        R = ref.layout(target, codec, nch, n, looping, 777, 30001, spi or None, None, version=version or None)
        if R["include_unaligned_loop"]:
            assert rc == -4                         # VGA_ERR_INVALID_OP: the reference fails on a null Adpcm
            continue
        assert rc == 0
        for k, v in R.items():
            assert getattr(L, k) == v, (nch, spi, looping, version, k)
        assert L.loop_start == (777 if looping else 0) and L.alignment_needed == 0
        assert L.channel_sample_count == n and L.channel_adpcm_bytes == n * ref.bps(codec)
        if target != RSTM:
            assert L.endianness == (endian if endian >= 0 else int(target == FSTM))


def test_codec_defaults_and_checks():
    assert layout(RSTM, ref.PCM16, 2, 100)[1].samples_per_interleave == 4096
    assert layout(RSTM, ref.PCM8, 2, 100)[1].samples_per_interleave == 8192
    assert layout(CSTM, ref.PCM16, 2, 100)[1].samples_per_seek_table_entry == 4096
    assert layout(FSTM, ref.PCM8, 2, 100)[1].samples_per_seek_table_entry == 8192
    assert layout(RSTM, ref.PCM8, 2, 100, samples_per_interleave=13)[0] == 0      # no divisible-by-14 rule
    assert layout(RSTM, 2, 2, 100)[0] == -1                                        # GC-ADPCM: the other call
    assert layout(RSTM, ref.PCM8, 2, 100, samples_per_seek_table_entry=1)[0] == -2
    assert layout(RSTM, ref.PCM8, 2, 100, looping=1, loop_start=50, loop_end=101)[0] == -2
    assert layout(CSTM, ref.PCM16, 2, 100, version=0x02030000)[0] == -4
    assert layout(FSTM, ref.PCM16, 2, 100, version=0x00040000)[0] == -4
    # the Python configuration follows the codec
    assert BxstmConfiguration(Codec=NwCodec.Pcm16Bit).SamplesPerInterleave == 4096
    assert BxstmConfiguration(Codec=NwCodec.Pcm8Bit).LoopPointAlignment == 8192
    assert BxstmConfiguration().SamplesPerInterleave == 14336
    BxstmConfiguration(Codec=NwCodec.Pcm8Bit, SamplesPerInterleave=1001)
    with pytest.raises(_lib.ArgumentOutOfRangeError):
        BxstmConfiguration(SamplesPerInterleave=1001)


def _rows(codec, nch, n, seed=1):
    rng = np.random.default_rng(seed)
    if codec == ref.PCM16:
        return [rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(nch)]
    return [rng.integers(0, 256, n).astype(np.uint8) for _ in range(nch)]


@pytest.mark.parametrize("target,codec,nch,looping", list(itertools.product([RSTM, CSTM, FSTM], [0, 1], [1, 2, 8], [0, 1])))
def test_parse_restatement_images(target, codec, nch, looping):
    rows = _rows(codec, nch, 5001)
    img = ref.build_image(target, codec, 44100, rows, looping=bool(looping), loop_start=300, loop_end=4000, spi=777)
    rc, I = parse(img)
    assert rc == 0
    expect = ref.parse_image(img)
    assert I.codec == codec and I.channel_count == nch and I.sample_rate == 44100
    assert I.looping == looping and I.loop_start == (300 if looping else 0)
    assert I.sample_count == (4000 if looping else 5001) == expect["sample_count"]
    assert I.audio_data_offset == expect["audio_offset"] and I.interleave_size == 777 * ref.bps(codec)
    assert I.adpcm_bytes == I.sample_count * ref.bps(codec)
    assert I.seek_block_offset == 0 and I.seek_entries == 0
    tr = ref.parse_image(img)["tracks"]
    assert I.track_count == len(tr)
    for t, e in zip(I.tracks[:I.track_count], tr):
        assert (t.channel_count, t.left, t.right, t.volume, t.panning) == \
            (e["channel_count"], e["left"], e["right"], e["volume"], e["panning"])


def test_refusals():
    rows = _rows(ref.PCM16, 2, 3000)
    img = ref.build_image(CSTM, ref.PCM16, 48000, rows)
    # a GC-ADPCM stream goes to vga_nwstm_parse; an IMA-ADPCM byte is refused too
    for target in (RSTM, CSTM):
        im = bytearray(ref.build_image(target, ref.PCM8, 48000, _rows(ref.PCM8, 1, 100)))
        off = 0x40 + 8 + 24                      # the stream info's codec byte (HEAD / INFO + reference table)
        assert im[off] == 0
        for codec in (2, 3):
            im[off] = codec
            rc, _ = parse(bytes(im))
            assert rc == -4
    # the GC-only parser keeps refusing PCM
    buf = np.frombuffer(img, dtype=np.uint8)
    info = _lib.NwInfoC()
    assert _lib.lib().vga_nwstm_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info)) == -4
    # truncations are refused and never read past the end
    for cut in list(range(0, 0x80, 3)) + [len(img) - 1, len(img) - 33]:
        rc, _ = parse(img[:cut])
        assert rc != 0
    bad = bytearray(img)
    bad[0:4] = b"XSTM"
    assert parse(bytes(bad))[0] == -3
    bad = bytearray(img)
    bad[4:6] = b"\x00\x00"
    assert parse(bytes(bad))[0] == -3
