"""8-bit WAVE and Pcm8Codec on the GPU: WaveTests.WavePcm8BuildAndParseEqual / WavePcm8LoopedBuildAndParseEqual
(VGAudio.Tests/Containers/WaveTests.cs) against a struct restatement of WaveWriter.cs with WaveCodec.Pcm8Bit, the
codec against numpy over every input value, and an 8-bit WAVE -> HCA chain."""
import ctypes as C
import struct

import numpy as np
import pytest

from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import Pcm16Format
from vgaudio_amd.hca import HcaWriter
from vgaudio_amd.pcm8 import Pcm8Codec, Pcm8Format, Pcm8SignedFormat
from vgaudio_amd.wave import WaveCodec, WaveReader, WaveWriter

pytestmark = pytest.mark.gpu

MASKS = {4: 0x0033, 5: 0x0133, 6: 0x0633, 7: 0x01f3, 8: 0x06f3}
SUBTYPE_PCM = bytes([0x01, 0, 0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])


def encode(s16):                                  # Pcm8Codec.Encode
    return ((np.asarray(s16, dtype=np.int32) + 0x8000) >> 8).astype(np.uint8)


def decode(b):                                    # Pcm8Codec.Decode
    return ((np.asarray(b, dtype=np.int32) - 0x80) << 8).astype(np.int16)


def wave8(rows, rate, looping=False, loop_start=0, loop_end=0):
    """WaveWriter.cs (:56-129) with BitDepth 8, written out with struct"""
    nch, n = len(rows), len(rows[0])
    fmt_size = 40 if nch > 2 else 16
    data = nch * n
    riff = 4 + 8 + fmt_size + 8 + data + (8 + 0x3c if looping else 0)
    out = b"RIFF" + struct.pack("<i", riff) + b"WAVE"
    out += b"fmt " + struct.pack("<iHHiiHH", fmt_size, 0xFFFE if nch > 2 else 1, nch, rate, rate * nch, nch, 8)
    if nch > 2:
        out += struct.pack("<HHi", 22, 8, MASKS.get(nch, (1 << nch) - 1)) + SUBTYPE_PCM
    if looping:
        out += b"smpl" + struct.pack("<i", 0x3c) + struct.pack("<7i", *[0] * 7) + struct.pack("<i", 1)
        out += struct.pack("<3i", 0, 0, 0) + struct.pack("<4i", loop_start, loop_end, 0, 0)
    out += b"data" + struct.pack("<i", data) + np.stack(rows).T.astype(np.uint8).tobytes()
    return out


def _rows(nch, n, seed):
    return [np.random.default_rng(seed + c).integers(0, 256, n).astype(np.uint8) for c in range(nch)]


@pytest.mark.parametrize("nch", [1, 2, 8])
@pytest.mark.parametrize("looped", [False, True])
@pytest.mark.parametrize("n", [10000, 10001])
def test_wave_pcm8_build_and_parse_equal(nch, looped, n):
    rows = _rows(nch, n, nch)
    fmt = Pcm8Format(rows, 22050)
    if looped:
        fmt.WithLoop(True, 123, 9001)
    img = WaveWriter.GetFile(fmt, WaveCodec.Pcm8Bit)
    assert img == wave8(rows, 22050, looped, 123 if looped else 0, 9001 if looped else 0)
    back = WaveReader.ReadPcm8Format(img)
    assert back.ChannelCount == nch and back.SampleRate == 22050
    assert (back.Looping, back.LoopStart, back.LoopEnd) == ((True, 123, 9001) if looped else (False, 0, 0))
    assert all(np.array_equal(a, b) for a, b in zip(back.Channels, rows))
    # from int16 through Encode on the device; read back to int16 through Decode
    pcm = Pcm16Format([decode(r) + 77 for r in rows], 22050)
    assert WaveWriter.GetFile(pcm, WaveCodec.Pcm8Bit) == wave8(rows, 22050)
    assert all(np.array_equal(a, decode(r)) for a, r in zip(back.ToPcm16().Channels, rows))
    with pytest.raises(_lib.ArgumentError):
        WaveReader.ReadFormat(img)                    # the 16-bit reader keeps refusing 8-bit files


def test_pcm8_codec_every_value():
    s = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(Pcm8Codec.Encode(s), encode(s))
    assert np.array_equal(Pcm8Codec.EncodeSigned(s), (s >> 8).astype(np.int8).view(np.uint8))
    assert np.array_equal(Pcm8Codec.Decode(b), decode(b))
    assert np.array_equal(Pcm8Codec.DecodeSigned(b), (b.view(np.int8).astype(np.int16) << 8).astype(np.int16))
    fmt = Pcm8SignedFormat.EncodeFromPcm16(Pcm16Format([s, s[::-1].copy()], 8000))
    assert np.array_equal(fmt.Channels[1], (s[::-1] >> 8).astype(np.int8).view(np.uint8))


def test_odd_frames_device_deinterleave():
    """odd frame sizes and a misaligned data chunk through vga_wave_deinterleave_pcm8_device, to int16 and to bytes"""
    import torch
    nch, n = 3, 4099
    rows = _rows(nch, n, 40)
    data = np.stack(rows).T.reshape(-1)
    d = torch.zeros(len(data) + 1, dtype=torch.uint8, device="cuda")
    d[1:] = torch.from_numpy(data).cuda()
    s = torch.cuda.current_stream().cuda_stream
    out16 = torch.zeros((nch, n + 5), dtype=torch.int16, device="cuda")
    out8 = torch.zeros((nch, n + 5), dtype=torch.uint8, device="cuda")
    L = _lib.lib()
    assert L.vga_wave_deinterleave_pcm8_device(C.c_void_p(d.data_ptr() + 1), n, nch, C.c_void_p(out16.data_ptr()), 0, n + 5,
                                               C.c_void_p(s)) == 0
    assert L.vga_wave_deinterleave_pcm8_device(C.c_void_p(d.data_ptr() + 1), n, nch, C.c_void_p(out8.data_ptr()), 1, n + 5,
                                               C.c_void_p(s)) == 0
    assert np.array_equal(out16.cpu().numpy()[:, :n], np.stack([decode(r) for r in rows]))
    assert np.array_equal(out8.cpu().numpy()[:, :n], np.stack(rows))


def test_data_not_divisible_by_channels_is_refused():
    img = bytearray(wave8(_rows(2, 100, 3), 8000))
    img = bytes(img[:-1])                            # 199 data bytes present for 2 channels
    with pytest.raises(_lib.InvalidDataError):
        WaveReader.ReadPcm8Format(img)


def test_wave_pcm8_to_hca_on_device():
    """8-bit WAVE -> vga_wave_deinterleave_pcm8_device (S16) -> HCA equals the HCA of Decode of the bytes"""
    rows = _rows(2, 48000, 11)
    img = wave8(rows, 48000)
    via_device = WaveReader.ReadPcm8Format(img).ToPcm16()
    direct = Pcm16Format([decode(r) for r in rows], 48000)
    assert HcaWriter().GetFile(via_device) == HcaWriter().GetFile(direct)
