"""WAVE reader/writer for 16-bit and 8-bit PCM -- host-side mirror of
VGAudio/Containers/Wave/WaveReader.cs and WaveWriter.cs.  The RIFF header is parsed on the host
(vga_wave_parse); the interleaved <-> planar transposes run on the GPU.  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, i16p, u8p
from .gcadpcm import Pcm16Format, _ptr_array
from .pcm8 import Pcm8Format

VGA_SAMPLES_S16, VGA_SAMPLES_8BIT = 0, 1          # include/vgaudio_hip_pcm.h


class WaveCodec:                                 # Containers/Wave/WaveCodec.cs
    Pcm16Bit = 0
    Pcm8Bit = 1


class WaveReader:
    """AudioReader<WaveReader, WaveStructure, WaveConfiguration>: ReadFormat(file bytes) -> Pcm16Format."""

    @staticmethod
    def ReadMetadata(file):
        data = np.frombuffer(bytes(file), dtype=np.uint8)
        info = _lib.WaveInfoC()
        check(_lib.lib().vga_wave_parse(data.ctypes.data_as(u8p), len(data), C.byref(info)))
        return info

    @staticmethod
    def ReadFormat(file):
        data = np.frombuffer(bytes(file), dtype=np.uint8)
        info = _lib.WaveInfoC()
        check(_lib.lib().vga_wave_parse(data.ctypes.data_as(u8p), len(data), C.byref(info)))
        chans = [np.zeros(info.sample_count, dtype=np.int16) for _ in range(info.channel_count)]
        check(_lib.lib().vga_wave_read_pcm16(data.ctypes.data_as(u8p), len(data), C.byref(info), _ptr_array(i16p, chans)))
        return Pcm16Format(chans, info.sample_rate).WithLoop(bool(info.looping), info.loop_start, info.loop_end)

    @staticmethod
    def ReadPcm8Format(file):
        """ReadFormat for an 8-bit file: the Pcm8Format (unsigned bytes) of WaveReader.cs:61-63"""
        data = np.frombuffer(bytes(file), dtype=np.uint8)
        info = _lib.WaveInfoC()
        check(_lib.lib().vga_wave_parse(data.ctypes.data_as(u8p), len(data), C.byref(info)))
        chans = [np.zeros(info.sample_count, dtype=np.uint8) for _ in range(info.channel_count)]
        ptrs = (C.c_void_p * max(len(chans), 1))(*[c.ctypes.data for c in chans])
        check(_lib.lib().vga_wave_read_pcm8(data.ctypes.data_as(u8p), len(data), C.byref(info), ptrs, VGA_SAMPLES_8BIT))
        return Pcm8Format(chans, info.sample_rate).WithLoop(bool(info.looping), info.loop_start, info.loop_end)


class WaveWriter:
    """AudioWriter<WaveWriter, WaveConfiguration>: GetFile(Pcm16Format), or with codec = WaveCodec.Pcm8Bit an 8-bit
    file from a Pcm8Format (bytes as they are) or a Pcm16Format (Pcm8Codec.Encode on the device)."""

    @staticmethod
    def GetFile(audio, codec=WaveCodec.Pcm16Bit):
        if codec == WaveCodec.Pcm8Bit:
            return WaveWriter._get_pcm8_file(audio)
        if not isinstance(audio, Pcm16Format):
            raise _lib.ArgumentError("WaveWriter takes a Pcm16Format (decode with ToPcm16 first)")
        p = _lib.WaveParamsC(audio.SampleRate, audio.SampleCount, int(audio.Looping), audio.LoopStart, audio.LoopEnd)
        size = _lib.lib().vga_wave_file_size(C.byref(p), audio.ChannelCount)
        if size < 0:
            check(int(size))
        out = np.zeros(size, dtype=np.uint8)
        check(_lib.lib().vga_wave_write_pcm16(_ptr_array(i16p, audio.Channels), audio.ChannelCount, C.byref(p),
                                              out.ctypes.data_as(u8p)))
        return out.tobytes()

    @staticmethod
    def _get_pcm8_file(audio):
        if getattr(audio, "Signed", False):
            audio = audio.ToPcm16()                      # GetFormat<Pcm8Format> from a signed format goes through PCM16
        if isinstance(audio, Pcm8Format):
            rows, kind = [np.ascontiguousarray(c, dtype=np.uint8) for c in audio.Channels], VGA_SAMPLES_8BIT
        elif isinstance(audio, Pcm16Format):
            rows, kind = [np.ascontiguousarray(c, dtype=np.int16) for c in audio.Channels], VGA_SAMPLES_S16
        else:
            raise _lib.ArgumentError("an 8-bit WaveWriter takes a Pcm8Format or a Pcm16Format")
        p = _lib.WaveParamsC(audio.SampleRate, audio.SampleCount, int(audio.Looping), audio.LoopStart, audio.LoopEnd)
        size = _lib.lib().vga_wave_pcm8_file_size(C.byref(p), audio.ChannelCount)
        if size < 0:
            check(int(size))
        out = np.zeros(size, dtype=np.uint8)
        ptrs = (C.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])
        check(_lib.lib().vga_wave_write_pcm8(ptrs, kind, audio.ChannelCount, C.byref(p), out.ctypes.data_as(u8p)))
        return out.tobytes()
