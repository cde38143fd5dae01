"""GENH for GC-ADPCM -- the host-side mirror of VGAudio/Containers/Genh/GenhReader.cs (the reference has no GENH
writer).  The header is parsed on the host (vga_genh_parse); the audio is taken apart on the GPU (vga_genh_read)."""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import check, u8p
from .gcadpcm import GcAdpcmChannel, GcAdpcmFormat, _ptr_array


class GenhCoefType(enum.IntFlag):                # GenhStructure.cs
    Split = 1
    LittleEndian = 2


class GenhConfiguration:
    """GenhConfiguration.cs: no options of its own."""


def parse(data):
    """vga_genh_parse: the header and the coefficients (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.GenhInfoC()
    check(_lib.lib().vga_genh_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


class GenhReader:
    """AudioReader<GenhReader, GenhStructure, GenhConfiguration>: ReadFormat(bytes) -> GcAdpcmFormat."""

    def ReadMetadata(self, data):
        return parse(data)

    def ReadFormat(self, data):
        return self.ReadWithConfig(data)[0]

    def ReadWithConfig(self, data):
        data = bytes(data)
        info = parse(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        adpcm = [np.zeros(info.adpcm_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
        check(_lib.lib().vga_genh_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), _ptr_array(u8p, adpcm)))
        # ToAudioStream (:31-48): channels built with the loop and no stored context, so the build derives it
        chans = [GcAdpcmChannel(adpcm[c], np.array(info.coefs[c][:], dtype=np.int16), info.sample_count)
                 for c in range(info.channel_count)]
        return GcAdpcmFormat(chans, info.sample_rate, bool(info.looping), info.loop_start, info.loop_end), GenhConfiguration()
