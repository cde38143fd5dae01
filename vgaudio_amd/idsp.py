"""IDSP for GC-ADPCM -- the host-side mirror of VGAudio/Containers/Idsp: IdspWriter.cs, IdspReader.cs and
IdspConfiguration.cs.  Size math and parsing run on the host (vga_idsp_layout_for, vga_idsp_parse); the images are
assembled and taken apart on the GPU (vga_idsp_write, vga_idsp_read).  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, u8p
from .gcadpcm import GcAdpcmChannel, GcAdpcmContext, GcAdpcmFormat, _i16, _ptr_array

BytesPerFrame = 8


class IdspConfiguration:
    """IdspConfiguration.cs + Configuration.cs (TrimFile).  RecalculateLoopContext is kept but, as in the reference,
    the writer does not read it."""

    def __init__(self, BlockSize=BytesPerFrame * 2, TrimFile=True, RecalculateLoopContext=True):
        self.BlockSize = BlockSize
        self.TrimFile = TrimFile
        self.RecalculateLoopContext = RecalculateLoopContext

    @property
    def BlockSize(self):
        return self._block_size

    @BlockSize.setter
    def BlockSize(self, value):                  # IdspConfiguration.cs
        if value < 0:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be non-negative")
        if value % BytesPerFrame != 0:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be divisible by 14")
        self._block_size = int(value)


def _ctx(channels, attr):
    return np.array([[getattr(c, attr).PredScale, getattr(c, attr).Hist1, getattr(c, attr).Hist2] for c in channels],
                    dtype=np.int16)


class IdspWriter:
    """AudioWriter<IdspWriter, IdspConfiguration>.GetFile(format, configuration) for a GcAdpcmFormat."""

    def __init__(self, configuration=None):
        self.Configuration = configuration or IdspConfiguration()

    def _params(self, fmt):
        c = self.Configuration
        return _lib.IdspParamsC(fmt.SampleRate, fmt.UnalignedSampleCount, int(fmt.Looping), fmt.UnalignedLoopStart,
                                fmt.UnalignedLoopEnd, c.BlockSize, int(bool(c.TrimFile)))

    def Layout(self, fmt):
        """The sizes IdspWriter.cs:17-51 derives (no device work)."""
        L = _lib.IdspLayoutC()
        check(_lib.lib().vga_idsp_layout_for(C.byref(self._params(fmt)), fmt.ChannelCount, C.byref(L)))
        return L

    def GetFile(self, audio, configuration=None):
        if configuration is not None:
            self.Configuration = configuration
        if not isinstance(audio, GcAdpcmFormat):
            raise _lib.ArgumentError("IdspWriter takes a GcAdpcmFormat (encode PCM with EncodeFromPcm16 first)")
        p = self._params(audio)
        L = self.Layout(audio)
        # SetupWriter: WithAlignment(ByteCountToSampleCount(BlockSize)) when interleaved (one batched channel build)
        mult = L.channel.loop_alignment_multiple if self.Configuration.BlockSize else audio.AlignmentMultiple
        built = audio._clone(alignmentMultiple=mult)
        nch = built.ChannelCount
        adpcm = [np.ascontiguousarray(c.GetAdpcmAudio(), dtype=np.uint8) for c in built.Channels]
        if any(len(a) != len(adpcm[0]) for a in adpcm):
            raise _lib.ArgumentOutOfRangeError("Inputs must be of equal length")                  # Interleave.cs:49-50
        coefs = np.ascontiguousarray(np.stack([c.Coefs for c in built.Channels]), dtype=np.int16).reshape(nch, 16)
        gain = np.array([c.Gain for c in audio.Channels], dtype=np.int16)
        out = np.zeros(L.file_size, dtype=np.uint8)
        check(_lib.lib().vga_idsp_write(C.byref(p), nch, _ptr_array(u8p, adpcm), len(adpcm[0]), _i16(coefs), _i16(gain),
                                        _i16(_ctx(audio.Channels, "StartContext")), _i16(_ctx(built.Channels, "LoopContext")),
                                        out.ctypes.data_as(u8p)))
        return out.tobytes()


def parse(data):
    """vga_idsp_parse: the header and channel infos (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.IdspInfoC()
    check(_lib.lib().vga_idsp_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


class IdspReader:
    """AudioReader<IdspReader, IdspStructure, IdspConfiguration>: ReadFormat(bytes) -> GcAdpcmFormat,
    ReadWithConfig(bytes) -> (format, IdspConfiguration(BlockSize = InterleaveSize))."""

    def ReadMetadata(self, data):
        return parse(data)

    def ReadFormat(self, data):
        data = bytes(data)
        return self._read(data, parse(data))

    def ReadWithConfig(self, data):
        data = bytes(data)
        info = parse(data)
        return self._read(data, info), IdspConfiguration(BlockSize=info.interleave_size)   # GetConfiguration (:59-65)

    @staticmethod
    def _read(data, info):
        buf = np.frombuffer(data, dtype=np.uint8)
        adpcm = [np.zeros(info.adpcm_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
        check(_lib.lib().vga_idsp_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), _ptr_array(u8p, adpcm)))
        return IdspReader._to_format(info, adpcm)

    @staticmethod
    def _to_format(info, adpcm):
        """ToAudioStream (:33-57): the stored contexts, nothing recomputed."""
        from .nwstm import _stored_format
        chans = []
        for c in range(info.channel_count):
            ch = GcAdpcmChannel(adpcm[c], np.array(info.coefs[c][:], dtype=np.int16), info.sample_count)
            ch.Gain = int(info.gain[c])
            ch.StartContext = GcAdpcmContext(*info.start_context[c][:])
            ch.LoopContext = GcAdpcmContext(*info.loop_context[c][:])
            ch.LoopContextStart = info.loop_start
            chans.append(ch)
        return _stored_format(chans, info.sample_rate, info.looping, info.loop_start, info.loop_end, None)
