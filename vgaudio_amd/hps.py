"""HPS (HAL DSP stream) for GC-ADPCM -- the host-side mirror of VGAudio/Containers/Hps: HpsWriter.cs, HpsReader.cs and
HpsConfiguration.cs.  Size math, the block map and parsing run on the host (vga_hps_layout_for, vga_hps_block_map,
vga_hps_parse); the images are assembled and taken apart on the GPU (vga_hps_write, vga_hps_read).  There is no CPU
path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, i16p, u8p
from .gcadpcm import GcAdpcmChannel, GcAdpcmContext, GcAdpcmDecoder, GcAdpcmFormat, GcAdpcmParameters, _i16, _ptr_array


class HpsConfiguration:
    """HpsConfiguration.cs: no options of its own."""


def _contexts(channels):
    return np.array([[c.StartContext.PredScale, c.StartContext.Hist1, c.StartContext.Hist2] for c in channels], dtype=np.int16)


class HpsWriter:
    """AudioWriter<HpsWriter, HpsConfiguration>.GetFile(format, configuration) for a GcAdpcmFormat."""

    def __init__(self, configuration=None):
        self.Configuration = configuration or HpsConfiguration()

    @staticmethod
    def _params(fmt):
        return _lib.HpsParamsC(fmt.SampleRate, fmt.UnalignedSampleCount, int(fmt.Looping), fmt.UnalignedLoopStart,
                               fmt.UnalignedLoopEnd)

    def Layout(self, fmt):
        """The sizes SetupWriter and CreateBlockMap derive (no device work)."""
        L = _lib.HpsLayoutC()
        check(_lib.lib().vga_hps_layout_for(C.byref(self._params(fmt)), fmt.ChannelCount, C.byref(L)))
        return L

    def BlockMap(self, fmt):
        """CreateBlockMap (HpsWriter.cs:114-160): one vga_hps_block per block."""
        L = self.Layout(fmt)
        blocks = (_lib.HpsBlockC * L.block_count)()
        check(_lib.lib().vga_hps_block_map(C.byref(self._params(fmt)), fmt.ChannelCount, blocks, L.block_count))
        return list(blocks)

    @staticmethod
    def HistSource(audio, built, L):
        """The rows WriteBlock's GetHist1 / GetHist2 index: the channels' Pcm field after SetupWriter.  Without
        alignment the final rebuild decodes the audio (EnsureLoopContextIsSelfCalculated); with it, the field is what
        the format carried into WithAlignment -- the decode of the unaligned audio, or None for channels whose loop
        context was read from a file.  Returns a list of rows or None (zeros)."""
        if L.alignment_needed:
            rows = [c.Pcm for c in audio.Channels]
            return None if any(r is None for r in rows) else rows
        if all(c._pcm is not None for c in built.Channels):
            return [c._pcm for c in built.Channels]
        return GcAdpcmDecoder.Decode([c.GetAdpcmAudio() for c in built.Channels], np.stack([c.Coefs for c in built.Channels]),
                                     GcAdpcmParameters(SampleCount=built.Channels[0].SampleCount))

    def GetFile(self, audio, configuration=None):
        if configuration is not None:
            self.Configuration = configuration
        if not isinstance(audio, GcAdpcmFormat):
            raise _lib.ArgumentError("HpsWriter takes a GcAdpcmFormat (encode PCM with EncodeFromPcm16 first)")
        p = self._params(audio)
        L = self.Layout(audio)
        built = audio._clone(alignmentMultiple=L.channel.loop_alignment_multiple)     # one batched channel build
        nch = built.ChannelCount
        adpcm = [np.ascontiguousarray(c.GetAdpcmAudio(), dtype=np.uint8) for c in built.Channels]
        if any(len(a) != L.channel_adpcm_bytes for a in adpcm):
            raise _lib.ArgumentError("channel audio does not match the layout")
        hist = self.HistSource(audio, built, L)
        hist = [np.ascontiguousarray(h, dtype=np.int16) for h in hist] if hist is not None else None
        pcm_len = min(len(h) for h in hist) if hist else 0
        coefs = np.ascontiguousarray(np.stack([c.Coefs for c in built.Channels]), dtype=np.int16).reshape(nch, 16)
        gain = np.array([c.Gain for c in audio.Channels], dtype=np.int16)          # GetCloneBuilder keeps Gain / StartContext
        start = _contexts(audio.Channels)
        out = np.zeros(L.file_size, dtype=np.uint8)
        check(_lib.lib().vga_hps_write(C.byref(p), nch, _ptr_array(u8p, adpcm), L.channel_adpcm_bytes, _i16(coefs), _i16(gain),
                                       _i16(start), _ptr_array(i16p, hist) if hist else None, pcm_len, out.ctypes.data_as(u8p)))
        return out.tobytes()


def parse(data):
    """vga_hps_parse: (info, [vga_hps_block_info]) -- the header, the block chain and the loop (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.HpsInfoC()
    check(_lib.lib().vga_hps_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info), None, 0))
    blocks = (_lib.HpsBlockInfoC * max(info.block_count, 1))()
    check(_lib.lib().vga_hps_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info), blocks, info.block_count))
    return info, blocks


class HpsReader:
    """AudioReader<HpsReader, HpsStructure, HpsConfiguration>: ReadFormat(bytes) -> GcAdpcmFormat."""

    def ReadMetadata(self, data):
        return parse(data)[0]

    def ReadFormat(self, data):
        return self.ReadWithConfig(data)[0]

    def ReadWithConfig(self, data):
        data = bytes(data)
        info, blocks = parse(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        adpcm = [np.zeros(info.adpcm_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
        check(_lib.lib().vga_hps_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), blocks, _ptr_array(u8p, adpcm)))
        return self._to_format(info, adpcm), HpsConfiguration()

    @staticmethod
    def _to_format(info, adpcm):
        """ToAudioStream (:33-65): the stored contexts, a loop that ends at the sample count."""
        from .nwstm import _stored_format
        chans = []
        for c in range(info.channel_count):
            ch = GcAdpcmChannel(adpcm[c], np.array(info.coefs[c][:], dtype=np.int16), info.sample_count)
            ch.Gain = int(info.gain[c])
            ch.StartContext = GcAdpcmContext(*info.start_context[c][:])
            ch.LoopContext = GcAdpcmContext(*info.loop_context[c][:])
            ch.LoopContextStart = info.loop_start
            chans.append(ch)
        return _stored_format(chans, info.sample_rate, info.looping, info.loop_start, info.sample_count, None)
