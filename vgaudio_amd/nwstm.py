"""NintendoWare streams for GC-ADPCM, PCM16 and PCM8 -- the host-side mirror of VGAudio/Containers/NintendoWare: BrstmWriter.cs,
BCFstmWriter.cs, BrstmReader.cs, BCFstmReader.cs, BxstmConfiguration.cs and Common.ToAdpcmStream.  Size math and
parsing run on the host (vga_nwstm_layout_for / vga_nwstm_parse); the images are assembled and taken apart on the
GPU (vga_nwstm_write / vga_nwstm_read; the vga_nwstm_pcm_* calls for PCM).  There is no CPU path."""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import check, i16p, u8p
from .gcadpcm import AudioTrack, GcAdpcmChannel, GcAdpcmContext, GcAdpcmFormat, Pcm16Format, _i16, _ptr_array
from .pcm8 import Pcm8Format, Pcm8SignedFormat

DEFAULT_SAMPLES = 14336                          # BytesToSamples(0x2000, GcAdpcm) (BxstmConfiguration.cs:17)


class NwTarget(enum.IntEnum):                    # NwTarget.cs
    Revolution = 0                               # BRSTM
    Ctr = 1                                      # BCSTM
    Cafe = 2                                     # BFSTM


class NwCodec(enum.IntEnum):                     # NwCodec.cs
    Pcm8Bit = 0
    Pcm16Bit = 1
    GcAdpcm = 2
    ImaAdpcm = 3


class BrstmTrackType(enum.IntEnum):              # Structures/BrstmTrackType.cs (the C ABI numbers Short 1)
    Standard = 0
    Short = 1


class BrstmSeekTableType(enum.IntEnum):          # Structures/BrstmSeekTableType.cs
    Standard = 0
    Short = 1


class Endianness(enum.IntEnum):
    LittleEndian = 0
    BigEndian = 1


class NwVersion:
    """NwVersion.cs: major.minor.micro.revision packed into one 32-bit word."""

    def __init__(self, major=0, minor=0, micro=0, revision=0):
        self.Version = (major << 24 | minor << 16 | micro << 8 | revision) & 0xFFFFFFFF

    @classmethod
    def FromPacked(cls, version):
        v = cls()
        v.Version = int(version) & 0xFFFFFFFF
        return v

    Major = property(lambda self: self.Version >> 24)
    Minor = property(lambda self: self.Version >> 16 & 0xFF)
    Micro = property(lambda self: self.Version >> 8 & 0xFF)
    Revision = property(lambda self: self.Version & 0xFF)

    def __eq__(self, other):
        return isinstance(other, NwVersion) and other.Version == self.Version

    def __repr__(self):
        return "NwVersion(%d, %d, %d, %d)" % (self.Major, self.Minor, self.Micro, self.Revision)


def BytesToSamples(byteCount, codec):            # Common.cs:30-43
    codec = NwCodec(codec)
    if codec == NwCodec.GcAdpcm:
        return byteCount // 8 * 14 + max(byteCount % 8 * 2 - 2, 0)
    return {NwCodec.Pcm16Bit: byteCount // 2, NwCodec.Pcm8Bit: byteCount}.get(codec, 0)


class BxstmConfiguration:
    """BxstmConfiguration.cs: the options of the BRSTM, BCSTM and BFSTM writers.  An option left at None follows the
    codec: BytesToSamples(0x2000, Codec), i.e. 14336 for GC-ADPCM, 4096 for PCM16 and 8192 for PCM8."""

    def __init__(self, SamplesPerInterleave=None, SamplesPerSeekTableEntry=None,
                 LoopPointAlignment=None, Endianness=None, Version=None, TrackType=BrstmTrackType.Standard,
                 SeekTableType=BrstmSeekTableType.Standard, RecalculateSeekTable=True, RecalculateLoopContext=True,
                 Codec=NwCodec.GcAdpcm):
        self.Codec = NwCodec(Codec)
        self._spi = self._spe = self._align = None
        if SamplesPerInterleave is not None:
            self.SamplesPerInterleave = SamplesPerInterleave
        if SamplesPerSeekTableEntry is not None:
            self.SamplesPerSeekTableEntry = SamplesPerSeekTableEntry
        if LoopPointAlignment is not None:
            self.LoopPointAlignment = LoopPointAlignment
        self.Endianness = Endianness
        self.Version = Version
        self.TrackType = BrstmTrackType(TrackType)
        self.SeekTableType = BrstmSeekTableType(SeekTableType)
        self.RecalculateSeekTable = RecalculateSeekTable
        self.RecalculateLoopContext = RecalculateLoopContext

    def _default(self):
        return BytesToSamples(0x2000, self.Codec)

    @property
    def SamplesPerInterleave(self):
        return self._spi if self._spi is not None else self._default()

    @SamplesPerInterleave.setter
    def SamplesPerInterleave(self, value):       # :42-59 (the divisible-by-14 rule is GC-ADPCM's)
        if value < 1:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be positive")
        if self.Codec == NwCodec.GcAdpcm and value % 14 != 0:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be divisible by 14")
        self._spi = int(value)

    @property
    def LoopPointAlignment(self):
        return self._align if self._align is not None else self._default()

    @LoopPointAlignment.setter
    def LoopPointAlignment(self, value):
        self._align = int(value)

    @property
    def SamplesPerSeekTableEntry(self):
        return self._spe if self._spe is not None else self._default()

    @SamplesPerSeekTableEntry.setter
    def SamplesPerSeekTableEntry(self, value):   # :70-80
        if value < 2:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be 2 or greater")
        self._spe = int(value)


class _NwWriter:
    """AudioWriter<_, BxstmConfiguration>.GetFile(format, configuration) for a GcAdpcmFormat."""
    target = None

    def __init__(self, configuration=None):
        self.Configuration = configuration or BxstmConfiguration()

    def _params(self, fmt, track_count):
        c = self.Configuration
        if c.LoopPointAlignment < 0:
            raise _lib.ArgumentOutOfRangeError("negative loop point alignment")
        align = c.LoopPointAlignment
        # SetupWriter (BrstmWriter.cs:88-103): WithAlignment only when the loop start is not aligned yet
        if not (align == 0 or fmt.LoopStart % align == 0) or not fmt.AlignmentMultiple:
            mult = align
        else:
            mult = fmt.AlignmentMultiple
        p = _lib.NwParamsC()
        p.target = int(self.target)
        p.sample_rate = fmt.SampleRate
        p.sample_count = fmt.UnalignedSampleCount
        p.looping = int(fmt.Looping)
        p.loop_start, p.loop_end = fmt.UnalignedLoopStart, fmt.UnalignedLoopEnd
        p.samples_per_interleave = c.SamplesPerInterleave
        p.samples_per_seek_table_entry = c.SamplesPerSeekTableEntry
        p.loop_point_alignment = mult
        p.track_type, p.seek_table_type = int(c.TrackType), int(c.SeekTableType)
        p.version = c.Version.Version if c.Version is not None else 0
        p.endianness = -1 if c.Endianness is None else int(c.Endianness)
        p.track_count = track_count
        p.keep_seek_table = int(not c.RecalculateSeekTable)
        p.keep_loop_context = int(not c.RecalculateLoopContext)
        return p

    def Layout(self, fmt):
        """Every size and offset the writer derives (no device work)."""
        L = _lib.NwLayoutC()
        p = self._params(fmt, len(fmt.Tracks))
        check(_lib.lib().vga_nwstm_layout_for(C.byref(p), fmt.ChannelCount, C.byref(L)))
        return L

    def _pcm_params(self, fmt, track_count):
        c = self.Configuration
        p = _lib.NwParamsC()
        p.target = int(self.target)
        p.sample_rate = fmt.SampleRate
        p.sample_count = fmt.SampleCount
        p.looping = int(fmt.Looping)
        p.loop_start, p.loop_end = fmt.LoopStart, fmt.LoopEnd
        p.samples_per_interleave = c.SamplesPerInterleave
        p.samples_per_seek_table_entry = c.SamplesPerSeekTableEntry
        p.loop_point_alignment = c.LoopPointAlignment
        p.track_type, p.seek_table_type = int(c.TrackType), int(c.SeekTableType)
        p.version = c.Version.Version if c.Version is not None else 0
        p.endianness = -1 if c.Endianness is None else int(c.Endianness)
        p.track_count = track_count
        return p

    def PcmLayout(self, fmt):
        """vga_nwstm_pcm_layout_for for the configured PCM codec (no device work)."""
        L = _lib.NwLayoutC()
        tracks = getattr(fmt, "Tracks", None) or AudioTrack.GetDefaultTrackList(fmt.ChannelCount)
        p = self._pcm_params(fmt, len(tracks))
        check(_lib.lib().vga_nwstm_pcm_layout_for(C.byref(p), int(self.Configuration.Codec), fmt.ChannelCount, C.byref(L)))
        return L

    def _get_pcm_file(self, audio):
        """SetupWriter's Pcm16Bit / Pcm8Bit branches: GetFormat<Pcm16Format> / GetFormat<Pcm8SignedFormat>.  A
        Pcm16Format is converted on the device while it is interleaved (EncodeSigned for PCM8)."""
        codec = self.Configuration.Codec
        if isinstance(audio, Pcm8SignedFormat) and codec == NwCodec.Pcm8Bit:
            rows, kind = audio.Channels, VGA_SAMPLES_8BIT
        elif isinstance(audio, Pcm16Format):
            rows, kind = audio.Channels, VGA_SAMPLES_S16
        elif isinstance(audio, Pcm8Format):
            return self._get_pcm_file(audio.ToPcm16())
        else:
            raise _lib.ArgumentError("a %s stream is written from a Pcm16Format or Pcm8SignedFormat" % codec.name)
        tracks = list(getattr(audio, "Tracks", None) or AudioTrack.GetDefaultTrackList(audio.ChannelCount))
        p = self._pcm_params(audio, len(tracks))
        L = _lib.NwLayoutC()
        check(_lib.lib().vga_nwstm_pcm_layout_for(C.byref(p), int(codec), audio.ChannelCount, C.byref(L)))
        tr = (_lib.NwTrackC * max(len(tracks), 1))()
        for i, t in enumerate(tracks):
            tr[i] = _lib.NwTrackC(t.ChannelCount, t.ChannelLeft, t.ChannelRight, t.Volume, t.Panning)
        dtype = np.int16 if kind == VGA_SAMPLES_S16 else np.uint8
        rows = [np.ascontiguousarray(r, dtype=dtype) for r in rows]
        ptrs = (C.c_void_p * max(len(rows), 1))(*[r.ctypes.data for r in rows])
        out = np.zeros(L.file_size, dtype=np.uint8)
        check(_lib.lib().vga_nwstm_pcm_write(C.byref(p), int(codec), audio.ChannelCount, tr, ptrs, kind, out.ctypes.data_as(u8p)))
        return out.tobytes()

    def GetFile(self, audio, configuration=None):
        if configuration is not None:
            self.Configuration = configuration
        if self.Configuration.Codec in (NwCodec.Pcm16Bit, NwCodec.Pcm8Bit):
            return self._get_pcm_file(audio)
        if not isinstance(audio, GcAdpcmFormat):
            raise _lib.ArgumentError("the NintendoWare writers take a GcAdpcmFormat (encode PCM with EncodeFromPcm16 first)")
        tracks = list(audio.Tracks)
        p = self._params(audio, len(tracks))
        L = _lib.NwLayoutC()
        check(_lib.lib().vga_nwstm_layout_for(C.byref(p), audio.ChannelCount, C.byref(L)))
        ch = L.channel
        # the channels rebuilt with LoopAlignmentMultiple and SamplesPerSeekTableEntry (one batched device call)
        fmt = audio._clone(alignmentMultiple=ch.loop_alignment_multiple,
                           samplesPerSeekTableEntry=ch.samples_per_seek_table_entry)
        nch = fmt.ChannelCount
        adpcm = [np.ascontiguousarray(c.GetAdpcmAudio(), dtype=np.uint8) for c in fmt.Channels]
        if any(len(a) != L.channel_adpcm_bytes for a in adpcm):
            raise _lib.ArgumentOutOfRangeError("Inputs must be of equal length")                  # Interleave.cs:49-50
        seek = [np.ascontiguousarray(c.GetSeekTable(), dtype=np.int16) for c in fmt.Channels]
        entries = min(len(s) // 2 for s in seek)
        coefs = np.ascontiguousarray(np.stack([c.Coefs for c in fmt.Channels]), dtype=np.int16).reshape(nch, 16)
        gain = np.array([c.Gain for c in fmt.Channels], dtype=np.int16)
        start = np.array([[c.StartContext.PredScale, c.StartContext.Hist1, c.StartContext.Hist2] for c in fmt.Channels],
                         dtype=np.int16)
        loop = np.array([[c.LoopContext.PredScale, c.LoopContext.Hist1, c.LoopContext.Hist2] for c in fmt.Channels],
                        dtype=np.int16)
        tr = (_lib.NwTrackC * max(len(tracks), 1))()
        for i, t in enumerate(tracks):
            tr[i] = _lib.NwTrackC(t.ChannelCount, t.ChannelLeft, t.ChannelRight, t.Volume, t.Panning)
        out = np.zeros(L.file_size, dtype=np.uint8)
        check(_lib.lib().vga_nwstm_write(C.byref(p), nch, tr, _ptr_array(u8p, adpcm), L.channel_adpcm_bytes, _i16(coefs),
                                         _i16(gain), _i16(start), _i16(loop),
                                         _ptr_array(i16p, seek) if entries else None, entries, out.ctypes.data_as(u8p)))
        return out.tobytes()


class BrstmWriter(_NwWriter):
    """BrstmWriter.cs"""
    target = NwTarget.Revolution


class BCFstmWriter(_NwWriter):
    """BCFstmWriter.cs: BCFstmWriter(NwTarget.Ctr) writes BCSTM, BCFstmWriter(NwTarget.Cafe) BFSTM."""

    def __init__(self, target, configuration=None):
        super().__init__(configuration)
        if NwTarget(target) == NwTarget.Revolution:
            raise _lib.ArgumentError("BCFstmWriter writes BCSTM (NwTarget.Ctr) or BFSTM (NwTarget.Cafe)")
        self.target = NwTarget(target)


VGA_SAMPLES_S16, VGA_SAMPLES_8BIT = 0, 1          # include/vgaudio_hip_pcm.h


def parse_pcm(data):
    """vga_nwstm_pcm_parse: a PCM8 / PCM16 stream's header and tracks (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.NwInfoC()
    check(_lib.lib().vga_nwstm_pcm_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


def parse(data):
    """vga_nwstm_parse: the stream's header, tracks and channel infos (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.NwInfoC()
    check(_lib.lib().vga_nwstm_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


def _stored_format(channels, sample_rate, looping, loop_start, loop_end, tracks):
    """GcAdpcmFormatBuilder(channels, rate).WithTracks(..).WithLoop(..).Build() for channels that carry what the
    file stored (Common.cs:90-95): the stored loop context and seek table are kept, nothing is recomputed."""
    fmt = GcAdpcmFormat([], sample_rate)
    fmt.Channels = channels
    fmt.Looping = bool(looping)
    fmt.UnalignedLoopStart = loop_start if looping else 0
    fmt.UnalignedLoopEnd = loop_end if looping else 0
    fmt.Tracks = list(tracks) if tracks else AudioTrack.GetDefaultTrackList(len(channels))
    if channels:
        fmt.SamplesPerSeekTableEntry = channels[0].SamplesPerSeekTableEntry
    return fmt


class _NwReader:
    """AudioReader<_, BxstmStructure, BxstmConfiguration>: ReadFormat(bytes) -> GcAdpcmFormat."""
    magics = ()

    def ReadInfo(self, data):
        info = parse(data)
        if bytes(data[:4]) not in self.magics:
            raise _lib.InvalidDataError("File has no %s header" % " or ".join(m.decode() for m in self.magics))
        return info

    def ReadFormat(self, data):
        data = bytes(data)
        info = self.ReadInfo(data)
        nch = info.channel_count
        buf = np.frombuffer(data, dtype=np.uint8)
        adpcm = [np.zeros(info.adpcm_bytes, dtype=np.uint8) for _ in range(nch)]
        seek = [np.zeros(info.seek_entries * 2, dtype=np.int16) for _ in range(nch)] if info.seek_entries else None
        check(_lib.lib().vga_nwstm_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), _ptr_array(u8p, adpcm),
                                        _ptr_array(i16p, seek) if seek else None))
        return self._to_format(info, adpcm, seek)

    def ReadAnyFormat(self, data):
        """AudioReader.ReadFormat through Common.ToAudioStream (Common.cs:45-65): GcAdpcmFormat, Pcm16Format or
        Pcm8SignedFormat by the stream's codec byte.  The loop end reads back as SampleCount (Common.cs:105,114)."""
        data = bytes(data)
        if len(data) >= 4 and data[:4] not in self.magics:
            parse(data)                                          # the reference's refusal for a foreign file
            raise _lib.InvalidDataError("File has no %s header" % " or ".join(m.decode() for m in self.magics))
        try:
            info = parse_pcm(data)
        except _lib.InvalidOperationError:
            return self.ReadFormat(data)                         # GC-ADPCM (or a refusal of vga_nwstm_parse)
        nch = info.channel_count
        pcm16 = info.codec == NwCodec.Pcm16Bit
        rows = [np.zeros(info.sample_count, dtype=np.int16 if pcm16 else np.uint8) for _ in range(nch)]
        ptrs = (C.c_void_p * nch)(*[r.ctypes.data for r in rows])
        buf = np.frombuffer(data, dtype=np.uint8)
        check(_lib.lib().vga_nwstm_pcm_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), ptrs,
                                            VGA_SAMPLES_S16 if pcm16 else VGA_SAMPLES_8BIT))
        fmt = Pcm16Format(rows, info.sample_rate) if pcm16 else Pcm8SignedFormat(rows, info.sample_rate)
        fmt.WithLoop(bool(info.looping), info.loop_start, info.sample_count)
        tracks = [AudioTrack(t.channel_count, t.left, t.right, t.volume, t.panning) for t in info.tracks[:info.track_count]]
        fmt.Tracks = tracks if tracks else AudioTrack.GetDefaultTrackList(nch)
        return fmt

    @staticmethod
    def _to_format(info, adpcm, seek):
        """Common.ToAdpcmStream (Common.cs:67-97)."""
        chans = []
        for c in range(info.channel_count):
            ch = GcAdpcmChannel(adpcm[c], np.array(info.coefs[c][:], dtype=np.int16), info.sample_count)
            ch.Gain = int(info.gain[c])
            ch.StartContext = GcAdpcmContext(*info.start_context[c][:])
            if info.looping:                                     # WithLoopContext(LoopStart, ...)
                ch.LoopContext = GcAdpcmContext(*info.loop_context[c][:])
                ch.LoopContextStart = info.loop_start
            if seek is not None:                                 # WithSeekTable(table, SamplesPerSeekTableEntry)
                ch._seek = seek[c]
                ch.SamplesPerSeekTableEntry = info.samples_per_seek_table_entry
            chans.append(ch)
        tracks = [AudioTrack(t.channel_count, t.left, t.right, t.volume, t.panning) for t in info.tracks[:info.track_count]]
        return _stored_format(chans, info.sample_rate, info.looping, info.loop_start, info.sample_count, tracks)


class BrstmReader(_NwReader):
    """BrstmReader.cs"""
    magics = (b"RSTM",)


class BCFstmReader(_NwReader):
    """BCFstmReader.cs (streams only: CWAV / FWAV and prefetch files raise InvalidOperationError)"""
    magics = (b"CSTM", b"FSTM")


def configuration_of(info):
    """GetConfiguration (BrstmReader.cs:40-54, BCFstmReader.cs:52-69): the options that write the file again."""
    c = BxstmConfiguration(Codec=info.codec)
    if info.codec == NwCodec.GcAdpcm or info.target != NwTarget.Revolution:
        c.SamplesPerSeekTableEntry = info.samples_per_seek_table_entry
    c.SamplesPerInterleave = info.samples_per_interleave
    if info.target == NwTarget.Revolution:
        c.TrackType = BrstmTrackType(info.track_type)
        c.SeekTableType = BrstmSeekTableType(info.seek_table_type)
    else:
        c.Endianness = Endianness(info.endianness)
        c.Version = NwVersion.FromPacked(info.version)
    return c
