"""NintendoWare streams for GC-ADPCM, PCM16 and PCM8 -- the host-side mirror of VGAudio/Containers/NintendoWare: BrstmWriter.cs,
BCFstmWriter.cs, BrstmReader.cs, BCFstmReader.cs, BxstmConfiguration.cs and Common.ToAdpcmStream.  Size math and
parsing run on the host (vga_nwstm_layout_for / vga_nwstm_parse); the images are assembled and taken apart on the
GPU (vga_nwstm_write / vga_nwstm_read; the vga_nwstm_pcm_* calls for PCM).  There is no CPU path."""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._fileset import FileSetBase, FileSetHandle, fetch_items, i64_or_none as _i64_or_none
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


# ---------------------------------------------------------------- sets of files on the device (include/vgaudio_hip/nw_files.h)
def _nw_file(channels, sample_rate, sample_count, looping=False, loop_start=0, loop_end=0):
    if not looping:
        loop_start = loop_end = 0
    return _lib.NwFileC(int(channels), int(sample_rate), int(sample_count), int(bool(looping)), int(loop_start), int(loop_end))


def _file_config(target, configuration=None):
    """vga_nw_file_config of a target and a BxstmConfiguration (None: the defaults)"""
    if isinstance(configuration, _lib.NwFileConfigC):
        return configuration
    c = configuration or BxstmConfiguration()
    if c.Codec != NwCodec.GcAdpcm:
        raise _lib.ArgumentError("sets of NintendoWare files hold GC-ADPCM streams (PCM streams go through the per-file writers)")
    if not (c.RecalculateSeekTable and c.RecalculateLoopContext):
        raise _lib.ArgumentError("only RecalculateSeekTable = RecalculateLoopContext = true is supported")
    if c.LoopPointAlignment < 0:
        raise _lib.ArgumentOutOfRangeError("negative loop point alignment")
    return _lib.NwFileConfigC(int(NwTarget(target)), c.SamplesPerInterleave, c.SamplesPerSeekTableEntry, c.LoopPointAlignment,
                              int(c.TrackType), int(c.SeekTableType), c.Version.Version if c.Version is not None else 0,
                              -1 if c.Endianness is None else int(c.Endianness))


class NwFileSet(FileSetBase):
    """A set of BRSTM / BCSTM / BFSTM files of different shapes, resident on the device (include/vgaudio_hip/nw_files.h has the
    layout): the channels of all files are the packed rows gcadpcm.AlignedFileSet leaves as its output, the seek tables one
    packed buffer, the images another.  `files`: one (channels, sample_rate, sample_count, looping, loop_start, loop_end) tuple or
    _lib.NwFileC per file, the loop the format's, before the writer aligns it; `target`: NwTarget; `configuration`: the
    BxstmConfiguration of the whole set (as VGAudio.Cli/Batch.cs applies one to every file).  The tensors are the caller's
    torch tensors on the current device; the calls run on torch's current stream and do not synchronise it."""
    _destroy = "vga_nw_files_destroy"

    def __init__(self, files=None, target=NwTarget.Revolution, configuration=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            cfg = _file_config(target, configuration)
            check(_lib.lib().vga_nw_files_create(arr, n, C.byref(cfg), C.byref(self._h)))
            self.image_sizes = [self.file_layout(arr[i], cfg).file_size for i in range(n)]
        self.totals = _lib.NwFilesTotalsC()
        check(_lib.lib().vga_nw_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, so, io = np.zeros(max(nf, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_nw_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), so.ctypes.data_as(i64p), io.ctypes.data_as(i64p)))
        self.first_channel, self.seek_offsets, self.image_offsets = fc[:nf], so[:nch], io[:nf]
        self.files, self.channels = nf, nch
        self.ragged = C.c_void_p(_lib.lib().vga_nw_files_ragged(self._h))        # borrowed: lives as long as this object

    @staticmethod
    def _files_array(files):
        files = [f if isinstance(f, _lib.NwFileC) else _nw_file(*f) for f in (files or [])]
        return (_lib.NwFileC * max(len(files), 1))(*files), len(files)

    @staticmethod
    def file_layout(f, cfg):
        """vga_nwstm_layout_for of one file of a set: the configuration plus the file's numbers"""
        p = _lib.NwParamsC()
        p.target, p.sample_rate, p.sample_count = cfg.target, f.sample_rate, f.sample_count
        p.looping, p.loop_start, p.loop_end = f.looping, f.loop_start, f.loop_end
        p.samples_per_interleave, p.samples_per_seek_table_entry = cfg.samples_per_interleave, cfg.samples_per_seek_table_entry
        p.loop_point_alignment, p.track_type, p.seek_table_type = cfg.loop_point_alignment, cfg.track_type, cfg.seek_table_type
        p.version, p.endianness = cfg.version, cfg.endianness
        L = _lib.NwLayoutC()
        check(_lib.lib().vga_nwstm_layout_for(C.byref(p), f.channels, C.byref(L)))
        return L

    @classmethod
    def layout(cls, files, target=NwTarget.Revolution, configuration=None):
        """(first_channel int32[files], seek_offsets int64[channels], image_offsets int64[files], NwFilesTotalsC): host only,
        needs no GPU"""
        arr, n = cls._files_array(files)
        cfg = _file_config(target, configuration)
        nch = sum(arr[i].channels for i in range(n) if arr[i].channels > 0)
        fc, so, io = np.zeros(max(n, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.NwFilesTotalsC(), C.POINTER(C.c_int64)
        check(_lib.lib().vga_nw_files_layout_for(arr, n, C.byref(cfg), fc.ctypes.data_as(C.POINTER(C.c_int)), so.ctypes.data_as(i64p),
                                                 io.ctypes.data_as(i64p), C.byref(tot)))
        return fc[:n], so[:tot.channels], io[:n], tot

    @classmethod
    def from_infos(cls, infos, image_offsets=None):
        """A set for reading, from the vga_nwstm_info of every file (parse()); image_offsets: multiples of 8, or None for images
        packed as write() packs them"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i in infos])
        offs = np.ascontiguousarray(image_offsets, dtype=np.int64) if image_offsets is not None else None
        h = C.c_void_p()
        check(_lib.lib().vga_nw_files_create_from_infos(ptrs, n, offs.ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None,
                                                        C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [i.audio_data_offset + i.audio_data_length for i in infos]
        return s

    def gc_files(self):
        """the _lib.GcFileC of every file (channel = vga_nwstm_layout_for(...).channel): what gcadpcm.AlignedFileSet takes"""
        arr = (_lib.GcFileC * max(self.files, 1))()
        check(_lib.lib().vga_nw_files_gc_files(self._h, arr))
        return list(arr[:self.files])

    def write(self, adpcm, coefs, images, gain=None, start_context=None, loop_context=None, seek=None, stream=None):
        """vga_nwstm_write_device_v.  adpcm: uint8[totals.adpcm_bytes] (the aligned rows), coefs: int16[channels*16], seek:
        int16[totals.seek_shorts]; images: uint8[totals.image_bytes]"""
        import torch
        from .dsp import DspFileSet
        ptr, t, n = DspFileSet._ptr, self.totals, self.channels
        check(_lib.lib().vga_nwstm_write_device_v(
            self._h, ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"), ptr(coefs, torch.int16, n * 16, "coefs"),
            ptr(gain, torch.int16, n, "gain"), ptr(start_context, torch.int16, n * 3, "start_context"),
            ptr(loop_context, torch.int16, n * 3, "loop_context"), ptr(seek, torch.int16, t.seek_shorts, "seek"),
            ptr(images, torch.uint8, t.image_bytes, "images"), DspFileSet._stream(stream)))

    def read(self, images, adpcm, coefs=None, gain=None, start_context=None, loop_context=None, stream=None):
        """vga_nwstm_read_device_v (a set from from_infos): images -> the rows of adpcm and the parsed per-channel arrays"""
        import torch
        from .dsp import DspFileSet
        ptr, t, n = DspFileSet._ptr, self.totals, self.channels
        check(_lib.lib().vga_nwstm_read_device_v(
            self._h, ptr(images, torch.uint8, t.image_bytes, "images"), ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"),
            ptr(coefs, torch.int16, n * 16, "coefs"), ptr(gain, torch.int16, n, "gain"),
            ptr(start_context, torch.int16, n * 3, "start_context"), ptr(loop_context, torch.int16, n * 3, "loop_context"),
            DspFileSet._stream(stream)))


def write_files(pcm16_list, target, configuration=None):
    """BrstmWriter / BCFstmWriter(target)(configuration).GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) for a list of Pcm16Format
    files -- with NwTarget.Revolution the whole of VGAudio.Cli/Batch.cs -- on the device and without a launch per file: one
    upload, vga_gcadpcm_coefs_device_v, vga_gcadpcm_encode_device_v, the alignment re-encode of gcadpcm.AlignedFileSet,
    vga_nwstm_write_device_v, one download.  Returns one `bytes` per file.  With configuration.Codec Pcm16Bit or Pcm8Bit the
    files are what GetFile(file) gives for that configuration, through vga_nwstm_pcm_write_device_v (NwPcmFileSet)."""
    import torch
    from .gcadpcm import AlignedFileSet
    files = list(pcm16_list)
    if isinstance(configuration, BxstmConfiguration) and configuration.Codec in (NwCodec.Pcm16Bit, NwCodec.Pcm8Bit):
        return _write_pcm_files(files, target, configuration)
    L = _lib.lib()
    s = NwFileSet([(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0,
                    f.LoopEnd if f.Looping else 0) for f in files], target, configuration)
    a = None
    try:
        if s.files == 0:
            return []
        a = AlignedFileSet(s.gc_files())
        t, nch = a.totals, a.channels
        if t.out_adpcm_bytes != s.totals.adpcm_bytes or list(a.seek_offsets) != list(s.seek_offsets):
            raise _lib.VgaError("internal: the aligned set's output is not the file set's input")
        pin, _ = a.offsets("in")
        host, c = np.zeros(t.pcm_samples, dtype=np.int16), 0
        for f in files:
            for ch in f.Channels:
                host[pin[c]:pin[c] + f.SampleCount] = np.asarray(ch, dtype=np.int16)[:f.SampleCount]
                c += 1
        new = lambda n, dtype: torch.zeros(max(int(n), 16), dtype=dtype, device="cuda")
        pcm = torch.from_numpy(host).cuda()
        coefs, adpcm, out = new(nch * 16, torch.int16), new(t.adpcm_bytes, torch.uint8), new(t.out_adpcm_bytes, torch.uint8)
        seek, ctx = new(t.seek_shorts, torch.int16), new(nch * 3, torch.int16)
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.vga_gcadpcm_ragged_coefs_workspace_bytes(a.ragged_in), t.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(L.vga_gcadpcm_coefs_device_v(a.ragged_in, pcm.data_ptr(), coefs.data_ptr(), ws.data_ptr(), ws.numel(), st))
        check(L.vga_gcadpcm_encode_device_v(a.ragged_in, pcm.data_ptr(), coefs.data_ptr(), None, None, adpcm.data_ptr(), st))
        a.align_channels(adpcm, coefs, out, seek=seek, loop_context=ctx, workspace=ws)
        s.write(out, coefs, images, loop_context=ctx, seek=seek)
        return s.images(images)
    finally:
        if a is not None:
            a.close()
        s.close()


# ------------------------------------------------ sets of PCM files on the device (include/vgaudio_hip_files/nw_pcm_files.h)
def _pcm_file_config(target, configuration):
    """(vga_nw_file_config, codec) of a target and a BxstmConfiguration whose Codec is Pcm16Bit or Pcm8Bit"""
    c = configuration or BxstmConfiguration(Codec=NwCodec.Pcm16Bit)
    if c.Codec not in (NwCodec.Pcm16Bit, NwCodec.Pcm8Bit):
        raise _lib.ArgumentError("sets of PCM NintendoWare files hold Pcm16Bit or Pcm8Bit streams (NwFileSet for GC-ADPCM)")
    cfg = _lib.NwFileConfigC(int(NwTarget(target)), c.SamplesPerInterleave, c.SamplesPerSeekTableEntry, c.LoopPointAlignment,
                             int(c.TrackType), int(c.SeekTableType), c.Version.Version if c.Version is not None else 0,
                             -1 if c.Endianness is None else int(c.Endianness))
    return cfg, int(c.Codec)


class NwPcmFileSet(FileSetHandle):
    """A set of PCM16 / PCM8 BRSTM / BCSTM / BFSTM files of different shapes, resident on the device
    (include/vgaudio_hip_files/nw_pcm_files.h has the layout): the channels of all files are packed int16 rows of ONE buffer,
    as wave.read_files_device leaves them, or at the caller's `pcm_offsets` (samples); the images one buffer, packed or at the
    caller's `image_offsets`.  `files`: one (channels, sample_rate, sample_count, looping, loop_start, loop_end) tuple or
    _lib.NwFileC per file; `target`: NwTarget; `configuration`: the BxstmConfiguration of the whole set, its Codec Pcm16Bit
    or Pcm8Bit.  The tensors are the caller's torch tensors on the current device; the calls run on torch's current stream
    and do not synchronise it."""
    _destroy = "vga_nw_pcm_files_destroy"

    def __init__(self, files=None, target=NwTarget.Revolution, configuration=None, pcm_offsets=None, image_offsets=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = NwFileSet._files_array(files)
            cfg, codec = _pcm_file_config(target, configuration)
            keep_p, po = _i64_or_none(pcm_offsets)
            keep_i, io = _i64_or_none(image_offsets)
            check(_lib.lib().vga_nw_pcm_files_create(arr, n, C.byref(cfg), codec, po, io, C.byref(self._h)))
            self.image_sizes = [self.file_layout(arr[i], cfg, codec).file_size for i in range(n)]
        self.totals = _lib.NwPcmFilesTotalsC()
        check(_lib.lib().vga_nw_pcm_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, po, io = np.zeros(max(nf, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_nw_pcm_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), po.ctypes.data_as(i64p), io.ctypes.data_as(i64p)))
        self.first_channel, self.pcm_offsets, self.image_offsets = fc[:nf], po[:nch], io[:nf]
        self.files, self.channels = nf, nch

    @staticmethod
    def file_params(f, cfg):
        """vga_nwstm_params of one file of a set: the configuration plus the file's numbers"""
        p = _lib.NwParamsC()
        p.target, p.sample_rate, p.sample_count = cfg.target, f.sample_rate, f.sample_count
        p.looping, p.loop_start, p.loop_end = f.looping, f.loop_start, f.loop_end
        p.samples_per_interleave, p.samples_per_seek_table_entry = cfg.samples_per_interleave, cfg.samples_per_seek_table_entry
        p.loop_point_alignment, p.track_type, p.seek_table_type = cfg.loop_point_alignment, cfg.track_type, cfg.seek_table_type
        p.version, p.endianness = cfg.version, cfg.endianness
        return p

    @classmethod
    def file_layout(cls, f, cfg, codec):
        """vga_nwstm_pcm_layout_for of one file of a set"""
        p, L = cls.file_params(f, cfg), _lib.NwLayoutC()
        check(_lib.lib().vga_nwstm_pcm_layout_for(C.byref(p), int(codec), f.channels, C.byref(L)))
        return L

    @classmethod
    def layout(cls, files, target=NwTarget.Revolution, configuration=None, pcm_offsets=None, image_offsets=None):
        """(first_channel int32[files], pcm_offsets int64[channels], image_offsets int64[files], NwPcmFilesTotalsC): host only,
        needs no GPU"""
        arr, n = NwFileSet._files_array(files)
        cfg, codec = _pcm_file_config(target, configuration)
        nch = sum(arr[i].channels for i in range(n) if arr[i].channels > 0)
        fc, po, io = np.zeros(max(n, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.NwPcmFilesTotalsC(), C.POINTER(C.c_int64)
        keep_p, pin = _i64_or_none(pcm_offsets)
        keep_i, iin = _i64_or_none(image_offsets)
        check(_lib.lib().vga_nw_pcm_files_layout_for(arr, n, C.byref(cfg), codec, pin, iin, fc.ctypes.data_as(C.POINTER(C.c_int)),
                                                     po.ctypes.data_as(i64p), io.ctypes.data_as(i64p), C.byref(tot)))
        return fc[:n], po[:tot.channels], io[:n], tot

    @classmethod
    def from_infos(cls, infos, pcm_offsets=None, image_offsets=None):
        """A set for reading, from the vga_nwstm_info of every file (parse_pcm()); image_offsets: any byte offsets, or None
        for images packed as a set for writing packs them"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i in infos])
        keep_p, po = _i64_or_none(pcm_offsets)
        keep_i, io = _i64_or_none(image_offsets)
        h = C.c_void_p()
        check(_lib.lib().vga_nw_pcm_files_create_from_infos(ptrs, n, po, io, C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [i.audio_data_offset + i.audio_data_length for i in infos]
        return s

    @staticmethod
    def _items(call, args, pcm_offsets, image_offsets, general):
        keep_p, po = _i64_or_none(pcm_offsets)
        keep_i, io = _i64_or_none(image_offsets)
        return fetch_items(call, (*args, po, io, int(general)), _lib.NwPcmFilesItemC)

    @classmethod
    def write_items(cls, files, target=NwTarget.Revolution, configuration=None, pcm_offsets=None, image_offsets=None, general=False):
        """the work items of vga_nwstm_pcm_write_device_v on such a set (_lib.NwPcmFilesItemC), host only"""
        arr, n = NwFileSet._files_array(files)
        cfg, codec = _pcm_file_config(target, configuration)
        return cls._items(_lib.lib().vga_nw_pcm_files_write_items_for, (arr, n, C.byref(cfg), codec), pcm_offsets, image_offsets, general)

    @classmethod
    def read_items(cls, infos, pcm_offsets=None, image_offsets=None, general=False):
        """the work items of vga_nwstm_pcm_read_device_v on a set of such infos, host only"""
        infos = list(infos)
        ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos])
        return cls._items(_lib.lib().vga_nw_pcm_files_read_items_for, (ptrs, len(infos)), pcm_offsets, image_offsets, general)

    def offsets(self):
        """(first_channel, pcm_offsets, image_offsets) of the object"""
        return self.first_channel, self.pcm_offsets, self.image_offsets

    def stats(self):
        """(vector files, general files, vector items, general items) of a call made by this thread now"""
        out = (C.c_int64 * 4)()
        check(_lib.lib().vga_nw_pcm_files_stats(self._h, out))
        return tuple(out)

    def write(self, pcm, images, stream=None):
        """vga_nwstm_pcm_write_device_v.  pcm: int16[totals.pcm_samples] (the rows); images: uint8[totals.image_bytes]"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t = self.totals
        check(_lib.lib().vga_nwstm_pcm_write_device_v(self._h, ptr(pcm, torch.int16, t.pcm_samples, "pcm"),
                                                      ptr(images, torch.uint8, t.image_bytes, "images"), stream_handle(stream)))

    def read(self, images, pcm, stream=None):
        """vga_nwstm_pcm_read_device_v (a set from from_infos).  images: uint8[totals.image_bytes]; pcm: int16[totals.pcm_samples]"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t = self.totals
        check(_lib.lib().vga_nwstm_pcm_read_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"),
                                                     ptr(pcm, torch.int16, t.pcm_samples, "pcm"), stream_handle(stream)))

    def images(self, host_buffer):
        """one `bytes` per file from the images' buffer (a device tensor or a numpy array); synchronises"""
        host = host_buffer.cpu().numpy() if hasattr(host_buffer, "cpu") else np.asarray(host_buffer, dtype=np.uint8)
        return [host[int(at):int(at) + int(size)].tobytes() for at, size in zip(self.image_offsets, self.image_sizes)]


def _write_pcm_files(files, target, configuration):
    """write_files for a configuration whose Codec is Pcm16Bit or Pcm8Bit: one upload into the packed rows,
    vga_nwstm_pcm_write_device_v, one download"""
    import torch
    for i, f in enumerate(files):
        if not isinstance(f, Pcm16Format):
            raise _lib.ArgumentError("file %d: write_files takes Pcm16Format files (decode with ToPcm16 first)" % i)
    described = [(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0, f.LoopEnd if f.Looping else 0)
                 for f in files]
    _, offsets, _, totals = NwPcmFileSet.layout(described, target, configuration)   # every refusal of a file, before anything is allocated
    if not files:
        return []
    host, c = np.zeros(totals.pcm_samples, dtype=np.int16), 0
    for f in files:
        for ch in f.Channels:
            host[int(offsets[c]):int(offsets[c]) + f.SampleCount] = np.asarray(ch, dtype=np.int16)[:f.SampleCount]
            c += 1
    s = NwPcmFileSet(described, target, configuration)
    try:
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        s.write(torch.from_numpy(host).cuda(), images)
        return s.images(images)
    finally:
        s.close()


def read_pcm_files(list_of_bytes):
    """BrstmReader / BCFstmReader.ReadFormat(file) for a list of PCM16 / PCM8 streams, without a launch per file: one upload,
    one vga_nwstm_pcm_read_device_v, one download.  One Pcm16Format per file with the stream's loop and tracks; a PCM8 stream
    comes as its Pcm8SignedFormat's ToPcm16() would give it (the set's rows are int16)."""
    import torch
    datas = [bytes(d) for d in list_of_bytes]
    if not datas:
        return []
    infos = [parse_pcm(d) for d in datas]
    s = NwPcmFileSet.from_infos(infos)
    try:
        host = np.zeros(s.totals.image_bytes, dtype=np.uint8)
        for d, at, size in zip(datas, s.image_offsets, s.image_sizes):
            host[int(at):int(at) + size] = np.frombuffer(d, dtype=np.uint8)[:size]
        pcm = torch.zeros(s.totals.pcm_samples, dtype=torch.int16, device="cuda")
        s.read(torch.from_numpy(host).cuda(), pcm)
        rows, offsets = pcm.cpu().numpy(), s.pcm_offsets
    finally:
        s.close()
    out, c = [], 0
    for info in infos:
        chans = [rows[int(offsets[c + i]):int(offsets[c + i]) + info.sample_count].copy() for i in range(info.channel_count)]
        c += info.channel_count
        fmt = Pcm16Format(chans, info.sample_rate).WithLoop(bool(info.looping), info.loop_start, info.sample_count)
        tracks = [AudioTrack(t.channel_count, t.left, t.right, t.volume, t.panning) for t in info.tracks[:info.track_count]]
        fmt.Tracks = tracks if tracks else AudioTrack.GetDefaultTrackList(info.channel_count)
        out.append(fmt)
    return out
