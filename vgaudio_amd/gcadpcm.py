"""Host-side mirror of the reference's GC-ADPCM codec and format classes, routed
through the C ABI (include/vgaudio_hip.h) into the HIP kernels.

Mirrors (reference paths relative to /root/reference/src/VGAudio/):
  GcAdpcmMath            Codecs/GcAdpcm/GcAdpcmMath.cs:7-47
  GcAdpcmParameters      Codecs/GcAdpcm/GcAdpcmParameters.cs:3-7 (+ CodecParameters.cs:5-6)
  GcAdpcmCoefficients    Codecs/GcAdpcm/GcAdpcmCoefficients.cs:9
  GcAdpcmEncoder         Codecs/GcAdpcm/GcAdpcmEncoder.cs:14,48
  GcAdpcmDecoder         Codecs/GcAdpcm/GcAdpcmDecoder.cs:10
  Pcm16Format            Formats/Pcm16/Pcm16Format.cs:14
  GcAdpcmChannel/Format  Formats/GcAdpcm/GcAdpcmFormat.cs:42-74,129-135

Same names, argument meaning and error behaviour (exceptions map 1:1, see
_lib.py).  Every method is one batched call into the GPU library; nothing here
computes codec results on the CPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetHandle
from ._lib import check, i16p, u8p


def _i16(a):
    return a.ctypes.data_as(i16p)


def _u8(a):
    return a.ctypes.data_as(u8p)


def _ptr_array(ptr_type, arrays):
    return (ptr_type * len(arrays))(*[a.ctypes.data_as(ptr_type) for a in arrays])


class GcAdpcmMath:
    BytesPerFrame = 8
    SamplesPerFrame = 14
    NibblesPerFrame = 16

    @staticmethod
    def NibbleCountToSampleCount(n):
        return _lib.lib().vga_gcadpcm_nibble_count_to_sample_count(int(n))

    @staticmethod
    def SampleCountToNibbleCount(n):
        return _lib.lib().vga_gcadpcm_sample_count_to_nibble_count(int(n))

    @staticmethod
    def NibbleToSample(n):
        return _lib.lib().vga_gcadpcm_nibble_to_sample(int(n))

    @staticmethod
    def SampleToNibble(n):
        return _lib.lib().vga_gcadpcm_sample_to_nibble(int(n))

    @staticmethod
    def SampleCountToByteCount(n):
        return _lib.lib().vga_gcadpcm_sample_count_to_byte_count(int(n))

    @staticmethod
    def ByteCountToSampleCount(n):
        return _lib.lib().vga_gcadpcm_byte_count_to_sample_count(int(n))


class GcAdpcmParameters:
    def __init__(self, SampleCount=-1, History1=0, History2=0, Progress=None):
        self.SampleCount = SampleCount
        self.History1 = History1
        self.History2 = History2
        self.Progress = Progress


def _as_channels(pcm, dtype):
    """Accept one 1-D array or a list / 2-D array of equal-length channels."""
    if isinstance(pcm, np.ndarray) and pcm.ndim == 1:
        return [np.ascontiguousarray(pcm, dtype=dtype)], True
    return [np.ascontiguousarray(p, dtype=dtype) for p in pcm], False


class GcAdpcmCoefficients:
    @staticmethod
    def CalculateCoefficients(source):
        """short[] -> short[16]; or a batch of equal-length channels -> [nch,16]."""
        chans, single = _as_channels(source, np.int16)
        nch = len(chans)
        n = len(chans[0]) if nch else 0
        if any(len(c) != n for c in chans):
            raise _lib.ArgumentError("channels of one batch must have equal length")
        coefs = np.zeros((nch, 16), dtype=np.int16)
        check(_lib.lib().vga_gcadpcm_calculate_coefficients_batch(_ptr_array(i16p, chans), nch, n, _i16(coefs)))
        return coefs[0] if single else coefs


class GcAdpcmEncoder:
    @staticmethod
    def Encode(pcm, coefs, config=None):
        """byte[] Encode(short[] pcm, short[] coefs, GcAdpcmParameters config = null); batched when
        pcm is a list / 2-D array (coefs then [nch,16]; History may be per-channel arrays)."""
        config = config or GcAdpcmParameters()
        chans, single = _as_channels(pcm, np.int16)
        nch = len(chans)
        n = len(chans[0]) if nch else 0
        if any(len(c) != n for c in chans):
            raise _lib.ArgumentError("channels of one batch must have equal length")
        sample_count = n if config.SampleCount == -1 else config.SampleCount
        coefs = np.ascontiguousarray(coefs, dtype=np.int16).reshape(nch, 16)
        h1 = np.ascontiguousarray(np.broadcast_to(np.asarray(config.History1, dtype=np.int16), (nch,)))
        h2 = np.ascontiguousarray(np.broadcast_to(np.asarray(config.History2, dtype=np.int16), (nch,)))
        nbytes = GcAdpcmMath.SampleCountToByteCount(max(sample_count, 0))
        outs = [np.zeros(nbytes, dtype=np.uint8) for _ in range(nch)]
        with _lib.reporting(config.Progress, -(-sample_count // 14)):   # frames per channel (GcAdpcmEncoder.cs:42)
            check(_lib.lib().vga_gcadpcm_encode_with_coefs_batch(
                _ptr_array(i16p, chans), nch, n, config.SampleCount, _i16(coefs), _i16(h1), _i16(h2),
                _ptr_array(u8p, outs)))
        return outs[0] if single else outs

    @staticmethod
    def DspEncodeFrame(pcmInOut, sampleCount, adpcmOut, coefsIn):
        """In-place single frame (GcAdpcmEncoder.cs:48-94) via the dsptool-compatible export."""
        buf = np.ascontiguousarray(pcmInOut, dtype=np.int16)
        out = np.zeros(8, dtype=np.uint8)
        co = np.ascontiguousarray(coefsIn, dtype=np.int16)
        _lib.lib().encodeFrame(_i16(buf), _u8(out), _i16(co), 1)
        pcmInOut[:] = buf
        adpcmOut[:8] = out


class GcAdpcmDecoder:
    @staticmethod
    def Decode(adpcm, coefficients, config=None):
        chans, single = _as_channels(adpcm, np.uint8)
        nch = len(chans)
        nb = len(chans[0]) if nch else 0
        if config is None:
            config = GcAdpcmParameters(SampleCount=GcAdpcmMath.ByteCountToSampleCount(nb))
        sample_count = config.SampleCount
        need = GcAdpcmMath.SampleCountToByteCount(max(sample_count, 0))
        if any(len(c) < need for c in chans):
            raise _lib.ArgumentError("adpcm shorter than SampleCount requires")   # IndexOutOfRange in C#
        coefs = np.ascontiguousarray(coefficients, dtype=np.int16).reshape(nch, 16)
        h1 = np.ascontiguousarray(np.broadcast_to(np.asarray(config.History1, dtype=np.int16), (nch,)))
        h2 = np.ascontiguousarray(np.broadcast_to(np.asarray(config.History2, dtype=np.int16), (nch,)))
        outs = [np.zeros(max(sample_count, 0), dtype=np.int16) for _ in range(nch)]
        check(_lib.lib().vga_gcadpcm_decode_batch(_ptr_array(u8p, chans), _i16(coefs), nch, sample_count,
                                                   _i16(h1), _i16(h2), _ptr_array(i16p, outs)))
        return outs[0] if single else outs

    @staticmethod
    def GetPredictorScale(adpcm, sample):
        return int(adpcm[sample // 14 * 8])


class Pcm16Format:
    """Planar PCM carrier: Channels is short[ChannelCount][SampleCount] (Pcm16Format.cs:14)."""

    def __init__(self, channels=None, sampleRate=48000):
        self.Channels = [np.ascontiguousarray(c, dtype=np.int16) for c in (channels if channels is not None else [])]
        self.SampleRate = sampleRate
        n = {len(c) for c in self.Channels}
        if len(n) > 1:
            raise _lib.ArgumentError("All channels must have the same sample count")
        self.SampleCount = n.pop() if n else 0
        self.Looping, self.LoopStart, self.LoopEnd = False, 0, 0

    @property
    def ChannelCount(self):
        return len(self.Channels)

    def WithLoop(self, loop, loopStart=None, loopEnd=None):
        """AudioFormatBaseBuilder.WithLoop (Formats/AudioFormatBaseBuilder.cs:23-58), applied in place."""
        if not loop:
            self.Looping, self.LoopStart, self.LoopEnd = False, 0, 0
            return self
        if loopStart is None and loopEnd is None:
            loopStart, loopEnd = 0, self.SampleCount
        if loopStart < 0 or loopStart > self.SampleCount:
            raise _lib.ArgumentOutOfRangeError("Loop points must be less than the number of samples and non-negative.")
        if loopEnd < 0 or loopEnd > self.SampleCount:
            raise _lib.ArgumentOutOfRangeError("Loop points must be less than the number of samples and non-negative.")
        if loopEnd < loopStart:
            raise _lib.ArgumentOutOfRangeError("The loop end must be greater than the loop start")
        self.Looping, self.LoopStart, self.LoopEnd = True, loopStart, loopEnd
        return self


class GcAdpcmContext:
    """PredScale / Hist1 / Hist2 (Codecs/GcAdpcm/GcAdpcmContext.cs)."""

    def __init__(self, predScale=0, hist1=0, hist2=0):
        self.PredScale, self.Hist1, self.Hist2 = int(predScale), int(hist1), int(hist2)


class AudioTrack:
    """Formats/AudioTrack.cs: one track of a multi-track container (BRSTM / BCSTM / BFSTM)."""

    def __init__(self, ChannelCount=0, ChannelLeft=0, ChannelRight=0, Volume=0x7f, Panning=0x40):
        self.ChannelCount, self.ChannelLeft, self.ChannelRight = ChannelCount, ChannelLeft, ChannelRight
        self.Volume, self.Panning = Volume, Panning

    def __eq__(self, other):
        return isinstance(other, AudioTrack) and vars(self) == vars(other)

    def __repr__(self):
        return "AudioTrack(%d, %d, %d, 0x%x, 0x%x)" % (self.ChannelCount, self.ChannelLeft, self.ChannelRight,
                                                      self.Volume, self.Panning)

    @staticmethod
    def GetDefaultTrackList(channelCount):       # AudioTrack.cs:69-82
        out = []
        for i in range(-(-channelCount // 2)):
            n = min(channelCount - i * 2, 2)
            out.append(AudioTrack(n, i * 2, i * 2 + 1 if n >= 2 else 0))
        return out


class GcAdpcmChannel:
    """Formats/GcAdpcm/GcAdpcmChannel.cs.  A channel made by the 3-argument constructor carries only the
    encoded audio; build_channels() (the batched GcAdpcmChannelBuilder.Build) adds what the reference derives:
    aligned audio, decoded PCM, loop context and seek table."""

    def __init__(self, adpcm, coefs, sampleCount):
        self.Adpcm, self.Coefs, self.UnalignedSampleCount = adpcm, coefs, sampleCount
        self.AlignmentNeeded = False
        self._aligned_adpcm = None
        self._aligned_count = sampleCount
        self._pcm = None
        self._seek = None
        self.SamplesPerSeekTableEntry = 0
        self.LoopContext = GcAdpcmContext()
        self.LoopContextStart = 0
        self.StartContext = GcAdpcmContext(adpcm[0] if len(adpcm) else 0, 0, 0)
        self.Gain = 0
        # the reference's private Pcm field (GcAdpcmChannel.cs:9,34,51-54): the PCM the channel's builder decoded for a
        # loop context or seek table, carried through clones, or None.  Only the HPS writer reads it (GetHist1 / GetHist2).
        self.Pcm = None

    @property
    def SampleCount(self):                       # GcAdpcmChannel.cs:11
        return self._aligned_count if self.AlignmentNeeded else self.UnalignedSampleCount

    def GetAdpcmAudio(self):                     # :63
        return self._aligned_adpcm if self.AlignmentNeeded else self.Adpcm

    def GetPcmAudio(self):                       # :57-60
        if self._pcm is None:
            self._pcm = GcAdpcmDecoder.Decode(self.GetAdpcmAudio(), self.Coefs, GcAdpcmParameters(SampleCount=self.SampleCount))
        return self._pcm

    def GetSeekTable(self):                      # :62
        return self._seek if self._seek is not None else np.zeros(0, dtype=np.int16)


def build_channels(channels, looping=False, loopStart=0, loopEnd=0, alignmentMultiple=0, samplesPerSeekTableEntry=0,
                   keepPcm=False, loopContext=True):
    """GcAdpcmChannelBuilder.Build for a batch of freshly encoded channels that share one loop
    (GcAdpcmFormat.cs:27-40) -- ONE GPU call (vga_gcadpcm_build_channels_batch).  Returns new channels.
    loopContext=False is the bare GcAdpcmAlignment constructor (no GetLoopContext)."""
    if not channels:
        return []
    n = channels[0].UnalignedSampleCount
    if any(c.UnalignedSampleCount != n for c in channels):
        raise _lib.ArgumentError("channels of one build must share the sample count")
    if not looping:
        loopStart = loopEnd = 0                  # GcAdpcmChannelBuilder.WithLoop(false) (:113-119)
    p = _lib.GcChannelParamsC(n, int(bool(looping)), loopStart, loopEnd, alignmentMultiple, samplesPerSeekTableEntry)
    L = _lib.GcChannelLayoutC()
    check(_lib.lib().vga_gcadpcm_channel_layout_for(C.byref(p), C.byref(L)))
    nch = len(channels)
    want_ctx = loopContext and L.loop_start_aligned != 0
    if not (L.alignment_needed or want_ctx or L.seek_table_entries or keepPcm):
        out = [GcAdpcmChannel(c.Adpcm, c.Coefs, n) for c in channels]           # nothing to derive
        for o, c in zip(out, channels):
            o.SamplesPerSeekTableEntry = samplesPerSeekTableEntry
            o.Pcm = c.Pcm
        return out
    src = [np.ascontiguousarray(c.Adpcm, dtype=np.uint8) for c in channels]
    coefs = np.ascontiguousarray(np.stack([c.Coefs for c in channels]), dtype=np.int16)
    nbytes = GcAdpcmMath.SampleCountToByteCount(L.sample_count_aligned)
    aligned = [np.zeros(nbytes, dtype=np.uint8) for _ in range(nch)] if L.alignment_needed else None
    pcm = [np.zeros(L.sample_count_aligned, dtype=np.int16) for _ in range(nch)]
    seek = [np.zeros(L.seek_table_entries * 2, dtype=np.int16) for _ in range(nch)] if L.seek_table_entries else None
    ctx = np.zeros((nch, 3), dtype=np.int16)
    check(_lib.lib().vga_gcadpcm_build_channels_batch(
        _ptr_array(u8p, src), _i16(coefs), nch, C.byref(p), _ptr_array(u8p, aligned) if aligned else None,
        _ptr_array(i16p, pcm), _ptr_array(i16p, seek) if seek else None, _i16(ctx) if loopContext else None))
    out = []
    for i, c in enumerate(channels):
        o = GcAdpcmChannel(c.Adpcm, c.Coefs, n)
        o.AlignmentNeeded = bool(L.alignment_needed)
        o._aligned_adpcm = aligned[i] if aligned else None
        o._aligned_count = L.sample_count_aligned
        o._pcm = pcm[i]
        o._seek = seek[i] if seek else None
        o.SamplesPerSeekTableEntry = samplesPerSeekTableEntry
        o.LoopContext = GcAdpcmContext(*ctx[i].tolist())
        o.LoopContextStart = L.loop_start_aligned
        # GcAdpcmChannel(builder): b.Pcm when the loop was aligned, else b.AlignedPcm -- the PCM decoded for the loop
        # context or seek table when the carried field was empty
        decoded = want_ctx or bool(L.seek_table_entries)
        o.Pcm = c.Pcm if L.alignment_needed or c.Pcm is not None or not decoded else pcm[i]
        out.append(o)
    return out


class GcAdpcmFormat:
    """IAudioFormat for GC-ADPCM; EncodeFromPcm16/ToPcm16 and the channel build of the constructor are each
    ONE batched GPU call (the reference's Parallel.For over channels, GcAdpcmFormat.cs:65 / :45 / :32)."""

    def __init__(self, channels=None, sampleRate=48000, looping=False, loopStart=0, loopEnd=0, alignmentMultiple=0,
                 samplesPerSeekTableEntry=0, tracks=None):
        self.SampleRate = sampleRate
        self.Looping = bool(looping)
        self.UnalignedLoopStart = loopStart if looping else 0
        self.UnalignedLoopEnd = loopEnd if looping else 0
        self.AlignmentMultiple = alignmentMultiple
        self.SamplesPerSeekTableEntry = samplesPerSeekTableEntry
        chans = list(channels) if channels is not None else []
        # GcAdpcmFormat(GcAdpcmFormatBuilder) rebuilds every channel with the format's loop (:27-40)
        self.Channels = build_channels(chans, self.Looping, self.UnalignedLoopStart, self.UnalignedLoopEnd, alignmentMultiple,
                                       samplesPerSeekTableEntry)
        # AudioFormatBase.cs:48: an empty or missing list means the default one
        self.Tracks = list(tracks) if tracks else AudioTrack.GetDefaultTrackList(len(self.Channels))

    @property
    def ChannelCount(self):
        return len(self.Channels)

    @property
    def UnalignedSampleCount(self):
        return self.Channels[0].UnalignedSampleCount if self.Channels else 0

    @property
    def _alignment_samples(self):                # GcAdpcmFormat.cs:19
        m = self.AlignmentMultiple
        s = self.UnalignedLoopStart
        return (s + m - s % m if m > 0 and s % m else s) - s

    @property
    def LoopStart(self):                         # :20
        return self.UnalignedLoopStart + self._alignment_samples

    @property
    def LoopEnd(self):                           # :21
        return self.UnalignedLoopEnd + self._alignment_samples

    @property
    def SampleCount(self):                       # :22
        return self.UnalignedSampleCount if self._alignment_samples == 0 else self.LoopEnd

    def _clone(self, **kw):
        a = dict(sampleRate=self.SampleRate, looping=self.Looping, loopStart=self.UnalignedLoopStart,
                 loopEnd=self.UnalignedLoopEnd, alignmentMultiple=self.AlignmentMultiple,
                 samplesPerSeekTableEntry=self.SamplesPerSeekTableEntry, tracks=self.Tracks)
        a.update(kw)
        base = [GcAdpcmChannel(c.Adpcm, c.Coefs, c.UnalignedSampleCount) for c in self.Channels]
        for b, c in zip(base, self.Channels):
            b.Pcm = c.Pcm                        # GetCloneBuilder: Pcm = Pcm
        return GcAdpcmFormat(base, **a)

    def WithLoop(self, loop, loopStart=None, loopEnd=None):          # AudioFormatBase.WithLoop (:61-63)
        if not loop:
            return self._clone(looping=False, loopStart=0, loopEnd=0)
        n = self.UnalignedSampleCount
        if loopStart is None and loopEnd is None:
            loopStart, loopEnd = 0, n
        if loopStart < 0 or loopStart > n or loopEnd < 0 or loopEnd > n:
            raise _lib.ArgumentOutOfRangeError("Loop points must be less than the number of samples and non-negative.")
        if loopEnd < loopStart:
            raise _lib.ArgumentOutOfRangeError("The loop end must be greater than the loop start")
        return self._clone(looping=True, loopStart=loopStart, loopEnd=loopEnd)

    def WithAlignment(self, loopStartAlignment):                     # GcAdpcmFormat.cs:124-126
        return self._clone(alignmentMultiple=loopStartAlignment)

    def WithSamplesPerSeekTableEntry(self, samplesPerEntry):
        """What the container writers do per channel (GetCloneBuilder().WithSamplesPerSeekTableEntry(n).Build(),
        e.g. the reference's own test helper, Tests/Formats/GcAdpcmFormatTests.cs:149-156), batched."""
        return self._clone(samplesPerSeekTableEntry=samplesPerEntry)

    def EncodeFromPcm16(self, pcm16, config=None):
        nch, n = pcm16.ChannelCount, pcm16.SampleCount
        if config is not None and config.Progress is not None:
            config.Progress.SetTotal(-(-n // 14) * nch)
        if config is not None and config.SampleCount != -1:
            # GcAdpcmEncoder.cs:17 honours the override; coefficients still come from the whole channel
            coefs = GcAdpcmCoefficients.CalculateCoefficients(pcm16.Channels) if nch else np.zeros((0, 16), np.int16)
            adpcm = GcAdpcmEncoder.Encode(pcm16.Channels, coefs, config) if nch else []
        else:
            coefs = np.zeros((nch, 16), dtype=np.int16)
            nbytes = GcAdpcmMath.SampleCountToByteCount(n)
            adpcm = [np.zeros(nbytes, dtype=np.uint8) for _ in range(nch)]
            h1 = config.History1 if config else 0
            h2 = config.History2 if config else 0
            with _lib.reporting(config.Progress if config is not None else None, -(-n // 14)):
                check(_lib.lib().vga_gcadpcm_encode_batch(_ptr_array(i16p, pcm16.Channels), nch, n, h1, h2, _i16(coefs),
                                                           _ptr_array(u8p, adpcm)))
        chans = [GcAdpcmChannel(adpcm[i], coefs[i].copy(), n) for i in range(nch)]
        # new GcAdpcmFormatBuilder(channels, rate).WithLoop(pcm16.Looping, LoopStart, LoopEnd).Build() (:70-73)
        return GcAdpcmFormat(chans, pcm16.SampleRate, pcm16.Looping, pcm16.LoopStart, pcm16.LoopEnd)

    def ToPcm16(self):                           # GcAdpcmFormat.cs:42-54
        if not self.Channels:
            return Pcm16Format([], self.SampleRate)
        if all(c._pcm is not None for c in self.Channels):
            pcm = [c._pcm for c in self.Channels]                    # GetPcmAudio(): already decoded by the build
        else:
            n = self.Channels[0].SampleCount
            pcm = GcAdpcmDecoder.Decode([c.GetAdpcmAudio() for c in self.Channels],
                                        np.stack([c.Coefs for c in self.Channels]), GcAdpcmParameters(SampleCount=n))
        out = Pcm16Format(pcm, self.SampleRate)
        out.Looping, out.LoopStart, out.LoopEnd = self.Looping, self.LoopStart, self.LoopEnd
        return out

    def BuildSeekTable(self, entryCount, bigEndian=True):
        """GcAdpcmFormat.BuildSeekTable (GcAdpcmFormat.cs:99-113): the channels' seek tables
        (GcAdpcmSeekTable.cs:25-38, built on the device) interleaved by 2, resized to entryCount."""
        tables = [c.GetSeekTable() for c in self.Channels]
        nch = len(tables)
        entries = max((len(t) // 2 for t in tables), default=0)
        inter = np.zeros(entries * 2 * nch, dtype=np.int16)
        for c, t in enumerate(tables):                               # ArrayExtensions.Interleave(2)
            v = inter.reshape(entries, nch, 2)
            v[:len(t) // 2, c, :] = t.reshape(-1, 2)
        out = np.zeros(entryCount * 2 * nch, dtype=np.int16)         # Array.Resize
        m = min(len(out), len(inter))
        out[:m] = inter[:m]
        return out.astype(">i2" if bigEndian else "<i2").tobytes()


def _encode_files_to_dsp(files, configs, dsp):
    """WAV set -> vga_gcadpcm_encode_device_v -> vga_gcadpcm_build_channels_device_v -> vga_dsp_write_device_v: the rows stay in
    HBM from the upload of the PCM to the download of the packed images; no launch per file"""
    import torch
    from .dsp import file_set
    L = _lib.lib()
    s = file_set(files, dsp)
    try:
        if s.files == 0:
            return []
        t, nch = s.totals, s.channels
        po = np.zeros(nch, dtype=np.int64)
        check(L.vga_gcadpcm_ragged_offsets(s.ragged, po.ctypes.data_as(C.POINTER(C.c_int64)), None))
        host = np.zeros(t.pcm_samples, dtype=np.int16)
        h1, h2, c = np.zeros(nch, np.int16), np.zeros(nch, np.int16), 0
        for f, cfg in zip(files, configs):
            for ch in f.Channels:
                host[po[c]:po[c] + f.SampleCount] = np.asarray(ch, dtype=np.int16)[:f.SampleCount]
                h1[c], h2[c] = (cfg.History1, cfg.History2) if cfg else (0, 0)
                c += 1
        dev = lambda a: torch.from_numpy(a).cuda()
        pcm, d_h1, d_h2 = dev(host), dev(h1), dev(h2)
        coefs = torch.zeros(nch * 16, dtype=torch.int16, device="cuda")
        adpcm = torch.zeros(t.adpcm_bytes, dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.vga_gcadpcm_ragged_coefs_workspace_bytes(s.ragged), t.build_workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        ctx = torch.zeros(nch * 3, dtype=torch.int16, device="cuda")
        images = torch.empty(t.image_bytes, dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(L.vga_gcadpcm_coefs_device_v(s.ragged, pcm.data_ptr(), coefs.data_ptr(), ws.data_ptr(), ws.numel(), st))
        check(L.vga_gcadpcm_encode_device_v(s.ragged, pcm.data_ptr(), coefs.data_ptr(), d_h1.data_ptr(), d_h2.data_ptr(), adpcm.data_ptr(), st))
        s.build_channels(adpcm, coefs, loop_context=ctx, workspace=ws)     # GcAdpcmChannel's loop context (DspWriter.cs:74-76)
        s.write_images(adpcm, coefs, images, loop_context=ctx)
        return s.split_images(images)
    finally:
        s.close()


def encode_files(pcm16_list, configs=None, dsp=None):
    """The reference's batch conversion (VGAudio.Cli/Batch.cs:24-25: Parallel.ForEach over files, each file
    GcAdpcmFormat.EncodeFromPcm16) as ONE ragged GPU call (vga_gcadpcm_encode_batch_v): `pcm16_list` holds one
    Pcm16Format per file, of any length and channel count; returns one GcAdpcmFormat per file, each what
    GcAdpcmFormat().EncodeFromPcm16(file) returns.  configs: None or one GcAdpcmParameters (or None) per file
    (History1 / History2; a SampleCount override takes the per-file path).
    dsp: a DspConfiguration -- the call then returns one DSP file (`bytes`) per input file, each what
    DspWriter(dsp).GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) returns, assembled on the device (vgaudio_amd.dsp.DspFileSet)."""
    files = list(pcm16_list)
    configs = list(configs) if configs is not None else [None] * len(files)
    if dsp is not None:
        if any(c is not None and c.SampleCount != -1 for c in configs):
            raise _lib.ArgumentError("encode_files(dsp=...): a SampleCount override is not supported")
        return _encode_files_to_dsp(files, configs, dsp)
    if any(c is not None and c.SampleCount != -1 for c in configs):
        return [GcAdpcmFormat().EncodeFromPcm16(f, c) for f, c in zip(files, configs)]
    chans, counts, h1, h2 = [], [], [], []
    for f, c in zip(files, configs):
        for ch in f.Channels:
            chans.append(ch)
            counts.append(f.SampleCount)
            h1.append(c.History1 if c else 0)
            h2.append(c.History2 if c else 0)
    nch = len(chans)
    counts = np.array(counts, dtype=np.int32)
    coefs = np.zeros((nch, 16), dtype=np.int16)
    adpcm = [np.zeros(GcAdpcmMath.SampleCountToByteCount(int(n)), dtype=np.uint8) for n in counts]
    h1 = np.array(h1, dtype=np.int16)
    h2 = np.array(h2, dtype=np.int16)
    if nch:
        check(_lib.lib().vga_gcadpcm_encode_batch_v(_ptr_array(i16p, chans), counts.ctypes.data_as(C.POINTER(C.c_int)), nch,
                                                     _i16(h1), _i16(h2), _i16(coefs), _ptr_array(u8p, adpcm)))
    out, at = [], 0
    for f in files:
        k = f.ChannelCount
        cs = [GcAdpcmChannel(adpcm[at + i], coefs[at + i].copy(), f.SampleCount) for i in range(k)]
        out.append(GcAdpcmFormat(cs, f.SampleRate, f.Looping, f.LoopStart, f.LoopEnd))
        at += k
    return out


def decode_files(formats):
    """ToPcm16 (GcAdpcmFormat.cs:42-54) of many files in ONE ragged GPU call (vga_gcadpcm_decode_batch_v)."""
    formats = list(formats)
    chans, coefs, counts = [], [], []
    for f in formats:
        for c in f.Channels:
            chans.append(np.ascontiguousarray(c.GetAdpcmAudio(), dtype=np.uint8))
            coefs.append(c.Coefs)
            counts.append(c.SampleCount)
    nch = len(chans)
    counts = np.array(counts, dtype=np.int32)
    pcm = [np.zeros(int(n), dtype=np.int16) for n in counts]
    if nch:
        co = np.ascontiguousarray(np.stack(coefs), dtype=np.int16)
        check(_lib.lib().vga_gcadpcm_decode_batch_v(_ptr_array(u8p, chans), _i16(co), counts.ctypes.data_as(C.POINTER(C.c_int)), nch,
                                                     None, None, _ptr_array(i16p, pcm)))
    out, at = [], 0
    for f in formats:
        k = f.ChannelCount
        p = Pcm16Format(pcm[at:at + k], f.SampleRate)
        p.Looping, p.LoopStart, p.LoopEnd = f.Looping, f.LoopStart, f.LoopEnd
        out.append(p)
        at += k
    return out


class AlignedFileSet(FileSetHandle):
    """A set of GC-ADPCM files whose loop starts may need the GcAdpcmAlignment re-encode, resident on the device
    (include/vgaudio_hip/gc_files_aligned.h has the layout): the channels of all files are the packed rows of two ragged
    batches, `ragged_in` over the files' sample counts (what the _device_v codec calls wrote) and `ragged_out` over their
    aligned sample counts; the seek tables are one packed buffer.
    `files`: one (channels, sample_rate, sample_count, looping, loop_start, loop_end[, alignment[, samples_per_seek_entry]])
    tuple or _lib.GcFileC per file.  The tensors are the caller's torch tensors on the current device; the call runs on
    torch's current stream and does not synchronise it."""
    _destroy = "vga_gc_aligned_destroy"

    def __init__(self, files=None):
        self._h = C.c_void_p()
        arr, n = self._files_array(files)
        check(_lib.lib().vga_gc_aligned_create(arr, n, C.byref(self._h)))
        self.totals = _lib.GcAlignedTotalsC()
        check(_lib.lib().vga_gc_aligned_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, so = np.zeros(max(nf, 1), np.int32), np.zeros(max(nch, 1), np.int64)
        check(_lib.lib().vga_gc_aligned_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), so.ctypes.data_as(C.POINTER(C.c_int64))))
        self.first_channel, self.seek_offsets = fc[:nf], so[:nch]
        self.files, self.channels = nf, nch
        self.ragged_in = C.c_void_p(_lib.lib().vga_gc_aligned_ragged_in(self._h))      # borrowed: live as long as this object
        self.ragged_out = C.c_void_p(_lib.lib().vga_gc_aligned_ragged_out(self._h))
        self.layouts = []                                                      # per file: vga_gcadpcm_channel_layout_for's numbers
        for f in arr[:n]:
            lay = _lib.GcChannelLayoutC()
            check(_lib.lib().vga_gcadpcm_channel_layout_for(C.byref(f.channel), C.byref(lay)))
            self.layouts.append(lay)

    @staticmethod
    def _files_array(files):
        from .dsp import _gc_file
        files = [f if isinstance(f, _lib.GcFileC) else _gc_file(*f) for f in (files or [])]
        return (_lib.GcFileC * max(len(files), 1))(*files), len(files)

    @classmethod
    def layout(cls, files):
        """(first_channel int32[files], seek_offsets int64[channels], GcAlignedTotalsC): host only, needs no GPU"""
        arr, n = cls._files_array(files)
        nch = sum(arr[i].channels for i in range(n) if arr[i].channels > 0)
        fc, so, tot = np.zeros(max(n, 1), np.int32), np.zeros(max(nch, 1), np.int64), _lib.GcAlignedTotalsC()
        check(_lib.lib().vga_gc_aligned_layout_for(arr, n, fc.ctypes.data_as(C.POINTER(C.c_int)), so.ctypes.data_as(C.POINTER(C.c_int64)),
                                                   C.byref(tot)))
        return fc[:n], so[:tot.channels], tot

    def offsets(self, which):
        """(pcm offsets, adpcm offsets) int64[channels] of `ragged_in` ("in") or `ragged_out` ("out")"""
        po, ao = np.zeros(max(self.channels, 1), np.int64), np.zeros(max(self.channels, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_gcadpcm_ragged_offsets(self.ragged_in if which == "in" else self.ragged_out, po.ctypes.data_as(i64p),
                                                    ao.ctypes.data_as(i64p)))
        return po[:self.channels], ao[:self.channels]

    def align_channels(self, adpcm, coefs, adpcm_out, pcm=None, seek=None, loop_context=None, status=None, workspace=None, stream=None):
        """vga_gcadpcm_align_channels_device_v.  adpcm: uint8[totals.adpcm_bytes], coefs: int16[channels*16], adpcm_out:
        uint8[totals.out_adpcm_bytes]; outputs that may be None: pcm int16[totals.out_pcm_samples], seek
        int16[totals.seek_shorts], loop_context int16[channels*3]; status: int32[1] or None; workspace:
        uint8[totals.workspace_bytes]"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        check(_lib.lib().vga_gcadpcm_align_channels_device_v(
            self._h, ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"), ptr(coefs, torch.int16, self.channels * 16, "coefs"),
            ptr(adpcm_out, torch.uint8, t.out_adpcm_bytes, "adpcm_out"), ptr(pcm, torch.int16, t.out_pcm_samples, "pcm"),
            ptr(seek, torch.int16, t.seek_shorts, "seek"), ptr(loop_context, torch.int16, self.channels * 3, "loop_context"),
            ptr(status, torch.int32, 1, "status"), ptr(workspace, torch.uint8, 0, "workspace"),
            workspace.numel() if workspace is not None else 0, DspFileSet._stream(stream)))


def build_files(pcm16_list, per_file_channel_params):
    """GcAdpcmFormat().EncodeFromPcm16(file)._clone(alignmentMultiple=, samplesPerSeekTableEntry=) for a list of files -- the
    coefficient search, the encode, the alignment re-encode, the seek tables and the loop contexts -- on the device and
    without a launch per file (AlignedFileSet).  `per_file_channel_params`: one (alignmentMultiple, samplesPerSeekTableEntry)
    per file.  Returns per file a dict of numpy arrays, each a list with one entry per channel: "adpcm" (the aligned
    stream), "seek" (int16[2 * entries]), "context" (int16[3]), "coefs" (int16[16]); and "sample_count" (the aligned one)."""
    import torch
    files, params = list(pcm16_list), list(per_file_channel_params)
    if len(files) != len(params):
        raise _lib.ArgumentError("build_files: one (alignmentMultiple, samplesPerSeekTableEntry) per file")
    L = _lib.lib()
    s = AlignedFileSet([(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0,
                         f.LoopEnd if f.Looping else 0, a, e) for f, (a, e) in zip(files, params)])
    try:
        if s.files == 0:
            return []
        t, nch = s.totals, s.channels
        pin, _ = s.offsets("in")
        _, aout = s.offsets("out")
        host, c = np.zeros(t.pcm_samples, dtype=np.int16), 0
        for f in files:
            for ch in f.Channels:
                host[pin[c]:pin[c] + f.SampleCount] = np.asarray(ch, dtype=np.int16)[:f.SampleCount]
                c += 1
        new = lambda n, dtype: torch.zeros(max(int(n), 16), dtype=dtype, device="cuda")
        pcm = torch.from_numpy(host).cuda()
        coefs, adpcm, out = new(nch * 16, torch.int16), new(t.adpcm_bytes, torch.uint8), new(t.out_adpcm_bytes, torch.uint8)
        seek, ctx = new(t.seek_shorts, torch.int16), new(nch * 3, torch.int16)
        ws = torch.empty(max(L.vga_gcadpcm_ragged_coefs_workspace_bytes(s.ragged_in), t.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(L.vga_gcadpcm_coefs_device_v(s.ragged_in, pcm.data_ptr(), coefs.data_ptr(), ws.data_ptr(), ws.numel(), st))
        check(L.vga_gcadpcm_encode_device_v(s.ragged_in, pcm.data_ptr(), coefs.data_ptr(), None, None, adpcm.data_ptr(), st))
        s.align_channels(adpcm, coefs, out, seek=seek, loop_context=ctx, workspace=ws)
        out, seek, ctx, coefs = out.cpu().numpy(), seek.cpu().numpy(), ctx.cpu().numpy(), coefs.cpu().numpy()      # synchronises
        result, c = [], 0
        for f, lay in zip(files, s.layouts):
            nbytes = GcAdpcmMath.SampleCountToByteCount(lay.sample_count_aligned)
            r = {"adpcm": [], "seek": [], "context": [], "coefs": [], "sample_count": lay.sample_count_aligned}
            for _ in range(f.ChannelCount):
                r["adpcm"].append(out[aout[c]:aout[c] + nbytes].copy())
                r["seek"].append(seek[s.seek_offsets[c]:s.seek_offsets[c] + 2 * lay.seek_table_entries].copy())
                r["context"].append(ctx[3 * c:3 * c + 3].copy())
                r["coefs"].append(coefs[16 * c:16 * c + 16].copy())
                c += 1
            result.append(r)
        return result
    finally:
        s.close()
