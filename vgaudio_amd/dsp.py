"""DSP container for GC-ADPCM -- the host-side mirror of VGAudio/Containers/Dsp/DspWriter.cs,
DspReader.cs and DspConfiguration.cs.  The file image is assembled and taken apart on the GPU (vga_dsp_write,
vga_dsp_read); only the header is parsed on the host (vga_dsp_parse).  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetHandle
from ._lib import check, i16p, u8p
from .gcadpcm import GcAdpcmChannel, GcAdpcmContext, GcAdpcmFormat, _i16, _ptr_array


class DspConfiguration:
    """Containers/Dsp/DspConfiguration.cs + Containers/Configuration.cs (TrimFile)."""

    def __init__(self, SamplesPerInterleave=0x3800, LoopPointAlignment=1, TrimFile=True, RecalculateLoopContext=True):
        self.SamplesPerInterleave = SamplesPerInterleave
        self.LoopPointAlignment = LoopPointAlignment
        self.TrimFile = TrimFile
        self.RecalculateLoopContext = RecalculateLoopContext

    @property
    def SamplesPerInterleave(self):
        return self._samples_per_interleave

    @SamplesPerInterleave.setter
    def SamplesPerInterleave(self, value):           # DspConfiguration.cs:31-45
        if value < 1:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be positive")
        if value % 14 != 0:
            raise _lib.ArgumentOutOfRangeError("Number of samples per interleave must be divisible by 14")
        self._samples_per_interleave = int(value)


class DspWriter:
    """AudioWriter<DspWriter, DspConfiguration> (Containers/AudioWriter.cs:11-44): GetFile(format, configuration)."""

    def __init__(self, configuration=None):
        self.Configuration = configuration or DspConfiguration()

    def _params(self, fmt):
        c = self.Configuration
        return _lib.DspParamsC(fmt.SampleRate, fmt.SampleCount, int(fmt.Looping), fmt.LoopStart, fmt.LoopEnd,
                               c.SamplesPerInterleave, c.LoopPointAlignment, int(bool(c.TrimFile)))

    def Layout(self, fmt):
        """The header geometry DspWriter.cs:18-36,99-100 derives (sizes only)."""
        L = _lib.DspLayoutC()
        p = self._params(fmt)
        check(_lib.lib().vga_dsp_layout_for(C.byref(p), fmt.ChannelCount, C.byref(L)))
        return L

    def GetFile(self, audio, configuration=None):
        if configuration is not None:
            self.Configuration = configuration
        if not isinstance(audio, GcAdpcmFormat):
            raise _lib.ArgumentError("DspWriter takes a GcAdpcmFormat (encode PCM with GcAdpcmFormat.EncodeFromPcm16 first)")
        fmt = audio
        nch = fmt.ChannelCount
        L = self.Layout(fmt)
        p = self._params(fmt)
        src = [np.ascontiguousarray(ch.GetAdpcmAudio(), dtype=np.uint8) for ch in fmt.Channels]
        if any(len(a) != len(src[0]) for a in src):
            raise _lib.ArgumentOutOfRangeError("Inputs must be of equal length")                 # Interleave.cs:49-50
        coefs = np.ascontiguousarray(np.stack([ch.Coefs for ch in fmt.Channels]), dtype=np.int16).reshape(nch, 16)
        gain = np.array([getattr(ch, "Gain", 0) for ch in fmt.Channels], dtype=np.int16)
        start = np.array([[ch.StartContext.PredScale, ch.StartContext.Hist1, ch.StartContext.Hist2] for ch in fmt.Channels],
                         dtype=np.int16)
        loop = np.array([[ch.LoopContext.PredScale, ch.LoopContext.Hist1, ch.LoopContext.Hist2] for ch in fmt.Channels],
                        dtype=np.int16)
        out = np.zeros(L.file_size, dtype=np.uint8)
        check(_lib.lib().vga_dsp_write(_ptr_array(u8p, src), len(src[0]), _i16(coefs), _i16(gain), _i16(start), _i16(loop),
                                       nch, C.byref(p), out.ctypes.data_as(u8p)))
        return out.tobytes()


def parse(data):
    """vga_dsp_parse: DspReader.ReadHeader plus the checks ReadData makes (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.DspInfoC()
    check(_lib.lib().vga_dsp_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


class DspReader:
    """AudioReader<DspReader, DspStructure, DspConfiguration> (Containers/Dsp/DspReader.cs): ReadFormat(bytes) ->
    GcAdpcmFormat, ReadWithConfig(bytes) -> (format, configuration), ReadMetadata(bytes) -> the parsed header
    (vga_dsp_info) without audio."""

    def ReadMetadata(self, data):
        return parse(data)

    def ReadFormat(self, data):
        return self.ReadWithConfig(data)[0]

    def ReadWithConfig(self, data):
        data = bytes(data)
        info = parse(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        adpcm = [np.zeros(info.adpcm_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
        check(_lib.lib().vga_dsp_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), _ptr_array(u8p, adpcm)))
        return self._to_format(info, adpcm), DspConfiguration()      # GetConfiguration: AudioReader's default (new TConfig())

    @staticmethod
    def _to_format(info, adpcm):
        """ToAudioStream (:33-55): the stored coefficients, gain, start and loop contexts; nothing is recomputed."""
        from .nwstm import _stored_format
        looping = bool(info.looping)
        chans = []
        for c in range(info.channel_count):
            ch = GcAdpcmChannel(adpcm[c], np.array(info.coefs[c][:], dtype=np.int16), info.sample_count)
            ch.Gain = int(info.gain[c])
            ch.StartContext = GcAdpcmContext(*info.start_context[c][:])
            if looping:                                          # WithLoop(..).WithLoopContext(LoopStart, ..)
                ch.LoopContext = GcAdpcmContext(*info.loop_context[c][:])
                ch.LoopContextStart = info.loop_start
            chans.append(ch)
        return _stored_format(chans, info.sample_rate, looping, info.loop_start, info.loop_end, None)


def _gc_file(channels, sample_rate, sample_count, looping=False, loop_start=0, loop_end=0, alignment=0, samples_per_entry=0):
    if not looping:
        loop_start = loop_end = 0                                # GcAdpcmChannelBuilder.WithLoop(false) (:113-119)
    return _lib.GcFileC(int(channels), int(sample_rate),
                        _lib.GcChannelParamsC(int(sample_count), int(bool(looping)), int(loop_start), int(loop_end), int(alignment),
                                              int(samples_per_entry)))


def stream_handle(stream):
    """the hipStream_t of a torch stream, or of torch's current stream: what every file set's device calls take"""
    import torch
    return C.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


def device_ptr(t, dtype, count, what):
    """the address of a file set's buffer: None, or a contiguous device tensor of `dtype` with at least `count` elements"""
    import torch
    if t is None:
        return None
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() >= count):
        raise _lib.ArgumentError("%s: a contiguous %s tensor on the device of at least %d elements" % (what, dtype, count))
    return t.data_ptr()


class DspFileSet(FileSetHandle):
    """A set of GC-ADPCM files of different shapes, resident on the device (include/vgaudio_hip/gc_files.h has the layout): the
    channels of all files are the packed rows of one ragged batch, the seek tables one packed buffer, the DSP images another.
    `files`: one (channels, sample_rate, sample_count, looping, loop_start, loop_end[, alignment[, samples_per_seek_entry]])
    tuple or _lib.GcFileC per file; `configuration`: the DspConfiguration of the whole set (as VGAudio.Cli/Batch.cs applies
    one to every file), or None for a set without images.  The tensors are the caller's torch tensors on the current device;
    the calls run on torch's current stream and do not synchronise it."""
    _destroy = "vga_gc_files_destroy"

    def __init__(self, files=None, configuration=None, _handle=None):
        self._h, sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            cfg = self._config(configuration)
            check(_lib.lib().vga_gc_files_create(arr, n, C.byref(cfg) if cfg is not None else None, C.byref(self._h)))
            sizes = self._image_sizes(arr, n, cfg)
        self.totals = _lib.GcFilesTotalsC()
        check(_lib.lib().vga_gc_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, so, io = np.zeros(max(nf, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_gc_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), so.ctypes.data_as(i64p), io.ctypes.data_as(i64p)))
        self.first_channel, self.seek_offsets, self.image_offsets = fc[:nf], so[:nch], io[:nf]
        self.files, self.channels = nf, nch
        self.ragged = C.c_void_p(_lib.lib().vga_gc_files_ragged(self._h))      # borrowed: lives as long as this object
        self.image_sizes = sizes                                               # bytes of every file's image (None without a configuration)

    @staticmethod
    def _files_array(files):
        files = [f if isinstance(f, _lib.GcFileC) else _gc_file(*f) for f in (files or [])]
        return (_lib.GcFileC * max(len(files), 1))(*files), len(files)

    @staticmethod
    def _config(configuration):
        if configuration is None or isinstance(configuration, _lib.DspFileConfigC):
            return configuration
        c = configuration
        return _lib.DspFileConfigC(c.SamplesPerInterleave, c.LoopPointAlignment, int(bool(c.TrimFile)))

    @staticmethod
    def _image_sizes(arr, n, cfg):
        if cfg is None:
            return None
        sizes = []
        for f in arr[:n]:
            p = _lib.DspParamsC(f.sample_rate, f.channel.sample_count, f.channel.looping, f.channel.loop_start, f.channel.loop_end,
                                cfg.samples_per_interleave, cfg.loop_point_alignment, cfg.trim_file)
            L = _lib.DspLayoutC()
            check(_lib.lib().vga_dsp_layout_for(C.byref(p), f.channels, C.byref(L)))
            sizes.append(L.file_size)
        return sizes

    @classmethod
    def layout(cls, files, configuration=None):
        """(first_channel int32[files], seek_offsets int64[channels], image_offsets int64[files], GcFilesTotalsC): host only,
        needs no GPU"""
        arr, n = cls._files_array(files)
        cfg = cls._config(configuration)
        nch = sum(arr[i].channels for i in range(n) if arr[i].channels > 0)
        fc, so, io = np.zeros(max(n, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.GcFilesTotalsC(), C.POINTER(C.c_int64)
        check(_lib.lib().vga_gc_files_layout_for(arr, n, C.byref(cfg) if cfg is not None else None, fc.ctypes.data_as(C.POINTER(C.c_int)),
                                                 so.ctypes.data_as(i64p), io.ctypes.data_as(i64p), C.byref(tot)))
        return fc[:n], so[:tot.channels], io[:n], tot

    @classmethod
    def from_infos(cls, infos, image_offsets=None):
        """A set for reading, from the vga_dsp_info of every file (parse()); image_offsets: multiples of 8, or None for images
        packed as write_images packs them"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i in infos])
        offs = None
        if image_offsets is not None:
            offs = np.ascontiguousarray(image_offsets, dtype=np.int64)
        h = C.c_void_p()
        check(_lib.lib().vga_gc_files_create_from_dsp(ptrs, n, offs.ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None, C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [i.audio_offset + i.data_length for i in infos]
        return s

    _stream = staticmethod(lambda stream: stream_handle(stream))
    _ptr = staticmethod(lambda t, dtype, count, what: device_ptr(t, dtype, count, what))

    def build_channels(self, adpcm, coefs, pcm=None, seek=None, loop_context=None, status=None, workspace=None, stream=None):
        """vga_gcadpcm_build_channels_device_v.  adpcm: uint8[totals.adpcm_bytes], coefs: int16[channels*16]; outputs (each may be
        None): pcm int16[totals.pcm_samples], seek int16[totals.seek_shorts], loop_context int16[channels*3]; status: int32[1]
        or None; workspace: uint8[totals.build_workspace_bytes] when pcm is None"""
        import torch
        t = self.totals
        check(_lib.lib().vga_gcadpcm_build_channels_device_v(
            self._h, self._ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"), self._ptr(coefs, torch.int16, self.channels * 16, "coefs"),
            self._ptr(pcm, torch.int16, t.pcm_samples, "pcm"), self._ptr(seek, torch.int16, t.seek_shorts, "seek"),
            self._ptr(loop_context, torch.int16, self.channels * 3, "loop_context"), self._ptr(status, torch.int32, 1, "status"),
            self._ptr(workspace, torch.uint8, 0, "workspace"), workspace.numel() if workspace is not None else 0, self._stream(stream)))

    def write_images(self, adpcm, coefs, images, gain=None, start_context=None, loop_context=None, stream=None):
        """vga_dsp_write_device_v: images uint8[totals.image_bytes]"""
        import torch
        t, n = self.totals, self.channels
        check(_lib.lib().vga_dsp_write_device_v(
            self._h, self._ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"), self._ptr(coefs, torch.int16, n * 16, "coefs"),
            self._ptr(gain, torch.int16, n, "gain"), self._ptr(start_context, torch.int16, n * 3, "start_context"),
            self._ptr(loop_context, torch.int16, n * 3, "loop_context"), self._ptr(images, torch.uint8, t.image_bytes, "images"),
            self._stream(stream)))

    def read_images(self, images, adpcm, coefs=None, gain=None, start_context=None, loop_context=None, stream=None):
        """vga_dsp_read_device_v (a set from from_infos): images -> the rows of adpcm and the per-channel header fields"""
        import torch
        t, n = self.totals, self.channels
        check(_lib.lib().vga_dsp_read_device_v(
            self._h, self._ptr(images, torch.uint8, t.image_bytes, "images"), self._ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"),
            self._ptr(coefs, torch.int16, n * 16, "coefs"), self._ptr(gain, torch.int16, n, "gain"),
            self._ptr(start_context, torch.int16, n * 3, "start_context"), self._ptr(loop_context, torch.int16, n * 3, "loop_context"),
            self._stream(stream)))

    def split_images(self, images):
        """one `bytes` per file from the packed images (a device tensor or a numpy array); synchronises"""
        if self.image_sizes is None:
            raise _lib.InvalidOperationError("the set was made without a DspConfiguration: it has no images")
        host = images.cpu().numpy() if hasattr(images, "cpu") else np.asarray(images, dtype=np.uint8)
        return [host[int(at):int(at) + int(size)].tobytes() for at, size in zip(self.image_offsets, self.image_sizes)]


def file_set(formats, configuration=None, samples_per_seek_entry=0):
    """The DspFileSet of a list of GcAdpcmFormat / Pcm16Format files: their shapes and loops"""
    return DspFileSet([_gc_file(f.ChannelCount, f.SampleRate, getattr(f, "UnalignedSampleCount", f.SampleCount), f.Looping,
                                f.LoopStart if f.Looping else 0, f.LoopEnd if f.Looping else 0, 0, samples_per_seek_entry)
                       for f in formats], configuration)
