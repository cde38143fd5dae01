"""IDSP for GC-ADPCM -- the host-side mirror of VGAudio/Containers/Idsp: IdspWriter.cs, IdspReader.cs and
IdspConfiguration.cs.  Size math and parsing run on the host (vga_idsp_layout_for, vga_idsp_parse); the images are
assembled and taken apart on the GPU (vga_idsp_write, vga_idsp_read).  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetBase
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


def _idsp_file(channels, sample_rate, sample_count, looping=False, loop_start=0, loop_end=0):
    return _lib.IdspFileC(int(channels), int(sample_rate), int(sample_count), int(bool(looping)), int(loop_start), int(loop_end))


def _file_config(configuration=None):
    c = configuration or IdspConfiguration()
    if isinstance(c, _lib.IdspFileConfigC):
        return c
    return _lib.IdspFileConfigC(int(c.BlockSize), int(bool(c.TrimFile)))


class IdspFileSet(FileSetBase):
    """A set of IDSP files of different shapes, resident on the device (include/vgaudio_hip_files/idsp_files.h has the layout):
    the channels of all files are the packed rows gcadpcm.AlignedFileSet leaves as its output, the images another packed
    buffer.  `files`: one (channels, sample_rate, sample_count, looping, loop_start, loop_end) tuple or _lib.IdspFileC per
    file, the loop the format's, before the writer aligns it; `configuration`: the IdspConfiguration of the whole set (as
    VGAudio.Cli/Batch.cs applies one to every file).  The tensors are the caller's torch tensors on the current device; the
    calls run on torch's current stream and do not synchronise it."""
    _destroy = "vga_idsp_files_destroy"

    def __init__(self, files=None, configuration=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            cfg = _file_config(configuration)
            check(_lib.lib().vga_idsp_files_create(arr, n, C.byref(cfg), C.byref(self._h)))
            self.image_sizes = [self.file_layout(arr[i], cfg).file_size for i in range(n)]
        self.totals = _lib.IdspFilesTotalsC()
        check(_lib.lib().vga_idsp_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, io = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int64)
        check(_lib.lib().vga_idsp_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), io.ctypes.data_as(C.POINTER(C.c_int64))))
        self.first_channel, self.image_offsets = fc[:nf], io[:nf]
        self.files, self.channels = nf, nch
        self.ragged = C.c_void_p(_lib.lib().vga_idsp_files_ragged(self._h))      # borrowed: lives as long as this object

    @staticmethod
    def _files_array(files):
        files = [f if isinstance(f, _lib.IdspFileC) else _idsp_file(*f) for f in (files or [])]
        return (_lib.IdspFileC * max(len(files), 1))(*files), len(files)

    @staticmethod
    def file_params(f, cfg):
        """the vga_idsp_params of one file of a set: the configuration plus the file's numbers"""
        return _lib.IdspParamsC(f.sample_rate, f.sample_count, f.looping, f.loop_start, f.loop_end, cfg.block_size, cfg.trim_file)

    @classmethod
    def file_layout(cls, f, cfg):
        """vga_idsp_layout_for of one file of a set"""
        L = _lib.IdspLayoutC()
        check(_lib.lib().vga_idsp_layout_for(C.byref(cls.file_params(f, cfg)), f.channels, C.byref(L)))
        return L

    @classmethod
    def layout(cls, files, configuration=None):
        """(first_channel int32[files], image_offsets int64[files], IdspFilesTotalsC): host only, needs no GPU"""
        arr, n = cls._files_array(files)
        cfg = _file_config(configuration)
        fc, io, tot = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), _lib.IdspFilesTotalsC()
        check(_lib.lib().vga_idsp_files_layout_for(arr, n, C.byref(cfg), fc.ctypes.data_as(C.POINTER(C.c_int)),
                                                   io.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(tot)))
        return fc[:n], io[:n], tot

    @classmethod
    def from_infos(cls, infos, image_offsets=None):
        """A set for reading, from the vga_idsp_info of every file (parse()); image_offsets: any byte offsets, or None for
        images packed as write() packs them"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i in infos])
        offs = np.ascontiguousarray(image_offsets, dtype=np.int64) if image_offsets is not None else None
        h = C.c_void_p()
        check(_lib.lib().vga_idsp_files_create_from_infos(ptrs, n, offs.ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None,
                                                          C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [i.audio_data_offset + i.channel_count * i.audio_data_length for i in infos]
        return s

    def gc_files(self):
        """the _lib.GcFileC of every file (channel = vga_idsp_layout_for(...).channel): what gcadpcm.AlignedFileSet takes"""
        arr = (_lib.GcFileC * max(self.files, 1))()
        check(_lib.lib().vga_idsp_files_gc_files(self._h, arr))
        return list(arr[:self.files])

    def stats(self):
        """vga_idsp_files_stats: (audio work items, those of 16-byte granules, bytes of the device tables, kernels this
        thread's last _v call launched)"""
        out = (C.c_int64 * 4)()
        check(_lib.lib().vga_idsp_files_stats(self._h, out))
        return tuple(out)

    def write(self, adpcm, coefs, images, gain=None, start_context=None, loop_context=None, stream=None):
        """vga_idsp_write_device_v.  adpcm: uint8[totals.adpcm_bytes] (the aligned rows), coefs: int16[channels*16]; images:
        uint8[totals.image_bytes]"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t, n = self.totals, self.channels
        check(_lib.lib().vga_idsp_write_device_v(
            self._h, ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"), ptr(coefs, torch.int16, n * 16, "coefs"),
            ptr(gain, torch.int16, n, "gain"), ptr(start_context, torch.int16, n * 3, "start_context"),
            ptr(loop_context, torch.int16, n * 3, "loop_context"), ptr(images, torch.uint8, t.image_bytes, "images"),
            stream_handle(stream)))

    def read(self, images, adpcm, coefs=None, gain=None, start_context=None, loop_context=None, stream=None):
        """vga_idsp_read_device_v (a set from from_infos): images -> the rows of adpcm and the parsed per-channel arrays"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t, n = self.totals, self.channels
        check(_lib.lib().vga_idsp_read_device_v(
            self._h, ptr(images, torch.uint8, t.image_bytes, "images"), ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"),
            ptr(coefs, torch.int16, n * 16, "coefs"), ptr(gain, torch.int16, n, "gain"),
            ptr(start_context, torch.int16, n * 3, "start_context"), ptr(loop_context, torch.int16, n * 3, "loop_context"),
            stream_handle(stream)))


def write_files(pcm16_list, configuration=None):
    """IdspWriter(configuration).GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) for a list of Pcm16Format files on the device and
    without a launch per file: one upload, vga_gcadpcm_coefs_device_v, vga_gcadpcm_encode_device_v, the alignment re-encode of
    gcadpcm.AlignedFileSet, vga_idsp_write_device_v, one download.  Returns one `bytes` per file."""
    import torch
    from .gcadpcm import AlignedFileSet
    files = list(pcm16_list)
    L = _lib.lib()
    s = IdspFileSet([(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0,
                      f.LoopEnd if f.Looping else 0) for f in files], configuration)
    a = None
    try:
        if s.files == 0:
            return []
        a = AlignedFileSet(s.gc_files())
        t, nch = a.totals, a.channels
        if t.out_adpcm_bytes != s.totals.adpcm_bytes:
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
        ctx = new(nch * 3, torch.int16)
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.vga_gcadpcm_ragged_coefs_workspace_bytes(a.ragged_in), t.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(L.vga_gcadpcm_coefs_device_v(a.ragged_in, pcm.data_ptr(), coefs.data_ptr(), ws.data_ptr(), ws.numel(), st))
        check(L.vga_gcadpcm_encode_device_v(a.ragged_in, pcm.data_ptr(), coefs.data_ptr(), None, None, adpcm.data_ptr(), st))
        a.align_channels(adpcm, coefs, out, loop_context=ctx, workspace=ws)
        # IdspWriter takes the start context from the format's channels, the ORIGINAL stream's: its first byte (a row that
        # needs no alignment keeps its bytes, so only the re-encoded ones could differ)
        _, ain = a.offsets("in")
        start = torch.zeros(nch * 3, dtype=torch.int16, device="cuda")
        start.view(-1, 3)[:, 0] = adpcm[torch.from_numpy(np.ascontiguousarray(ain, dtype=np.int64)).cuda()].to(torch.int16)
        has_bytes = np.repeat([f.SampleCount > 0 for f in files], [f.ChannelCount for f in files])
        start.view(-1, 3)[:, 0] *= torch.from_numpy(has_bytes.astype(np.int16)).cuda()        # a row of no bytes: 0
        s.write(out, coefs, images, start_context=start, loop_context=ctx)
        return s.images(images)
    finally:
        if a is not None:
            a.close()
        s.close()


def read_files(list_of_bytes, pcm=False):
    """IdspReader().ReadFormat(file) for a list of files: the headers are parsed on the host, all audio is taken out of the
    images in one vga_idsp_read_device_v call.  Returns one GcAdpcmFormat per file; with pcm=True also what
    vga_gcadpcm_decode_device_v makes of the rows where they lie (no host round trip in between): (formats, one list of
    int16 channel arrays per file)."""
    import torch
    datas = [bytes(d) for d in list_of_bytes]
    infos = [parse(d) for d in datas]
    s = IdspFileSet.from_infos(infos)
    try:
        if s.files == 0:
            return ([], []) if pcm else []
        L = _lib.lib()
        host = np.zeros(s.totals.image_bytes, dtype=np.uint8)
        for d, at, size in zip(datas, s.image_offsets, s.image_sizes):
            host[int(at):int(at) + size] = np.frombuffer(d, dtype=np.uint8)[:size]
        images = torch.from_numpy(host).cuda()
        adpcm = torch.zeros(s.totals.adpcm_bytes, dtype=torch.uint8, device="cuda")
        coefs = torch.zeros(max(s.channels * 16, 16), dtype=torch.int16, device="cuda")
        start = torch.zeros(max(s.channels * 3, 16), dtype=torch.int16, device="cuda")
        s.read(images, adpcm, coefs=coefs, start_context=start)
        po, ao = np.zeros(s.channels, np.int64), np.zeros(s.channels, np.int64)
        check(L.vga_gcadpcm_ragged_offsets(s.ragged, po.ctypes.data_as(C.POINTER(C.c_int64)), ao.ctypes.data_as(C.POINTER(C.c_int64))))
        decoded = None
        if pcm:
            out = torch.zeros(s.totals.pcm_samples, dtype=torch.int16, device="cuda")
            status = torch.zeros(4, dtype=torch.int32, device="cuda")
            ctx = start[:s.channels * 3].view(-1, 3)
            h1, h2 = ctx[:, 1].contiguous(), ctx[:, 2].contiguous()
            check(L.vga_gcadpcm_decode_device_v(s.ragged, adpcm.data_ptr(), coefs.data_ptr(), h1.data_ptr(), h2.data_ptr(), out.data_ptr(),
                                                status.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            decoded = out.cpu().numpy()
        rows = adpcm.cpu().numpy()
        formats, pcms = [], []
        for f, info in enumerate(infos):
            first = int(s.first_channel[f])
            chans = [rows[int(ao[first + c]):int(ao[first + c]) + info.adpcm_bytes].copy() for c in range(info.channel_count)]
            formats.append(IdspReader._to_format(info, chans))
            if pcm:
                pcms.append([decoded[int(po[first + c]):int(po[first + c]) + info.sample_count].copy() for c in range(info.channel_count)])
        return (formats, pcms) if pcm else formats
    finally:
        s.close()
