"""WAVE reader/writer for 16-bit and 8-bit PCM -- host-side mirror of
VGAudio/Containers/Wave/WaveReader.cs and WaveWriter.cs.  The RIFF header is parsed on the host
(vga_wave_parse); the interleaved <-> planar transposes run on the GPU.  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetHandle, fetch_items, i64_or_none as _i64_or_none
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


# ---------------------------------------------------------------- sets of files (include/vgaudio_hip_files/wave_files.h)
def _wave_file(f):
    """a _lib.WaveFileC from one, or from (channels, bits, _lib.WaveParamsC)"""
    return f if isinstance(f, _lib.WaveFileC) else _lib.WaveFileC(f[0], f[1], f[2])


class WaveFileSet(FileSetHandle):
    """A set of WAVE files of different shapes, resident on the device (include/vgaudio_hip_files/wave_files.h has the layout):
    the channels of all files are packed int16 rows of ONE buffer -- as criadx.RaggedAdx, crihca.RaggedHca and the GC ragged
    objects take their input, or at the caller's `pcm_offsets` (samples) --, the images one buffer, packed or at the caller's
    `image_offsets` (any byte).  `files`: one _lib.WaveFileC or (channels, bits, _lib.WaveParamsC) per file.  The tensors are
    the caller's torch tensors on the current device; the calls run on torch's current stream and do not synchronise it."""
    _destroy = "vga_wave_files_destroy"

    def __init__(self, files=None, pcm_offsets=None, image_offsets=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            keep_p, po = _i64_or_none(pcm_offsets)
            keep_i, io = _i64_or_none(image_offsets)
            check(_lib.lib().vga_wave_files_create(arr, n, po, io, C.byref(self._h)))
            self.image_sizes = [self.file_size(arr[i]) for i in range(n)]
        self.totals = _lib.WaveFilesTotalsC()
        check(_lib.lib().vga_wave_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, po, io = np.zeros(max(nf, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_wave_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), po.ctypes.data_as(i64p), io.ctypes.data_as(i64p)))
        self.first_channel, self.pcm_offsets, self.image_offsets = fc[:nf], po[:nch], io[:nf]
        self.files, self.channels = nf, nch

    @staticmethod
    def _files_array(files):
        files = [_wave_file(f) for f in (files or [])]
        return (_lib.WaveFileC * max(len(files), 1))(*files), len(files)

    @staticmethod
    def file_size(f):
        """vga_wave_file_size / vga_wave_pcm8_file_size of one file of a set"""
        call = _lib.lib().vga_wave_file_size if f.bits == 16 else _lib.lib().vga_wave_pcm8_file_size
        size = call(C.byref(f.params), f.channels)
        if size < 0:
            check(int(size))
        return int(size)

    @classmethod
    def layout(cls, files, pcm_offsets=None, image_offsets=None):
        """(first_channel int32[files], pcm_offsets int64[channels], image_offsets int64[files], WaveFilesTotalsC): host only,
        needs no GPU"""
        arr, n = cls._files_array(files)
        nch = sum(arr[i].channels for i in range(n) if arr[i].channels > 0)
        fc, po, io = np.zeros(max(n, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.WaveFilesTotalsC(), C.POINTER(C.c_int64)
        keep_p, pin = _i64_or_none(pcm_offsets)
        keep_i, iin = _i64_or_none(image_offsets)
        check(_lib.lib().vga_wave_files_layout_for(arr, n, pin, iin, fc.ctypes.data_as(C.POINTER(C.c_int)), po.ctypes.data_as(i64p),
                                                   io.ctypes.data_as(i64p), C.byref(tot)))
        return fc[:n], po[:tot.channels], io[:n], tot

    @classmethod
    def from_infos(cls, infos, pcm_offsets=None, image_offsets=None):
        """A set for reading, from the vga_wave_info of every file (WaveReader.ReadMetadata); image_offsets: any byte offsets,
        or None for images packed as a set for writing packs them"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i in infos])
        keep_p, po = _i64_or_none(pcm_offsets)
        keep_i, io = _i64_or_none(image_offsets)
        h = C.c_void_p()
        check(_lib.lib().vga_wave_files_create_from_infos(ptrs, n, po, io, C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [int(i.data_offset) + i.data_size for i in infos]
        return s

    @staticmethod
    def _items(call, first, n, pcm_offsets, image_offsets, general):
        keep_p, po = _i64_or_none(pcm_offsets)
        keep_i, io = _i64_or_none(image_offsets)
        return fetch_items(call, (first, n, po, io, int(general)), _lib.WaveFilesItemC)

    @classmethod
    def write_items(cls, files, pcm_offsets=None, image_offsets=None, general=False):
        """the work items of vga_wave_write_device_v on such a set (_lib.WaveFilesItemC), host only"""
        arr, n = cls._files_array(files)
        return cls._items(_lib.lib().vga_wave_files_write_items_for, arr, n, pcm_offsets, image_offsets, general)

    @classmethod
    def read_items(cls, infos, pcm_offsets=None, image_offsets=None, general=False):
        """the work items of vga_wave_read_device_v on a set of such infos, host only"""
        infos = list(infos)
        ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos])
        return cls._items(_lib.lib().vga_wave_files_read_items_for, ptrs, len(infos), pcm_offsets, image_offsets, general)

    def stats(self):
        """(tile files, general files, tile items, general items) of a call made by this thread now"""
        out = (C.c_int64 * 4)()
        check(_lib.lib().vga_wave_files_stats(self._h, out))
        return tuple(out)

    def read_device(self, images, pcm, stream=None):
        """vga_wave_read_device_v (a set from from_infos).  images: uint8[totals.image_bytes]; pcm: int16[totals.pcm_samples]"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t = self.totals
        check(_lib.lib().vga_wave_read_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"),
                                                ptr(pcm, torch.int16, t.pcm_samples, "pcm"), stream_handle(stream)))

    def write_device(self, pcm, images, stream=None):
        """vga_wave_write_device_v.  pcm: int16[totals.pcm_samples] (the rows); images: uint8[totals.image_bytes]"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t = self.totals
        check(_lib.lib().vga_wave_write_device_v(self._h, ptr(pcm, torch.int16, t.pcm_samples, "pcm"),
                                                 ptr(images, torch.uint8, t.image_bytes, "images"), stream_handle(stream)))

    def images(self, host_buffer):
        """one `bytes` per file from the images' buffer (a device tensor or a numpy array); synchronises"""
        host = host_buffer.cpu().numpy() if hasattr(host_buffer, "cpu") else np.asarray(host_buffer, dtype=np.uint8)
        return [host[int(at):int(at) + int(size)].tobytes() for at, size in zip(self.image_offsets, self.image_sizes)]


def read_files_device(list_of_bytes, pcm_offsets=None):
    """The data chunks of a list of WAVE files (16-bit, or 8-bit through Pcm8Codec.Decode) as packed int16 rows on the device,
    in ONE vga_wave_read_device_v call: (pcm tensor int16[totals.pcm_samples], pcm_offsets int64[rows], infos).  The rows of
    file f are the next infos[f].channel_count ones, infos[f].sample_count samples each; with pcm_offsets None they lie as
    criadx.RaggedAdx, crihca.RaggedHca and the GC ragged objects take them for the same sample counts."""
    import torch
    datas = [bytes(d) for d in list_of_bytes]
    infos = [WaveReader.ReadMetadata(d) for d in datas]
    s = WaveFileSet.from_infos(infos, pcm_offsets)
    try:
        host = np.zeros(s.totals.image_bytes, dtype=np.uint8)
        for d, at, size in zip(datas, s.image_offsets, s.image_sizes):
            host[int(at):int(at) + size] = np.frombuffer(d, dtype=np.uint8)[:size]
        pcm = torch.zeros(s.totals.pcm_samples, dtype=torch.int16, device="cuda")
        if s.files:
            s.read_device(torch.from_numpy(host).cuda(), pcm)
        return pcm, s.pcm_offsets.copy(), infos
    finally:
        s.close()


def read_files(list_of_bytes):
    """WaveReader.ReadFormat(file) for a list of files, without a launch per file: one Pcm16Format per file, loop points
    included.  An 8-bit file comes as ReadPcm8Format(file).ToPcm16() would give it (the set's rows are int16)."""
    if not list(list_of_bytes):
        return []
    pcm, offsets, infos = read_files_device(list_of_bytes)
    rows = pcm.cpu().numpy()
    out, c = [], 0
    for info in infos:
        chans = [rows[int(offsets[c + i]):int(offsets[c + i]) + info.sample_count].copy() for i in range(info.channel_count)]
        c += info.channel_count
        out.append(Pcm16Format(chans, info.sample_rate).WithLoop(bool(info.looping), info.loop_start, info.loop_end))
    return out


def write_files(pcm16_list, codec=WaveCodec.Pcm16Bit):
    """WaveWriter.GetFile(file, codec) for a list of Pcm16Format files, on the device and without a launch per file: one
    `bytes` per file, in the caller's order.  With WaveCodec.Pcm8Bit the rows go through Pcm8Codec.Encode on the device."""
    import torch
    files = list(pcm16_list)
    for i, f in enumerate(files):
        if not isinstance(f, Pcm16Format):
            raise _lib.ArgumentError("file %d: write_files takes Pcm16Format files (decode with ToPcm16 first)" % i)
    bits = 8 if codec == WaveCodec.Pcm8Bit else 16
    described = [_lib.WaveFileC(f.ChannelCount, bits, _lib.WaveParamsC(f.SampleRate, f.SampleCount, int(f.Looping), f.LoopStart, f.LoopEnd))
                 for f in files]
    _, offsets, _, totals = WaveFileSet.layout(described)             # every refusal of a file, before anything is allocated
    if not files:
        return []
    host, c = np.zeros(totals.pcm_samples, dtype=np.int16), 0
    for f in files:
        for ch in f.Channels:
            host[int(offsets[c]):int(offsets[c]) + f.SampleCount] = np.asarray(ch, dtype=np.int16)[:f.SampleCount]
            c += 1
    s = WaveFileSet(described)
    try:
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        s.write_device(torch.from_numpy(host).cuda(), images)
        return s.images(images)
    finally:
        s.close()
