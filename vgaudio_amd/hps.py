"""HPS (HAL DSP stream) for GC-ADPCM -- the host-side mirror of VGAudio/Containers/Hps: HpsWriter.cs, HpsReader.cs and
HpsConfiguration.cs.  Size math, the block map and parsing run on the host (vga_hps_layout_for, vga_hps_block_map,
vga_hps_parse); the images are assembled and taken apart on the GPU (vga_hps_write, vga_hps_read).  There is no CPU
path."""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetBase
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


def _hps_file(channels, sample_rate, sample_count, looping=False, loop_start=0, loop_end=0):
    return _lib.HpsFileC(int(channels), int(sample_rate), int(sample_count), int(bool(looping)), int(loop_start), int(loop_end))


class HpsFileSet(FileSetBase):
    """A set of HPS files of different shapes, resident on the device (include/vgaudio_hip_files/hps_files.h has the layout):
    the channels of all files are the packed rows gcadpcm.AlignedFileSet leaves as its output, the images another packed
    buffer.  `files`: one (channels, sample_rate, sample_count, looping, loop_start, loop_end) tuple or _lib.HpsFileC per
    file, the loop the format's, before the writer aligns it.  The tensors are the caller's torch tensors on the current
    device; the calls run on torch's current stream and do not synchronise it."""
    _destroy = "vga_hps_files_destroy"

    def __init__(self, files=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            check(_lib.lib().vga_hps_files_create(arr, n, C.byref(self._h)))
            self.image_sizes = [self.file_layout(arr[i]).file_size for i in range(n)]
        self.totals = _lib.HpsFilesTotalsC()
        check(_lib.lib().vga_hps_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, io, fb = np.zeros(max(nf, 1), np.int32), np.zeros(max(nf, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_hps_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), io.ctypes.data_as(i64p), fb.ctypes.data_as(i64p)))
        self.first_channel, self.image_offsets, self.first_block = fc[:nf], io[:nf], fb[:nf]
        self.files, self.channels = nf, nch
        self.ragged = C.c_void_p(_lib.lib().vga_hps_files_ragged(self._h))       # borrowed: lives as long as this object

    @staticmethod
    def _files_array(files):
        files = [f if isinstance(f, _lib.HpsFileC) else _hps_file(*f) for f in (files or [])]
        return (_lib.HpsFileC * max(len(files), 1))(*files), len(files)

    @staticmethod
    def file_params(f):
        """the vga_hps_params of one file of a set"""
        return _lib.HpsParamsC(f.sample_rate, f.sample_count, f.looping, f.loop_start, f.loop_end)

    @classmethod
    def file_layout(cls, f):
        """vga_hps_layout_for of one file of a set"""
        L = _lib.HpsLayoutC()
        check(_lib.lib().vga_hps_layout_for(C.byref(cls.file_params(f)), f.channels, C.byref(L)))
        return L

    @classmethod
    def layout(cls, files):
        """(first_channel int32[files], image_offsets int64[files], first_block int64[files], HpsFilesTotalsC): host only,
        needs no GPU"""
        arr, n = cls._files_array(files)
        fc, io, fb = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.HpsFilesTotalsC(), C.POINTER(C.c_int64)
        check(_lib.lib().vga_hps_files_layout_for(arr, n, fc.ctypes.data_as(C.POINTER(C.c_int)), io.ctypes.data_as(i64p),
                                                  fb.ctypes.data_as(i64p), C.byref(tot)))
        return fc[:n], io[:n], fb[:n], tot

    @classmethod
    def from_infos(cls, parsed, image_offsets=None):
        """A set for reading, from the (vga_hps_info, block table) of every file (parse()); image_offsets: any byte offsets,
        or None for images packed as write() packs them"""
        parsed = list(parsed)
        n = len(parsed)
        infos = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i, _ in parsed])
        tables = (C.c_void_p * max(n, 1))(*[C.addressof(b) for _, b in parsed])
        offs = np.ascontiguousarray(image_offsets, dtype=np.int64) if image_offsets is not None else None
        h = C.c_void_p()
        check(_lib.lib().vga_hps_files_create_from_infos(infos, tables, n, offs.ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None,
                                                         C.byref(h)))
        s = cls(_handle=h)
        s._parsed = parsed                                                       # (keeps the ctypes objects alive)
        s.image_sizes = [max(max(b[k].audio_offset + b[k].size, b[k].audio_offset + b[k].size // i.channel_count * (i.channel_count - 1) + b[k].audio_bytes)
                             for k in range(i.block_count)) for i, b in parsed]
        return s

    def gc_files(self):
        """the _lib.GcFileC of every file (channel = vga_hps_layout_for(...).channel): what gcadpcm.AlignedFileSet takes"""
        arr = (_lib.GcFileC * max(self.files, 1))()
        check(_lib.lib().vga_hps_files_gc_files(self._h, arr))
        return list(arr[:self.files])

    def stats(self):
        """vga_hps_files_stats: (audio work items, block table entries, bytes of the device tables, kernels this thread's
        last _v call launched)"""
        out = (C.c_int64 * 4)()
        check(_lib.lib().vga_hps_files_stats(self._h, out))
        return tuple(out)

    def write(self, adpcm, coefs, images, gain=None, start_context=None, pcm=None, stream=None):
        """vga_hps_write_device_v.  adpcm: uint8[totals.adpcm_bytes] (the aligned rows), coefs: int16[channels*16], pcm:
        int16[totals.pcm_samples] (the aligned set's PCM output) or None; images: uint8[totals.image_bytes]"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t, n = self.totals, self.channels
        check(_lib.lib().vga_hps_write_device_v(
            self._h, ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"), ptr(coefs, torch.int16, n * 16, "coefs"),
            ptr(gain, torch.int16, n, "gain"), ptr(start_context, torch.int16, n * 3, "start_context"),
            ptr(pcm, torch.int16, t.pcm_samples, "pcm"), ptr(images, torch.uint8, t.image_bytes, "images"), stream_handle(stream)))

    def read(self, images, adpcm, coefs=None, gain=None, start_context=None, loop_context=None, stream=None):
        """vga_hps_read_device_v (a set from from_infos): images -> the rows of adpcm and the parsed per-channel arrays"""
        import torch
        from .dsp import device_ptr as ptr, stream_handle
        t, n = self.totals, self.channels
        check(_lib.lib().vga_hps_read_device_v(
            self._h, ptr(images, torch.uint8, t.image_bytes, "images"), ptr(adpcm, torch.uint8, t.adpcm_bytes, "adpcm"),
            ptr(coefs, torch.int16, n * 16, "coefs"), ptr(gain, torch.int16, n, "gain"),
            ptr(start_context, torch.int16, n * 3, "start_context"), ptr(loop_context, torch.int16, n * 3, "loop_context"),
            stream_handle(stream)))


def write_files(pcm16_list):
    """The HPS images of a list of Pcm16Format files, made on the device without a launch per file.  They are
    HpsWriter().GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) EXCEPT in the header of a block that starts in the re-encoded
    tail of a file whose loop start needed alignment: hist1 / hist2 come from the aligned set's PCM output here, where HpsWriter
    reads the Pcm field the format carried INTO the alignment (HpsWriter.HistSource) -- the same samples up to the last kept
    frame, other samples, or an IndexOutOfRangeException, behind it.  One upload, vga_gcadpcm_coefs_device_v,
    vga_gcadpcm_encode_device_v, the alignment re-encode of gcadpcm.AlignedFileSet, vga_hps_write_device_v, one download.
    Returns one `bytes` per file."""
    import torch
    from .gcadpcm import AlignedFileSet
    files = list(pcm16_list)
    L = _lib.lib()
    s = HpsFileSet([(f.ChannelCount, f.SampleRate, f.SampleCount, f.Looping, f.LoopStart if f.Looping else 0,
                     f.LoopEnd if f.Looping else 0) for f in files])
    a = None
    try:
        if s.files == 0:
            return []
        a = AlignedFileSet(s.gc_files())
        t, nch = a.totals, a.channels
        if t.out_adpcm_bytes != s.totals.adpcm_bytes or t.out_pcm_samples != s.totals.pcm_samples:
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
        pcm_out = new(t.out_pcm_samples, torch.int16)
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        ws = torch.empty(max(L.vga_gcadpcm_ragged_coefs_workspace_bytes(a.ragged_in), t.workspace_bytes, 16), dtype=torch.uint8, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(L.vga_gcadpcm_coefs_device_v(a.ragged_in, pcm.data_ptr(), coefs.data_ptr(), ws.data_ptr(), ws.numel(), st))
        check(L.vga_gcadpcm_encode_device_v(a.ragged_in, pcm.data_ptr(), coefs.data_ptr(), None, None, adpcm.data_ptr(), st))
        a.align_channels(adpcm, coefs, out, pcm=pcm_out, workspace=ws)
        # HpsWriter takes the start context from the format's channels, the ORIGINAL stream's: its first byte
        _, ain = a.offsets("in")
        start = torch.zeros(nch * 3, dtype=torch.int16, device="cuda")
        start.view(-1, 3)[:, 0] = adpcm[torch.from_numpy(np.ascontiguousarray(ain, dtype=np.int64)).cuda()].to(torch.int16)
        s.write(out, coefs, images, start_context=start, pcm=pcm_out)
        return s.images(images)
    finally:
        if a is not None:
            a.close()
        s.close()


def read_files(list_of_bytes, pcm=False):
    """HpsReader().ReadFormat(file) for a list of files: the headers and block chains are parsed on the host, all audio is
    taken out of the images in one vga_hps_read_device_v call.  Returns one GcAdpcmFormat per file; with pcm=True also what
    vga_gcadpcm_decode_device_v makes of the rows where they lie (no host round trip in between): (formats, one list of
    int16 channel arrays per file)."""
    import torch
    datas = [bytes(d) for d in list_of_bytes]
    parsed = [parse(d) for d in datas]
    s = HpsFileSet.from_infos(parsed)
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
        for f, (info, _) in enumerate(parsed):
            first = int(s.first_channel[f])
            chans = [rows[int(ao[first + c]):int(ao[first + c]) + info.adpcm_bytes].copy() for c in range(info.channel_count)]
            formats.append(HpsReader._to_format(info, chans))
            if pcm:
                pcms.append([decoded[int(po[first + c]):int(po[first + c]) + info.sample_count].copy() for c in range(info.channel_count)])
        return (formats, pcms) if pcm else formats
    finally:
        s.close()
