"""ADX container -- host-side mirror of VGAudio/Containers/Adx/AdxWriter.cs, AdxReader.cs and
AdxConfiguration.cs.  The image is assembled and taken apart on the GPU (vga_adx_write, vga_adx_read), encryption
included (vga_adx_crypt, vga_adx_find_key_device); only the header is parsed on the host.  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetBase, fetch_items, i64_or_none as _i64_or_none
from ._lib import check, u8p
from .criadx import CriAdxChannel, CriAdxEncryption, CriAdxFormat, CriAdxParameters, CriAdxType
from .gcadpcm import Pcm16Format, _i16, _ptr_array


class AdxConfiguration:
    """Containers/Adx/AdxConfiguration.cs:5-13 + Configuration.TrimFile."""

    def __init__(self, Version=4, EncryptionType=0, EncryptionKey=None, FrameSize=18, Filter=2, Type=CriAdxType.Linear,
                 TrimFile=True, Progress=None):
        self.Version, self.EncryptionType, self.EncryptionKey = Version, EncryptionType, EncryptionKey
        self.FrameSize, self.Filter, self.Type, self.TrimFile, self.Progress = FrameSize, Filter, Type, TrimFile, Progress


class AdxWriter:
    """AudioWriter<AdxWriter, AdxConfiguration>: GetFile(audio, configuration)."""

    def __init__(self, configuration=None):
        self.Configuration = configuration or AdxConfiguration()

    def _setup(self, audio):                                 # SetupWriter (:39-56)
        cfg = self.Configuration
        if isinstance(audio, Pcm16Format):                   # AudioData.GetFormat<CriAdxFormat>(encodingConfig)
            audio = CriAdxFormat().EncodeFromPcm16(audio, CriAdxParameters(
                Progress=cfg.Progress, Version=cfg.Version, FrameSize=cfg.FrameSize, Filter=cfg.Filter, Type=cfg.Type))
        if not isinstance(audio, CriAdxFormat):
            raise _lib.ArgumentError("AdxWriter takes a CriAdxFormat or a Pcm16Format")
        return audio

    def _params(self, fmt):
        cfg = self.Configuration
        return _lib.AdxFileParamsC(fmt.SampleRate, fmt.SampleCount, int(fmt.Looping), fmt.LoopStart, fmt.LoopEnd,
                                   fmt.AlignmentSamples, fmt.FrameSize, fmt.Version, fmt.Type, fmt.HighpassFrequency,
                                   cfg.EncryptionType, int(bool(cfg.TrimFile)))

    def Layout(self, fmt):
        L = _lib.AdxFileLayoutC()
        p = self._params(fmt)
        check(_lib.lib().vga_adx_file_layout_for(C.byref(p), fmt.ChannelCount, C.byref(L)))
        return L

    def GetFile(self, audio, configuration=None):
        if configuration is not None:
            self.Configuration = configuration
        fmt = self._setup(audio)
        L = self.Layout(fmt)
        p = self._params(fmt)
        src = [np.ascontiguousarray(ch.Audio, dtype=np.uint8) for ch in fmt.Channels]
        cfg = self.Configuration
        if cfg.EncryptionKey is not None:                    # WriteData (:123-128): encrypt copies, not the format's audio
            src = [a.copy() for a in src]
            CriAdxEncryption.EncryptDecrypt(src, cfg.EncryptionKey, cfg.EncryptionType, fmt.FrameSize)
        if any(len(a) != len(src[0]) for a in src):
            raise _lib.ArgumentOutOfRangeError("Inputs must be of equal length")            # Interleave.cs:49-50
        hist = np.array([ch.History for ch in fmt.Channels], dtype=np.int16)
        out = np.zeros(L.file_size, dtype=np.uint8)
        check(_lib.lib().vga_adx_write(_ptr_array(u8p, src), len(src[0]), _i16(hist), fmt.ChannelCount, C.byref(p),
                                       out.ctypes.data_as(u8p)))
        return out.tobytes()


def parse(data):
    """vga_adx_parse: AdxReader.ReadHeader plus the checks ReadData makes (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.AdxFileInfoC()
    check(_lib.lib().vga_adx_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


class AdxReader:
    """AudioReader<AdxReader, AdxStructure, AdxConfiguration> (Containers/Adx/AdxReader.cs).  EncryptionKey: a CriAdxKey
    or None; Keys: the candidates FindKey tries when the file is encrypted and no key is given (the reference's list,
    CriAdxEncryptionKeys.cs, stays with the caller).  No key found: the audio stays encrypted, as in the reference."""

    def __init__(self, EncryptionKey=None, Keys=None):
        self.EncryptionKey = EncryptionKey
        self.Keys = list(Keys) if Keys else []

    def ReadMetadata(self, data):
        return parse(data)

    def ReadFormat(self, data):
        return self.ReadWithConfig(data)[0]

    def ReadWithConfig(self, data):
        data = bytes(data)
        info = parse(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        audio = [np.zeros(info.audio_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
        check(_lib.lib().vga_adx_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), _ptr_array(u8p, audio)))
        key = self.EncryptionKey                                 # ReadFile (:31): EncryptionKey ?? FindKey(structure)
        if key is None and info.revision != 0:
            key = CriAdxEncryption.FindKey(audio, info.revision, info.frame_size, self.Keys)
        if key is not None:                                      # ToAudioStream (:40-43)
            CriAdxEncryption.EncryptDecrypt(audio, key, info.revision, info.frame_size)
        cfg = AdxConfiguration(FrameSize=info.frame_size, Type=info.type, EncryptionType=info.revision, EncryptionKey=key)
        return self._to_format(info, audio), cfg                 # GetConfiguration (:59-69)

    @staticmethod
    def _to_format(info, audio):
        """ToAudioStream (:45-56)."""
        ins = info.inserted_samples
        chans = [CriAdxChannel(audio[c], int(info.history[c][0]), info.version) for c in range(info.channel_count)]
        return CriAdxFormat(chans, info.sample_count - ins, info.sample_rate, info.frame_size, info.highpass_frequency, ins,
                            info.type, info.version, bool(info.looping), info.loop_start_sample - ins, info.loop_end_sample - ins)


# ---------------------------------------------------------------- sets of files on the device (include/vgaudio_hip/adx_files.h)
def _adx_file(f):
    if isinstance(f, _lib.AdxFileC):
        return f
    channels, params = f
    return _lib.AdxFileC(int(channels), params if isinstance(params, _lib.AdxFileParamsC) else _lib.AdxFileParamsC(*params))


class AdxFileSet(FileSetBase):
    """A set of ADX files of different shapes, resident on the device (include/vgaudio_hip/adx_files.h has the layout): the
    channels of all files are packed rows -- as criadx.RaggedAdx leaves its output, or at the caller's `audio_offsets` --, the
    images one packed buffer.  `files`: one _lib.AdxFileC or (channels, _lib.AdxFileParamsC) per file, the params what
    vga_adx_write_device takes.  The tensors are the caller's torch tensors on the current device; the calls run on torch's
    current stream and do not synchronise it."""
    _destroy = "vga_adx_files_destroy"

    def __init__(self, files=None, audio_offsets=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            keep, offs = _i64_or_none(audio_offsets)
            check(_lib.lib().vga_adx_files_create(arr, n, offs, C.byref(self._h)))
            self.image_sizes = [self.file_layout(arr[i]).file_size for i in range(n)]
        self.totals = _lib.AdxFilesTotalsC()
        check(_lib.lib().vga_adx_files_totals_of(self._h, C.byref(self.totals)))
        nf, nch = self.totals.files, self.totals.channels
        fc, ao, io = np.zeros(max(nf, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_adx_files_offsets(self._h, fc.ctypes.data_as(C.POINTER(C.c_int)), ao.ctypes.data_as(i64p), io.ctypes.data_as(i64p)))
        self.first_channel, self.audio_offsets, self.image_offsets = fc[:nf], ao[:nch], io[:nf]
        self.files, self.channels = nf, nch

    @staticmethod
    def _files_array(files):
        files = [_adx_file(f) for f in (files or [])]
        return (_lib.AdxFileC * max(len(files), 1))(*files), len(files)

    @staticmethod
    def file_layout(f):
        """vga_adx_file_layout_for of one file of a set"""
        L = _lib.AdxFileLayoutC()
        check(_lib.lib().vga_adx_file_layout_for(C.byref(f.params), f.channels, C.byref(L)))
        return L

    @classmethod
    def layout(cls, files, audio_offsets=None):
        """(first_channel int32[files], audio_offsets int64[channels], image_offsets int64[files], AdxFilesTotalsC): host only,
        needs no GPU"""
        arr, n = cls._files_array(files)
        nch = sum(arr[i].channels for i in range(n) if arr[i].channels > 0)
        fc, ao, io = np.zeros(max(n, 1), np.int32), np.zeros(max(nch, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.AdxFilesTotalsC(), C.POINTER(C.c_int64)
        keep, offs = _i64_or_none(audio_offsets)
        check(_lib.lib().vga_adx_files_layout_for(arr, n, offs, fc.ctypes.data_as(C.POINTER(C.c_int)), ao.ctypes.data_as(i64p),
                                                  io.ctypes.data_as(i64p), C.byref(tot)))
        return fc[:n], ao[:tot.channels], io[:n], tot

    @classmethod
    def from_infos(cls, infos, image_offsets=None):
        """A set for reading, from the vga_adx_file_info of every file (parse()); image_offsets: any byte offsets, or None for
        images packed as write_device packs them"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) for i in infos])
        keep, offs = _i64_or_none(image_offsets)
        h = C.c_void_p()
        check(_lib.lib().vga_adx_files_create_from_infos(ptrs, n, offs, C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
        return s

    @classmethod
    def write_items(cls, files, audio_offsets=None, general=False):
        """the work items of vga_adx_write_device_v on such a set (_lib.AdxFilesItemC), host only"""
        arr, n = cls._files_array(files)
        keep, offs = _i64_or_none(audio_offsets)
        return fetch_items(_lib.lib().vga_adx_files_write_items_for, (arr, n, offs, int(general)), _lib.AdxFilesItemC)

    @classmethod
    def read_items(cls, infos, image_offsets=None, general=False):
        """the work items of vga_adx_read_device_v on a set of such infos, host only"""
        infos = list(infos)
        ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos])
        keep, offs = _i64_or_none(image_offsets)
        return fetch_items(_lib.lib().vga_adx_files_read_items_for, (ptrs, len(infos), offs, int(general)), _lib.AdxFilesItemC)

    def stats(self):
        """(span files, general files, span items, general items) of a call made by this thread now"""
        out = (C.c_int64 * 4)()
        check(_lib.lib().vga_adx_files_stats(self._h, out))
        return tuple(out)

    def write_device(self, audio, images, history=None, stream=None):
        """vga_adx_write_device_v.  audio: uint8[totals.audio_bytes] (the rows), history: int16[channels] (needed if any file is
        version 4); images: uint8[totals.image_bytes]"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        check(_lib.lib().vga_adx_write_device_v(self._h, ptr(audio, torch.uint8, t.audio_bytes, "audio"),
                                                ptr(history, torch.int16, self.channels, "history"),
                                                ptr(images, torch.uint8, t.image_bytes, "images"), DspFileSet._stream(stream)))

    def read_device(self, images, audio, history=None, stream=None):
        """vga_adx_read_device_v (a set from from_infos): images -> the rows of audio and, if given, the start history of
        every row"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        check(_lib.lib().vga_adx_read_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"),
                                               ptr(audio, torch.uint8, t.audio_bytes, "audio"),
                                               ptr(history, torch.int16, self.channels, "history"), DspFileSet._stream(stream)))

    # ---- keyed calls (include/vgaudio_hip_files/adx_keyed_files.h)
    @staticmethod
    def _keys(keys):
        """(address, count) of device keys: an int32 tensor of 3 * n values (device_keys)"""
        import torch
        if keys is None:
            return None, 0
        if not (isinstance(keys, torch.Tensor) and keys.is_cuda and keys.dtype == torch.int32 and keys.is_contiguous() and keys.numel() % 3 == 0):
            raise _lib.ArgumentError("keys: a contiguous int32 tensor on the device, (seed, mult, inc) per key (adx.device_keys)")
        return keys.data_ptr(), keys.numel() // 3

    def write_keyed_device(self, audio, images, keys, key_index=None, history=None, status=None, stream=None):
        """vga_adx_write_keyed_device_v: write_device with the audio of file f encrypted under keys[key_index[f]] (key_index None:
        keys[0] for every file; an index < 0: unkeyed) and the file's own encryption type.  keys: device_keys(...);
        key_index, status: int32[files] on the device or None"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        kp, nk = self._keys(keys)
        check(_lib.lib().vga_adx_write_keyed_device_v(self._h, ptr(audio, torch.uint8, t.audio_bytes, "audio"),
                                                      ptr(history, torch.int16, self.channels, "history"), kp, nk,
                                                      ptr(key_index, torch.int32, self.files, "key_index"),
                                                      ptr(images, torch.uint8, t.image_bytes, "images"),
                                                      ptr(status, torch.int32, self.files, "status"), DspFileSet._stream(stream)))

    def read_keyed_device(self, images, audio, keys, key_index=None, history=None, status=None, stream=None):
        """vga_adx_read_keyed_device_v (a set from from_infos): read_device with the rows of file f decrypted under
        keys[key_index[f]] and encryption type = the file's revision.  key_index: e.g. what find_keys_device returned"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        kp, nk = self._keys(keys)
        check(_lib.lib().vga_adx_read_keyed_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"), kp, nk,
                                                     ptr(key_index, torch.int32, self.files, "key_index"),
                                                     ptr(audio, torch.uint8, t.audio_bytes, "audio"),
                                                     ptr(history, torch.int16, self.channels, "history"),
                                                     ptr(status, torch.int32, self.files, "status"), DspFileSet._stream(stream)))

    def find_keys_workspace_bytes(self, nkeys8, nkeys9):
        return int(_lib.lib().vga_adx_find_keys_workspace_bytes(self._h, int(nkeys8), int(nkeys9)))

    def find_keys_device(self, images, keys8, keys9, workspace=None, stream=None):
        """vga_adx_find_keys_device_v (a set from from_infos).  keys8 / keys9: device_keys(...) or None, the candidates for files
        of revision 8 / of any other non-zero revision.  Returns an int32[files] device tensor of indices into
        torch.cat([keys8, keys9]) (-1: no candidate fits), written on the stream and not read here: it goes straight into
        read_keyed_device with keys = that concatenation.  workspace: uint8[find_keys_workspace_bytes] or None (allocated)."""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        (_, n8), (_, n9) = self._keys(keys8), self._keys(keys9)
        both = [k for k in (keys8, keys9) if k is not None and k.numel()]
        keys = both[0] if len(both) == 1 else torch.cat(both) if both else None
        need = self.find_keys_workspace_bytes(n8, n9)
        if workspace is None:
            workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=images.device)
        index = torch.empty(max(self.files, 1), dtype=torch.int32, device=images.device)
        check(_lib.lib().vga_adx_find_keys_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"), self._keys(keys)[0], n8, n9,
                                                    index.data_ptr(), ptr(workspace, torch.uint8, need, "workspace"), workspace.numel(),
                                                    DspFileSet._stream(stream)))
        self._find_keep = (keys, workspace)                            # alive until the next call (the stream may still read them)
        return index[:self.files]

    @classmethod
    def find_items(cls, infos, image_offsets=None):
        """the work items of find_keys_device's scan on a set of such infos (_lib.AdxFindKeysItemC), host only"""
        infos = list(infos)
        ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos])
        keep, offs = _i64_or_none(image_offsets)
        return fetch_items(_lib.lib().vga_adx_find_keys_items_for, (ptrs, len(infos), offs), _lib.AdxFindKeysItemC)


def device_keys(keys):
    """a list of CriAdxKey as the keyed calls of AdxFileSet take it: an int32 tensor (seed, mult, inc per key) on the device"""
    import torch
    host = np.array([[k.Seed, k.Mult, k.Inc] for k in keys], dtype=np.int32).reshape(-1)
    return torch.from_numpy(host).cuda()


def write_files(pcm16_list, configuration=None):
    """AdxWriter(configuration).GetFile(file) for a list of Pcm16Format files, on the device and without a launch per file: the
    files are grouped by the codec parameter set they need (sample rate, loop padding), one criadx.RaggedAdx per group encodes
    into one buffer, one AdxFileSet over all of them writes the images -- encrypted inside that call when the configuration
    carries an EncryptionKey (AdxWriter.cs:123-131).  Returns one `bytes` per file, in the caller's order.
    A file the encoder refuses (no samples with version 4 and no padding) raises, naming the file."""
    import torch
    from .criadx import RaggedAdx, _get_next_multiple
    cfg = configuration or AdxConfiguration()
    files = list(pcm16_list)
    spf = (cfg.FrameSize - 2) * 2
    groups, align = {}, []
    for i, f in enumerate(files):
        loop_start = f.LoopStart if f.Looping else 0
        a = _get_next_multiple(loop_start, spf * 2 if f.ChannelCount == 1 else spf) - loop_start      # CriAdxFormat.cs:59-62
        align.append(a)
        if f.SampleCount == 0 and cfg.Version == 4 and a == 0:
            raise _lib.ArgumentError("file %d: empty PCM: the reference reads pcm[0] (CriAdxCodec.cs:71)" % i)
        groups.setdefault((f.SampleRate, a), []).append(i)
    order = [i for members in groups.values() for i in members]
    described = []
    for i in order:
        f, a = files[i], align[i]
        looping = bool(f.Looping)
        described.append(_lib.AdxFileC(f.ChannelCount, _lib.AdxFileParamsC(
            f.SampleRate, f.SampleCount + a, int(looping), (f.LoopStart if looping else 0) + a, (f.LoopEnd if looping else 0) + a, a,
            cfg.FrameSize, cfg.Version, cfg.Type, 500, cfg.EncryptionType, int(bool(cfg.TrimFile)))))
    AdxFileSet.layout(described)                                   # every refusal of a file, before anything is allocated
    if not files:
        return []
    ragged, s = [], None
    try:
        pcm_at = adx_at = 0
        offsets, pcm_parts = [], []
        for (rate, a), members in groups.items():
            params = CriAdxParameters(SampleRate=rate, FrameSize=cfg.FrameSize, Padding=a, Filter=cfg.Filter, Type=cfg.Type, Version=cfg.Version)
            r = RaggedAdx(params, [files[i].SampleCount for i in members for _ in range(files[i].ChannelCount)])
            ragged.append((r, pcm_at, adx_at, len(offsets)))
            host, c = np.zeros(r.totals.pcm_samples, dtype=np.int16), 0
            for i in members:
                for ch in files[i].Channels:
                    n = files[i].SampleCount
                    host[r.pcm_offsets[c]:r.pcm_offsets[c] + n] = np.asarray(ch, dtype=np.int16)[:n]
                    c += 1
            pcm_parts.append(host)
            offsets += [adx_at + int(o) for o in r.adx_offsets]
            pcm_at += r.totals.pcm_samples                           # multiples of 8 samples / 16 bytes: every base stays aligned
            adx_at += r.totals.adx_bytes
        s = AdxFileSet(described, audio_offsets=offsets if len(ragged) > 1 else None)
        if [int(o) for o in s.audio_offsets] != offsets:
            raise _lib.VgaError("internal: the ragged batches' rows are not the file set's")
        pcm = torch.from_numpy(np.concatenate(pcm_parts)).cuda()
        adx = torch.zeros(max(adx_at, s.totals.audio_bytes), dtype=torch.uint8, device="cuda")
        history = torch.zeros(max(s.channels, 1), dtype=torch.int16, device="cuda")
        ws = torch.empty(max(max(r.totals.encode_workspace_bytes for r, _, _, _ in ragged), 16), dtype=torch.uint8, device="cuda")
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        for r, p0, a0, c0 in ragged:
            if r.channels:
                r.encode_device(pcm[p0:], adx[a0:], ws, history=history[c0:])
        if cfg.EncryptionKey is not None:
            d_keys = device_keys([cfg.EncryptionKey])                  # (alive until the images have been copied back)
            s.write_keyed_device(adx, images, d_keys, history=history)
        else:
            s.write_device(adx, images, history=history)
        out = s.images(images)
        result = [None] * len(files)
        for k, i in enumerate(order):
            result[i] = out[k]
        return result
    finally:
        for r, _, _, _ in ragged:
            r.close()
        if s is not None:
            s.close()


def read_files(list_of_bytes, EncryptionKey=None, Keys=None, Keys8=None, Keys9=None):
    """AdxReader(EncryptionKey, Keys).ReadFormat(file) for a list of files: the headers are parsed on the host, all audio is
    taken out of the images in one call on the device.  EncryptionKey: a CriAdxKey applied to every file, whatever its revision
    (AdxReader.cs:31,40-43).  Otherwise the key of every encrypted file is searched on the device among the candidates
    (CriAdxEncryption.FindKey) and the rows are decrypted in the same read, nothing returning to the host in between: Keys is
    tried on every encrypted file, as AdxReader(Keys=...) here tries it; or Keys8 on files of revision 8 and Keys9 on every
    other non-zero revision, the reference's two lists (CriAdxEncryption.cs:46).  Returns one CriAdxFormat per file; a file no
    candidate fits stays encrypted, as AdxReader leaves it.  With no key argument nothing is searched."""
    import torch
    datas = [bytes(d) for d in list_of_bytes]
    infos = [parse(d) for d in datas]
    s = AdxFileSet.from_infos(infos)
    try:
        if s.files == 0:
            return []
        host = np.zeros(s.totals.image_bytes, dtype=np.uint8)
        for d, at, size in zip(datas, s.image_offsets, s.image_sizes):
            host[int(at):int(at) + size] = np.frombuffer(d, dtype=np.uint8)[:size]
        images = torch.from_numpy(host).cuda()
        audio = torch.zeros(s.totals.audio_bytes, dtype=torch.uint8, device="cuda")
        keys8, keys9 = list(Keys8 if Keys8 is not None else Keys or []), list(Keys9 if Keys9 is not None else Keys or [])
        if EncryptionKey is not None:
            d_keys = device_keys([EncryptionKey])                      # (alive until the rows have been copied back)
            s.read_keyed_device(images, audio, d_keys)
        elif keys8 or keys9:
            d8, d9 = (device_keys(k) if k else None for k in (keys8, keys9))
            index = s.find_keys_device(images, d8, d9)
            d_keys = device_keys(keys8 + keys9)
            s.read_keyed_device(images, audio, d_keys, key_index=index)
        else:
            s.read_device(images, audio)
        rows = audio.cpu().numpy()
        out = []
        for f, info in enumerate(infos):
            first = int(s.first_channel[f])
            chans = [rows[int(s.audio_offsets[first + c]):int(s.audio_offsets[first + c]) + info.audio_bytes].copy()
                     for c in range(info.channel_count)]
            out.append(AdxReader._to_format(info, chans))
        return out
    finally:
        s.close()
