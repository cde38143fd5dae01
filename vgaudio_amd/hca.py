"""HCA container -- host-side mirror of VGAudio/Containers/Hca/HcaWriter.cs, HcaReader.cs and
HcaConfiguration.cs over vga_hca_write / vga_hca_file_header and vga_hca_parse / vga_hca_read (frames copied and their
CRCs checked on the GPU; decryption by vga_hca_crypt)."""
import ctypes as C

import numpy as np

from . import _lib
from ._fileset import FileSetBase, fetch_items, i64_or_none as _i64_or_none
from ._lib import check, u8p
from .crihca import CriHcaEncryption, CriHcaFormat, CriHcaKey, CriHcaParameters, CriHcaQuality, HcaInfo
from .gcadpcm import Pcm16Format


class HcaConfiguration:
    """Containers/Hca/HcaConfiguration.cs:5-11."""

    def __init__(self, EncryptionKey=None, Quality=CriHcaQuality.NotSet, Bitrate=0, LimitBitrate=False, Progress=None):
        self.EncryptionKey, self.Quality, self.Bitrate, self.LimitBitrate, self.Progress = (
            EncryptionKey, Quality, Bitrate, LimitBitrate, Progress)


class HcaWriter:
    """AudioWriter<HcaWriter, HcaConfiguration>: GetFile(audio, configuration)."""

    def __init__(self, configuration=None):
        self.Configuration = configuration or HcaConfiguration()

    def _setup(self, audio):                                 # SetupWriter (:23-46)
        cfg = self.Configuration
        if isinstance(audio, Pcm16Format):
            enc = CriHcaParameters(Progress=cfg.Progress, Bitrate=cfg.Bitrate, LimitBitrate=cfg.LimitBitrate)
            if cfg.Quality != CriHcaQuality.NotSet:
                enc.Quality = cfg.Quality
            audio = CriHcaFormat().EncodeFromPcm16(audio, enc)
        if not isinstance(audio, CriHcaFormat):
            raise _lib.ArgumentError("HcaWriter takes a CriHcaFormat or a Pcm16Format")
        if cfg.EncryptionKey is not None:                    # :39-45 -- like the reference, this encrypts the format's frames in place
            audio.AudioData = np.ascontiguousarray(audio.AudioData, dtype=np.uint8)
            CriHcaEncryption.Crypt(audio.Hca, audio.AudioData, cfg.EncryptionKey, False)
            audio.Hca.EncryptionType = cfg.EncryptionKey.KeyType
        return audio

    @staticmethod
    def _comment(hca):
        return None if hca.Comment is None else hca.Comment.encode("utf-8")

    def GetHeader(self, fmt):
        hca = fmt.Hca
        out = np.zeros(hca.HeaderSize, dtype=np.uint8)
        check(_lib.lib().vga_hca_file_header(C.byref(hca.c), self._comment(hca), float(hca.Volume), int(hca.EncryptionType),
                                             int(self.Configuration.EncryptionKey is not None), out.ctypes.data_as(u8p)))
        return out.tobytes()

    def GetFile(self, audio, configuration=None):
        if configuration is not None:
            self.Configuration = configuration
        fmt = self._setup(audio)
        hca = fmt.Hca
        size = _lib.lib().vga_hca_file_size(C.byref(hca.c))
        if size < 0:
            check(size)
        frames = np.ascontiguousarray(fmt.AudioData, dtype=np.uint8).reshape(-1)
        if len(frames) != hca.FrameCount * hca.FrameSize:
            raise _lib.ArgumentError("AudioData does not hold FrameCount frames of FrameSize bytes")
        out = np.zeros(size, dtype=np.uint8)
        check(_lib.lib().vga_hca_write(C.byref(hca.c), frames.ctypes.data_as(u8p), self._comment(hca), float(hca.Volume),
                                       int(hca.EncryptionType), int(self.Configuration.EncryptionKey is not None),
                                       out.ctypes.data_as(u8p)))
        return out.tobytes()


def parse(data):
    """vga_hca_parse: HcaReader.ReadHcaHeader and the size of the frames (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.HcaFileInfoC()
    check(_lib.lib().vga_hca_parse(buf.ctypes.data_as(u8p), len(buf), C.byref(info)))
    return info


def hca_info_of(info):
    """The HcaInfo the reader builds: the codec fields plus Comment, Volume and EncryptionType."""
    hca = HcaInfo(_lib.HcaInfoC.from_buffer_copy(info.hca))
    hca.Comment = info.comment.decode("utf-8", "replace") if info.has_comment else None
    hca.Volume = info.volume
    hca.EncryptionType = info.encryption_type
    return hca


class HcaReader:
    """AudioReader<HcaReader, HcaStructure, HcaConfiguration> (Containers/Hca/HcaReader.cs).  Decrypt = False leaves the
    frames and EncryptionType as they are; EncryptionKey: a CriHcaKey or None; Keys: the candidates FindKey tries for
    type 56 files when no key is given (the reference's list, CriHcaEncryptionKeys.cs, stays with the caller).
    BadCrcFrames: after a read, the frames whose CRC-16 did not match (kept, as in the reference)."""

    def __init__(self, Decrypt=True, EncryptionKey=None, Keys=None):
        self.Decrypt = Decrypt
        self.EncryptionKey = EncryptionKey
        self.Keys = list(Keys) if Keys else []
        self.BadCrcFrames = 0

    def ReadMetadata(self, data):
        return parse(data)

    def ReadFormat(self, data):
        return self.ReadWithConfig(data)[0]

    def _find_key(self, hca, frames):                        # FindKey (:238-252)
        if hca.EncryptionType == 1:
            return CriHcaKey(CriHcaKey.Type1)
        if hca.EncryptionType == 56:
            key = CriHcaEncryption.FindKey(hca, frames, self.Keys)
            if key is None:
                raise _lib.InvalidDataError("Cannot find key to decrypt HCA file.")
            return key
        return None

    def ReadWithConfig(self, data):
        data = bytes(data)
        info = parse(data)
        hca = hca_info_of(info)
        buf = np.frombuffer(data, dtype=np.uint8)
        frames = np.zeros((hca.FrameCount, hca.FrameSize), dtype=np.uint8)
        bad = C.c_int(0)
        check(_lib.lib().vga_hca_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), frames.ctypes.data_as(u8p), C.byref(bad)))
        self.BadCrcFrames = bad.value
        key = (self.EncryptionKey if self.EncryptionKey is not None else self._find_key(hca, frames)) if self.Decrypt else None
        if key is not None:                                      # ToAudioStream (:39-49)
            CriHcaEncryption.Crypt(hca, frames, key, True)
            hca.EncryptionType = 0
        return CriHcaFormat(frames, hca), HcaConfiguration(EncryptionKey=key)     # GetConfiguration (:51-57)


# ---------------------------------------------------------------- sets of files on the device (include/vgaudio_hip/hca_files.h)
def _tables_or_none(tables):
    """ntables x 256 bytes -> (keep-alive, pointer, count)"""
    if tables is None or len(tables) == 0:
        return None, None, 0
    a = np.ascontiguousarray(np.asarray(tables, dtype=np.uint8).reshape(-1, 256))
    return a, a.ctypes.data_as(u8p), len(a)


def _hca_file(f):
    if isinstance(f, _lib.HcaFileC):
        return f
    info, comment, volume, encryption_type, encrypted_ids, key = f
    c = _lib.HcaInfoC.from_buffer_copy(info.c if isinstance(info, HcaInfo) else info)
    if isinstance(comment, str):
        comment = comment.encode("utf-8")
    return _lib.HcaFileC(c, comment, float(volume), int(encryption_type), int(encrypted_ids), int(key))


class HcaFileSet(FileSetBase):
    """A set of HCA files of different shapes, resident on the device (include/vgaudio_hip/hca_files.h has the layout): the
    frames of all files lie packed -- as crihca.RaggedHca leaves its output, or at the caller's `frame_offsets` --, the images
    in one packed buffer.  `files`: one _lib.HcaFileC or (info, comment, volume, encryption_type, encrypted_ids, key) per file:
    what vga_hca_write_device takes, and the index of the file's table in `tables` (ntables x 256 bytes; -1: no key).  The
    tensors are the caller's torch tensors on the current device; the calls run on torch's current stream and do not
    synchronise it."""
    _destroy = "vga_hca_files_destroy"

    def __init__(self, files=None, frame_offsets=None, tables=None, _handle=None):
        self._h, self.image_sizes = C.c_void_p(), None
        if _handle is not None:
            self._h = _handle
        else:
            arr, n = self._files_array(files)
            keep, offs = _i64_or_none(frame_offsets)
            keep_t, tp, nt = _tables_or_none(tables)
            check(_lib.lib().vga_hca_files_create(arr, n, offs, tp, nt, C.byref(self._h)))
            self.image_sizes = [arr[i].hca.header_size + arr[i].hca.frame_count * arr[i].hca.frame_size for i in range(n)]
        self.totals = _lib.HcaFilesTotalsC()
        check(_lib.lib().vga_hca_files_totals_of(self._h, C.byref(self.totals)))
        nf = self.totals.files
        fo, io = np.zeros(max(nf, 1), np.int64), np.zeros(max(nf, 1), np.int64)
        i64p = C.POINTER(C.c_int64)
        check(_lib.lib().vga_hca_files_offsets(self._h, fo.ctypes.data_as(i64p), io.ctypes.data_as(i64p)))
        self.frame_offsets, self.image_offsets = fo[:nf], io[:nf]
        self.files = nf

    @staticmethod
    def _files_array(files):
        files = [_hca_file(f) for f in (files or [])]
        return (_lib.HcaFileC * max(len(files), 1))(*files), len(files)

    @classmethod
    def layout(cls, files, frame_offsets=None):
        """(frame_offsets int64[files], image_offsets int64[files], HcaFilesTotalsC): host only, needs no GPU"""
        arr, n = cls._files_array(files)
        fo, io = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
        tot, i64p = _lib.HcaFilesTotalsC(), C.POINTER(C.c_int64)
        keep, offs = _i64_or_none(frame_offsets)
        check(_lib.lib().vga_hca_files_layout_for(arr, n, offs, fo.ctypes.data_as(i64p), io.ctypes.data_as(i64p), C.byref(tot)))
        return fo[:n], io[:n], tot

    @classmethod
    def from_infos(cls, infos, image_offsets=None, keys=None, tables=None, frame_offsets=None):
        """A set for reading, from the vga_hca_file_info of every file (parse()); image_offsets: any byte offsets, or None for
        images packed as write_device packs them; keys: one index into `tables` (decryption tables) per file, -1 for none"""
        infos = list(infos)
        n = len(infos)
        ptrs = (C.c_void_p * max(n, 1))(*[C.addressof(i) if i is not None else None for i in infos])
        keep, offs = _i64_or_none(image_offsets)
        keep_f, foffs = _i64_or_none(frame_offsets)
        keep_t, tp, nt = _tables_or_none(tables)
        kp = None
        if keys is not None:
            keep_k = np.ascontiguousarray(list(keys) + [0], dtype=np.int32)
            kp = keep_k.ctypes.data_as(C.POINTER(C.c_int))
        h = C.c_void_p()
        check(_lib.lib().vga_hca_files_create_from_infos(ptrs, n, offs, kp, tp, nt, foffs, C.byref(h)))
        s = cls(_handle=h)
        s.image_sizes = [i.frames_offset + i.hca.frame_count * i.hca.frame_size for i in infos]
        return s

    @classmethod
    def write_items(cls, files, frame_offsets=None, general=False):
        """the work items of vga_hca_write_device_v on such a set (_lib.HcaFilesItemC), host only"""
        arr, n = cls._files_array(files)
        keep, offs = _i64_or_none(frame_offsets)
        return fetch_items(_lib.lib().vga_hca_files_write_items_for, (arr, n, offs, int(general)), _lib.HcaFilesItemC)

    @classmethod
    def read_items(cls, infos, image_offsets=None, frame_offsets=None, general=False):
        """the work items of vga_hca_read_device_v on a set of such infos, host only"""
        infos = list(infos)
        ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos])
        keep, offs = _i64_or_none(image_offsets)
        keep_f, foffs = _i64_or_none(frame_offsets)
        return fetch_items(_lib.lib().vga_hca_files_read_items_for, (ptrs, len(infos), offs, foffs, int(general)), _lib.HcaFilesItemC)

    def stats(self):
        """(span files, general files, span items, general items) of a call made by this thread now"""
        out = (C.c_int64 * 4)()
        check(_lib.lib().vga_hca_files_stats(self._h, out))
        return tuple(out)

    def write_device(self, frames, images, stream=None):
        """vga_hca_write_device_v.  frames: uint8[totals.frame_bytes]; images: uint8[totals.image_bytes]"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        check(_lib.lib().vga_hca_write_device_v(self._h, ptr(frames, torch.uint8, t.frame_bytes, "frames"),
                                                ptr(images, torch.uint8, t.image_bytes, "images"), DspFileSet._stream(stream)))

    def read_device(self, images, frames, bad_crc=None, stream=None):
        """vga_hca_read_device_v (a set from from_infos): images -> the frames and, if given, the bad-CRC counts ADDED to
        bad_crc (int32[files], zeroed by the caller)"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        check(_lib.lib().vga_hca_read_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"),
                                               ptr(frames, torch.uint8, t.frame_bytes, "frames"),
                                               ptr(bad_crc, torch.int32, self.files, "bad_crc"), DspFileSet._stream(stream)))

    # ---- keys on the device (include/vgaudio_hip_files/hca_keyed_files.h)
    def find_keys_workspace_bytes(self, nkeys):
        return int(_lib.lib().vga_hca_find_keys_workspace_bytes(self._h, int(nkeys)))

    def find_keys_device(self, images, tables, nkeys, type1_index=-1, status=None, workspace=None, stream=None):
        """vga_hca_find_keys_device_v (a set from from_infos, made without keys).  tables: a uint8 device tensor of decryption
        tables, 256 bytes each (device_tables), whose first `nkeys` are the candidates for type-56 files; type1_index: what a
        type-1 file gets.  Returns an int32[files] device tensor of table indices (-1: none), written on the stream and not
        read here: it goes straight into read_keyed_device.  status: int32[files] or None; workspace: uint8[
        find_keys_workspace_bytes(nkeys)] or None (allocated).  The object is not changed: what the call allocates (the index
        tensor, the workspace when none is given) is recorded on `stream`, so torch's allocator does not hand it out again while
        that stream still uses it; `tables` and a workspace of the caller's are the caller's to keep alive."""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        need = self.find_keys_workspace_bytes(nkeys)
        own_workspace = None
        if workspace is None:
            workspace = own_workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=images.device)
        index = torch.empty(max(self.files, 1), dtype=torch.int32, device=images.device)
        check(_lib.lib().vga_hca_find_keys_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"),
                                                    ptr(tables, torch.uint8, 256 * max(int(nkeys), 0), "tables"), int(nkeys), int(type1_index),
                                                    index.data_ptr(), ptr(status, torch.int32, self.files, "status"),
                                                    ptr(workspace, torch.uint8, need, "workspace"), workspace.numel(),
                                                    DspFileSet._stream(stream)))
        if stream is not None:                                         # what this call allocated is used on the caller's stream
            for t_ in ([index] if own_workspace is None else [index, own_workspace]):
                t_.record_stream(stream)
        return index[:self.files]

    def read_keyed_device(self, images, tables, frames, key_index=None, bad_crc=None, status=None, stream=None):
        """vga_hca_read_keyed_device_v (a set from from_infos, made without keys): read_device with file f deciphered through
        tables[key_index[f]] (uint8 device tensor, 256 bytes a table; key_index: int32[files] on the device, e.g. what
        find_keys_device returned, or None for table 0); status: int32[files] or None"""
        import torch
        from .dsp import DspFileSet
        ptr, t = DspFileSet._ptr, self.totals
        ntables = 0 if tables is None else tables.numel() // 256
        check(_lib.lib().vga_hca_read_keyed_device_v(self._h, ptr(images, torch.uint8, t.image_bytes, "images"),
                                                     ptr(tables, torch.uint8, 0, "tables"), ntables,
                                                     ptr(key_index, torch.int32, self.files, "key_index"),
                                                     ptr(frames, torch.uint8, t.frame_bytes, "frames"),
                                                     ptr(bad_crc, torch.int32, self.files, "bad_crc"),
                                                     ptr(status, torch.int32, self.files, "status"), DspFileSet._stream(stream)))

    @classmethod
    def find_items(cls, infos, nkeys):
        """the work items of find_keys_device's test launches on a set of such infos (_lib.HcaFindKeysItemC), host only"""
        infos = list(infos)
        ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos])
        return fetch_items(_lib.lib().vga_hca_find_keys_items_for, (ptrs, len(infos), int(nkeys)), _lib.HcaFindKeysItemC)


def device_tables(keys):
    """a list of CriHcaKey as the keyed calls of HcaFileSet take it: their decryption tables, 256 bytes each, as one uint8
    tensor on the device"""
    import torch
    host = np.ascontiguousarray(np.stack([k.DecryptionTable for k in keys]), dtype=np.uint8).reshape(-1)
    return torch.from_numpy(host.copy()).cuda()


def _shape_class(h):
    """what the streams of one crihca.RaggedHca must agree in (include/vgaudio_hip/hca_ragged.h)"""
    return (h.channel_count, h.sample_rate, h.frame_size, h.min_resolution, h.max_resolution, h.track_count, h.channel_config,
            h.total_band_count, h.base_band_count, h.stereo_band_count, h.bands_per_hfr_group, h.hfr_group_count, h.use_ath_curve)


def plan_write_groups(infos, sample_counts):
    """How write_files routes its files: (groups, singles).  groups: lists of file indices, one crihca.RaggedHca (one set of
    encode launches) each, by shape class in the order the classes first appear; singles: the files that get a
    vga_hca_encode_device call of their own.  A looping file joins its class like any other, except where
      * the file holds audio behind its HcaInfo.sample_count (sample_counts[i] > infos[i].sample_count) and the reference's
        encoder would read it (crihca.loop_may_read_tail: a loop shorter than the post audio) -- a packed row ends at
        sample_count and cannot supply it --, or
      * its class would be that file alone: its own call costs no object.
    Host only, needs no GPU."""
    from .crihca import loop_may_read_tail
    groups, singles = {}, []
    for i, (h, n) in enumerate(zip(infos, sample_counts)):
        if h.looping and n > h.sample_count and loop_may_read_tail(h):
            singles.append(i)
        else:
            groups.setdefault(_shape_class(h), []).append(i)
    for key in [k for k, m in groups.items() if len(m) == 1 and infos[m[0]].looping]:
        singles += groups.pop(key)
    return list(groups.values()), sorted(singles)


def write_files(pcm16_list, configuration=None):
    """HcaWriter(configuration).GetFile(file) for a list of Pcm16Format files, on the device and without a launch per file or
    per key: the files are grouped by shape class and one crihca.RaggedHca per class encodes them, looping files beside plain
    ones (encode_loops_device); the few files plan_write_groups names are encoded by vga_hca_encode_device into their own
    place, all of it at explicit offsets in one frames buffer; one HcaFileSet over everything encrypts
    (configuration.EncryptionKey: every file gets its table, KeyType as encryption type and masked chunk ids) and writes the
    images.  Returns one `bytes` per file, in the caller's order."""
    import torch
    from .crihca import RaggedHca
    cfg = configuration or HcaConfiguration()
    files = list(pcm16_list)
    L = _lib.lib()
    infos = []
    for i, f in enumerate(files):
        p = CriHcaParameters(Bitrate=cfg.Bitrate, LimitBitrate=cfg.LimitBitrate, ChannelCount=f.ChannelCount, SampleRate=f.SampleRate,
                             SampleCount=f.SampleCount, Looping=bool(f.Looping), LoopStart=f.LoopStart if f.Looping else 0,
                             LoopEnd=f.LoopEnd if f.Looping else 0)
        if cfg.Quality != CriHcaQuality.NotSet:
            p.Quality = cfg.Quality
        c, h = p._c(), _lib.HcaInfoC()
        try:
            check(L.vga_hca_encoder_initialize(C.byref(c), C.byref(h)))
        except _lib.VgaError as e:
            raise type(e)("file %d: %s" % (i, e)) from None
        infos.append(h)
    key = cfg.EncryptionKey
    enc_type, tables = (key.KeyType, [key.EncryptionTable]) if key is not None else (0, None)
    groups, loops = plan_write_groups(infos, [f.SampleCount for f in files])
    order = [i for members in groups for i in members] + loops
    described = [_lib.HcaFileC(infos[i], None, 1.0, enc_type, int(key is not None), 0 if key is not None else -1) for i in order]
    HcaFileSet.layout(described)                                      # every refusal of a file, before anything is allocated
    if not files:
        return []
    ragged, s = [], None
    try:
        frames_at, offsets, jobs = 0, [], []
        for members in groups:
            r = RaggedHca([infos[i] for i in members])
            host, row = np.zeros(max(r.totals.pcm_samples, 8), dtype=np.int16), 0
            for i in members:
                for ch in files[i].Channels:
                    n = infos[i].sample_count                         # (a looping file's rows end where its HcaInfo does)
                    host[r.pcm_row_offsets[row]:r.pcm_row_offsets[row] + n] = np.asarray(ch, dtype=np.int16)[:n]
                    row += 1
            ragged.append(r)
            jobs.append((r, host, frames_at))
            offsets += [frames_at + int(o) for o in r.frame_offsets]
            frames_at += (r.totals.frame_bytes + 15) // 16 * 16
        loop_jobs = []
        for i in loops:
            h, f = infos[i], files[i]
            n = f.SampleCount
            host = np.zeros((h.channel_count, max(n, 1)), dtype=np.int16)
            for c, ch in enumerate(f.Channels):
                host[c, :n] = np.asarray(ch, dtype=np.int16)[:n]
            loop_jobs.append((h, host, n, frames_at))
            offsets.append(frames_at)
            frames_at += (h.frame_count * h.frame_size + 8 + 15) // 16 * 16
        s = HcaFileSet(described, frame_offsets=offsets, tables=tables)
        frames = torch.zeros(max(frames_at, s.totals.frame_bytes), dtype=torch.uint8, device="cuda")
        images = torch.empty(s.totals.image_bytes, dtype=torch.uint8, device="cuda")
        status = torch.zeros(len(files) + 1, dtype=torch.int32, device="cuda")
        st, done, keep = C.c_void_p(torch.cuda.current_stream().cuda_stream), 0, []
        for r, host, at in jobs:
            pcm = torch.from_numpy(host).cuda()
            keep.append(pcm)
            if r.streams:
                r.encode_loops_device(pcm, frames[at:], status[done:])
            done += r.streams
        for h, host, n, at in loop_jobs:
            pcm = torch.from_numpy(host).cuda()
            keep.append(pcm)
            check(L.vga_hca_encode_device(pcm.data_ptr(), pcm.numel(), pcm.shape[1], 1, n, C.byref(h), frames.data_ptr() + at,
                                          (h.frame_count * h.frame_size + 8 + 1) // 2 * 2, status.data_ptr() + 4 * done, st))
            done += 1
        s.write_device(frames, images)
        out = s.images(images)
        flags = status.cpu().numpy()
        for k, i in enumerate(order):
            if flags[k]:
                raise _lib.InvalidDataError("file %d: the encoder reports status %d" % (i, int(flags[k])))
        result = [None] * len(files)
        for k, i in enumerate(order):
            result[i] = out[k]
        return result
    finally:
        for r in ragged:
            r.close()
        if s is not None:
            s.close()


def _read_files_found(datas, infos, Keys):
    """read_files with candidates: keys found and frames deciphered on the device, one synchronisation (the copy back)"""
    import torch
    keys = list(Keys)
    s = HcaFileSet.from_infos(infos)
    try:
        if s.files == 0:
            return [], []
        host = np.zeros(s.totals.image_bytes, dtype=np.uint8)
        for d, at, size in zip(datas, s.image_offsets, s.image_sizes):
            host[int(at):int(at) + size] = np.frombuffer(d, dtype=np.uint8)[:size]
        images = torch.from_numpy(host).cuda()
        tables = device_tables(keys + [CriHcaKey(CriHcaKey.Type1)])    # the type-1 table sits behind the candidates
        frames = torch.zeros(s.totals.frame_bytes, dtype=torch.uint8, device="cuda")
        bad = torch.zeros(s.files, dtype=torch.int32, device="cuda")
        status = torch.empty(s.files, dtype=torch.int32, device="cuda")
        index = s.find_keys_device(images, tables, len(keys), type1_index=len(keys), status=status)
        s.read_keyed_device(images, tables, frames, key_index=index, bad_crc=bad)
        flat = frames.cpu().numpy()                                     # the one synchronisation
        found, state, counts = index.cpu().numpy(), status.cpu().numpy(), bad.cpu().numpy()
        for f in range(s.files):
            if state[f] == 1:
                raise _lib.InvalidDataError("file %d: Cannot find key to decrypt HCA file." % f)
            if state[f] == 2:
                raise _lib.InvalidDataError("file %d: Invalid frame header" % f)
        out = []
        for f, info in enumerate(infos):
            hca = hca_info_of(info)
            at, n = int(s.frame_offsets[f]), hca.FrameCount * hca.FrameSize
            if found[f] >= 0:
                hca.EncryptionType = 0
            out.append(CriHcaFormat(flat[at:at + n].copy().reshape(hca.FrameCount, hca.FrameSize), hca))
        return out, [int(b) for b in counts]
    finally:
        s.close()


def read_files(list_of_bytes, Decrypt=True, EncryptionKey=None, Keys=None):
    """HcaReader(Decrypt, EncryptionKey, Keys).ReadWithConfig(file) for a list of files: the headers are parsed on the host, all
    frames are taken out of the images, CRC-checked and decrypted in one vga_hca_read_device_v call.  Returns
    (formats, bad_crc): one CriHcaFormat per file, EncryptionType 0 where decrypted, and the bad-CRC frames per file.
    Keys: the candidates for type-56 files when no EncryptionKey is given; the keys are then found and used on the device
    (HcaFileSet.find_keys_device, read_keyed_device) and nothing but the final copy synchronises; a file no candidate fits
    raises "file <f>: Cannot find key to decrypt HCA file." after that copy.  Without Keys a type-56 file without a key is
    refused by name before anything runs."""
    import torch
    datas = [bytes(d) for d in list_of_bytes]
    infos = [parse(d) for d in datas]
    if Decrypt and EncryptionKey is None and Keys is not None:
        return _read_files_found(datas, infos, Keys)
    tables, keys, type1 = [], [], None
    for i, info in enumerate(infos):
        k = -1
        if Decrypt and EncryptionKey is not None:
            k = 0
        elif Decrypt and info.encryption_type == 1:
            k = type1 = len(tables) if type1 is None else type1
        elif Decrypt and info.encryption_type == 56:
            raise _lib.InvalidDataError("file %d: Cannot find key to decrypt HCA file." % i)
        if k == len(tables):
            tables.append((EncryptionKey if EncryptionKey is not None else CriHcaKey(CriHcaKey.Type1)).DecryptionTable)
        keys.append(k)
    s = HcaFileSet.from_infos(infos, keys=keys, tables=tables or None)
    try:
        if s.files == 0:
            return [], []
        host = np.zeros(s.totals.image_bytes, dtype=np.uint8)
        for d, at, size in zip(datas, s.image_offsets, s.image_sizes):
            host[int(at):int(at) + size] = np.frombuffer(d, dtype=np.uint8)[:size]
        images = torch.from_numpy(host).cuda()
        frames = torch.zeros(s.totals.frame_bytes, dtype=torch.uint8, device="cuda")
        bad = torch.zeros(s.files, dtype=torch.int32, device="cuda")
        s.read_device(images, frames, bad)
        flat = frames.cpu().numpy()
        out = []
        for f, info in enumerate(infos):
            hca = hca_info_of(info)
            at, n = int(s.frame_offsets[f]), hca.FrameCount * hca.FrameSize
            if keys[f] >= 0:
                hca.EncryptionType = 0
            out.append(CriHcaFormat(flat[at:at + n].copy().reshape(hca.FrameCount, hca.FrameSize), hca))
        return out, [int(b) for b in bad.cpu().numpy()]
    finally:
        s.close()
