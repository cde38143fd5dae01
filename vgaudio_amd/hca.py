"""HCA container -- host-side mirror of VGAudio/Containers/Hca/HcaWriter.cs, HcaReader.cs and
HcaConfiguration.cs over vga_hca_write / vga_hca_file_header and vga_hca_parse / vga_hca_read (frames copied and their
CRCs checked on the GPU; decryption by vga_hca_crypt)."""
import ctypes as C

import numpy as np

from . import _lib
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
