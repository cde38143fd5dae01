"""ADX container -- host-side mirror of VGAudio/Containers/Adx/AdxWriter.cs, AdxReader.cs and
AdxConfiguration.cs.  The image is assembled and taken apart on the GPU (vga_adx_write, vga_adx_read), encryption
included (vga_adx_crypt, vga_adx_find_key_device); only the header is parsed on the host.  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
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
