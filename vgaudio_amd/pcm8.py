"""8-bit PCM -- the host-side mirror of VGAudio/Codecs/Pcm8/Pcm8Codec.cs and Formats/Pcm8 (Pcm8Format: unsigned, as in
WAVE; Pcm8SignedFormat: signed, as in NintendoWare streams).  The conversions run on the GPU
(vga_pcm8_encode_device / vga_pcm8_decode_device, include/vgaudio_hip_pcm.h).  There is no CPU path."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .gcadpcm import AudioTrack, Pcm16Format


def _rows_on_device(rows, dtype):
    import torch
    n = len(rows[0]) if rows else 0
    host = np.zeros((len(rows), max(n, 1)), dtype=dtype)
    for i, r in enumerate(rows):
        host[i, :n] = r
    return torch.from_numpy(host).to("cuda"), n


def _convert(rows, signed, encode):
    """rows of int16 (encode) or uint8 (decode) -> the other kind, one batched device call"""
    import torch
    if not rows:
        return []
    if len({len(r) for r in rows}) > 1:
        raise _lib.ArgumentError("All channels must have the same sample count")
    src, n = _rows_on_device(rows, np.int16 if encode else np.uint8)
    dst = torch.empty((len(rows), src.shape[1]), dtype=torch.uint8 if encode else torch.int16, device=src.device)
    stream = torch.cuda.current_stream().cuda_stream
    fn = _lib.lib().vga_pcm8_encode_device if encode else _lib.lib().vga_pcm8_decode_device
    check(fn(C.c_void_p(src.data_ptr()), src.shape[1], n, len(rows), int(signed), C.c_void_p(dst.data_ptr()), dst.shape[1],
             C.c_void_p(stream)))
    out = dst.cpu().numpy()
    return [np.ascontiguousarray(out[i, :n]) for i in range(len(rows))]


class Pcm8Codec:
    """Pcm8Codec.cs on the device, one channel at a time (the formats below convert all channels in one call)."""

    @staticmethod
    def Encode(array):
        return _convert([np.asarray(array, dtype=np.int16)], False, True)[0]

    @staticmethod
    def Decode(array):
        return _convert([np.asarray(array, dtype=np.uint8)], False, False)[0]

    @staticmethod
    def EncodeSigned(array):
        return _convert([np.asarray(array, dtype=np.int16)], True, True)[0]

    @staticmethod
    def DecodeSigned(array):
        return _convert([np.asarray(array, dtype=np.uint8)], True, False)[0]


class Pcm8Format:
    """Pcm8Format.cs: Channels is byte[ChannelCount][SampleCount], unsigned (0x80 = silence)."""
    Signed = False

    def __init__(self, channels=None, sampleRate=48000):
        self.Channels = [np.ascontiguousarray(c, dtype=np.uint8) for c in (channels if channels is not None else [])]
        self.SampleRate = sampleRate
        n = {len(c) for c in self.Channels}
        if len(n) > 1:
            raise _lib.ArgumentError("All channels must have the same sample count")
        self.SampleCount = n.pop() if n else 0
        self.Looping, self.LoopStart, self.LoopEnd = False, 0, 0
        self.Tracks = AudioTrack.GetDefaultTrackList(len(self.Channels))

    @property
    def ChannelCount(self):
        return len(self.Channels)

    WithLoop = Pcm16Format.WithLoop

    def WithTracks(self, tracks):
        self.Tracks = list(tracks) if tracks else AudioTrack.GetDefaultTrackList(self.ChannelCount)
        return self

    def ToPcm16(self):
        """Pcm8Format.ToPcm16 / Pcm8SignedFormat: Decode or DecodeSigned of every channel"""
        pcm = Pcm16Format(_convert(self.Channels, self.Signed, False), self.SampleRate)
        pcm.WithLoop(self.Looping, self.LoopStart, self.LoopEnd)
        pcm.Tracks = list(self.Tracks)
        return pcm

    @classmethod
    def EncodeFromPcm16(cls, pcm16):
        """Pcm8Format.EncodeFromPcm16 / Pcm8SignedFormat: Encode or EncodeSigned of every channel"""
        fmt = cls(_convert(pcm16.Channels, cls.Signed, True), pcm16.SampleRate)
        fmt.WithLoop(pcm16.Looping, pcm16.LoopStart, pcm16.LoopEnd)
        fmt.WithTracks(getattr(pcm16, "Tracks", None))
        return fmt


class Pcm8SignedFormat(Pcm8Format):
    """Pcm8SignedFormat.cs: the same bytes read as sbyte (0 = silence)."""
    Signed = True
