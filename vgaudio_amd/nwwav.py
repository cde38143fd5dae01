"""NintendoWare wave files (BRWAV, BCWAV, BFWAV) and stream prefetch files (BCSTP, BFSTP): BrwavReader.cs and the wave /
prefetch branches of BCFstmReader.cs over include/vgaudio_hip_nwwav.h.  One file at a time is host work; NwWaveBank
takes the channels of a whole sound bank out of one device buffer in one launch (vga_nwwav_bank_*)."""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import check, i16p, u8p
from .gcadpcm import GcAdpcmChannel, GcAdpcmContext, Pcm16Format, _ptr_array
from .nwstm import NwCodec, _stored_format
from .pcm8 import Pcm8SignedFormat


class NwWaveKind(enum.IntEnum):                   # VGA_NWWAV_*
    Rwav = 0
    Cwav = 1
    Fwav = 2
    Cstp = 3
    Fstp = 4


def parse(data):
    """vga_nwwav_parse: the file's header and channel infos (no device work)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = _lib.NwWavInfoC()
    check(_lib.lib().vga_nwwav_parse(buf.ctypes.data_as(u8p) if len(buf) else None, len(buf), C.byref(info)))
    return info


def read_channels(data, info):
    """vga_nwwav_read: every channel's bytes as stored."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rows = [np.zeros(info.channel_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
    check(_lib.lib().vga_nwwav_read(buf.ctypes.data_as(u8p), len(buf), C.byref(info), _ptr_array(u8p, rows)))
    return rows


class _NwWaveReader:
    """AudioReader<_, BxstmStructure, BxstmConfiguration>: ReadFormat(bytes) through Common.ToAudioStream."""
    magics = ()

    def ReadInfo(self, data):
        data = bytes(data)
        if data[:4] not in self.magics:
            raise _lib.InvalidDataError("File has no %s header" % " or ".join(m.decode() for m in self.magics))
        return parse(data)

    def Read(self, data):
        return self.ReadFormat(data)

    def ReadFormat(self, data):
        """GcAdpcmFormat, Pcm16Format or Pcm8SignedFormat by the codec byte, with the loop Common.ToAudioStream sets
        (LoopStart .. SampleCount; a prefetch file does not loop)."""
        data = bytes(data)
        info = self.ReadInfo(data)
        rows = read_channels(data, info)
        if info.codec == NwCodec.GcAdpcm:
            chans = []
            for c, row in enumerate(rows):
                ch = GcAdpcmChannel(row, np.array(info.coefs[c][:], dtype=np.int16), info.sample_count)
                ch.Gain = int(info.gain[c])
                ch.StartContext = GcAdpcmContext(*info.start_context[c][:])
                if info.looping:
                    ch.LoopContext = GcAdpcmContext(*info.loop_context[c][:])
                    ch.LoopContextStart = info.loop_start
                chans.append(ch)
            return _stored_format(chans, info.sample_rate, info.looping, info.loop_start, info.sample_count, None)
        if info.codec == NwCodec.Pcm16Bit:                       # ToShortArray(structure.Endianness)
            order = ">i2" if info.endianness == 1 else "<i2"
            fmt = Pcm16Format([r.view(order).astype(np.int16) for r in rows], info.sample_rate)
        else:
            fmt = Pcm8SignedFormat(rows, info.sample_rate)
        fmt.WithLoop(bool(info.looping), info.loop_start, info.sample_count)
        return fmt


class BrwavReader(_NwWaveReader):
    """BrwavReader.cs"""
    magics = (b"RWAV",)


class BCFwavReader(_NwWaveReader):
    """BCFstmReader.cs for what is not a stream: wave files (CWAV, FWAV) and prefetch files (CSTP, FSTP)"""
    magics = (b"CWAV", b"FWAV", b"CSTP", b"FSTP")


class NwWaveBank:
    """vga_nwwav_bank over a list of file images: the images are packed into one device buffer (each at a multiple of
    `align` bytes, 1 = back to back), and read() / decode_to_pcm16() run on the current torch stream."""

    def __init__(self, images, align=1):
        import torch
        self.images = [bytes(i) for i in images]
        n = len(self.images)
        self.infos = (_lib.NwWavInfoC * max(n, 1))()
        for f, img in enumerate(self.images):
            buf = np.frombuffer(img, dtype=np.uint8)
            check(_lib.lib().vga_nwwav_parse(buf.ctypes.data_as(u8p) if len(buf) else None, len(buf), C.byref(self.infos[f])))
        self.file_offsets = np.zeros(max(n, 1), dtype=np.int64)
        at = 0
        for f, img in enumerate(self.images):
            at = -(-at // align) * align
            self.file_offsets[f] = at
            at += len(img)
        self._h = C.c_void_p()
        check(_lib.lib().vga_nwwav_bank_create(self.infos, self.file_offsets.ctypes.data_as(C.POINTER(C.c_int64)), n, C.byref(self._h)))
        L = _lib.lib()
        host = np.zeros(max(at, 16), dtype=np.uint8)
        for f, img in enumerate(self.images):
            host[self.file_offsets[f]:self.file_offsets[f] + len(img)] = np.frombuffer(img, dtype=np.uint8)
        assert L.vga_nwwav_bank_source_bytes(self._h) <= at
        self.d_files = torch.from_numpy(host).cuda()
        self.channels = L.vga_nwwav_bank_channels(self._h)
        ints = lambda: np.zeros(max(self.channels, 1), dtype=np.int32)
        self.file, self.channel, self.codec, self.sample_counts = ints(), ints(), ints(), ints()
        self.offsets = np.zeros(max(self.channels, 1), dtype=np.int64)
        ip = C.POINTER(C.c_int)
        check(L.vga_nwwav_bank_rows(self._h, *(a.ctypes.data_as(ip) for a in (self.file, self.channel, self.codec, self.sample_counts)),
                                    self.offsets.ctypes.data_as(C.POINTER(C.c_int64))))
        for name in ("file", "channel", "codec", "sample_counts", "offsets"):
            setattr(self, name, getattr(self, name)[:self.channels])
        self.gc_channels = L.vga_nwwav_bank_codec_channels(self._h, NwCodec.GcAdpcm)
        g = max(self.gc_channels, 1)
        self.gc_sample_counts = np.zeros(g, dtype=np.int32)
        if self.gc_channels:
            check(L.vga_nwwav_bank_gc_sample_counts(self._h, self.gc_sample_counts.ctypes.data_as(ip)))
        self.gc_coefs, self.gc_hist1, self.gc_hist2 = np.zeros((g, 16), np.int16), np.zeros(g, np.int16), np.zeros(g, np.int16)
        self.gc_gain = np.zeros(g, np.int16)
        check(L.vga_nwwav_bank_gc_tables(self._h, *(a.ctypes.data_as(i16p) for a in (self.gc_coefs, self.gc_hist1, self.gc_hist2, self.gc_gain))))
        self.adpcm_bytes = L.vga_nwwav_bank_adpcm_bytes(self._h)
        self.pcm16_samples = L.vga_nwwav_bank_pcm16_samples(self._h)
        self.pcm8_bytes = L.vga_nwwav_bank_pcm8_bytes(self._h)

    def close(self):
        if self._h:
            _lib.lib().vga_nwwav_bank_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()

    def read(self):
        """vga_nwwav_bank_read_device -> (d_adpcm uint8, d_pcm16 int16, d_pcm8 uint8) device tensors, packed"""
        import torch
        outs = (torch.empty(self.adpcm_bytes, dtype=torch.uint8, device="cuda"),
                torch.empty(self.pcm16_samples, dtype=torch.int16, device="cuda"),
                torch.empty(self.pcm8_bytes, dtype=torch.uint8, device="cuda"))
        ptr = lambda t: t.data_ptr() if t.numel() else None
        check(_lib.lib().vga_nwwav_bank_read_device(self._h, self.d_files.data_ptr(), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]),
                                                    torch.cuda.current_stream().cuda_stream))
        return outs

    def decode_to_pcm16(self):
        """bank read, then vga_gcadpcm_decode_device_v on the GC-ADPCM rows and Pcm8Codec.DecodeSigned on the PCM8 rows:
        -> per file, a list of its channels' int16 samples (host arrays)"""
        import torch
        L = _lib.lib()
        stream = torch.cuda.current_stream().cuda_stream
        d_adpcm, d_pcm16, d_pcm8 = self.read()
        gc_pcm = pcm8_as16 = gc_off = None
        if self.gc_channels:
            ragged = C.c_void_p()
            check(L.vga_gcadpcm_ragged_create(self.gc_sample_counts.ctypes.data_as(C.POINTER(C.c_int)), self.gc_channels, C.byref(ragged)))
            try:
                assert L.vga_gcadpcm_ragged_adpcm_bytes(ragged) == self.adpcm_bytes
                gc_off = np.zeros(self.gc_channels, dtype=np.int64)
                check(L.vga_gcadpcm_ragged_offsets(ragged, gc_off.ctypes.data_as(C.POINTER(C.c_int64)), None))
                d_gc = torch.zeros(L.vga_gcadpcm_ragged_pcm_samples(ragged), dtype=torch.int16, device="cuda")
                d_status = torch.zeros(4, dtype=torch.int32, device="cuda")
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                d_coefs, d_h1, d_h2 = up(self.gc_coefs), up(self.gc_hist1), up(self.gc_hist2)
                check(L.vga_gcadpcm_decode_device_v(ragged, d_adpcm.data_ptr(), d_coefs.data_ptr(), d_h1.data_ptr(), d_h2.data_ptr(),
                                                    d_gc.data_ptr(), d_status.data_ptr(), stream))
                gc_pcm = d_gc.cpu().numpy()
                if int(d_status[0]):
                    raise _lib.ArgumentError("a GC-ADPCM frame header names a predictor above 7")
            finally:
                L.vga_gcadpcm_ragged_destroy(ragged)
        if self.pcm8_bytes:                                      # the packed buffer as one row: the offsets carry over
            d_8 = torch.empty(self.pcm8_bytes, dtype=torch.int16, device="cuda")
            check(L.vga_pcm8_decode_device(d_pcm8.data_ptr(), self.pcm8_bytes, self.pcm8_bytes, 1, 1, d_8.data_ptr(), self.pcm8_bytes, stream))
            pcm8_as16 = d_8.cpu().numpy()
        pcm16 = d_pcm16.cpu().numpy()
        out = [[] for _ in self.images]
        g = 0
        for r in range(self.channels):
            n, at = int(self.sample_counts[r]), int(self.offsets[r])
            if self.codec[r] == NwCodec.GcAdpcm:
                src, at = gc_pcm, int(gc_off[g])
                g += 1
            else:
                src = pcm16 if self.codec[r] == NwCodec.Pcm16Bit else pcm8_as16
            out[int(self.file[r])].append(src[at:at + n].copy() if n else np.zeros(0, dtype=np.int16))
        return out
