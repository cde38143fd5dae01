"""PCM8 / PCM16 BRSTM, BCSTM and BFSTM on the GPU: the reference suite's *BuildAndParseEqualPcm16 / Pcm8 cases
(VGAudio.Tests/Containers/{Brstm,Bcstm,Bfstm}Tests.cs) against the byte-for-byte restatement in nwstm_pcm_ref.py,
batched device calls against single-file host calls, every granule size, the busy-stream rule and codec chains."""
import ctypes as C

import numpy as np
import pytest

import nwstm_pcm_ref as ref
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AudioTrack, GcAdpcmFormat, Pcm16Format
from vgaudio_amd.nwstm import (BCFstmReader, BCFstmWriter, BrstmReader, BrstmWriter, BxstmConfiguration, NwCodec,
                               NwTarget, parse_pcm)
from vgaudio_amd.pcm8 import Pcm8SignedFormat

pytestmark = pytest.mark.gpu

S16, BYTES = 0, 1
TARGETS = {"Brstm": NwTarget.Revolution, "Bcstm": NwTarget.Ctr, "Bfstm": NwTarget.Cafe}


def _torch():
    import torch
    return torch


def _writer(target, cfg):
    return BrstmWriter(cfg) if target == NwTarget.Revolution else BCFstmWriter(target, cfg)


def _reader(target):
    return BrstmReader() if target == NwTarget.Revolution else BCFstmReader()


def _pcm16(nch, n, seed=0):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return [((np.sin(t * (0.01 + 0.003 * c)) * 20000).astype(np.int32) + rng.integers(-3000, 3000, n)).clip(-32768, 32767)
            .astype(np.int16) for c in range(nch)]


def _stored_rows(codec, pcm):
    return pcm if codec == ref.PCM16 else [ref.encode_signed(r) for r in pcm]


@pytest.mark.parametrize("name", sorted(TARGETS))
@pytest.mark.parametrize("codec", [ref.PCM16, ref.PCM8])
@pytest.mark.parametrize("nch", [1, 2, 8])
def test_build_and_parse_equal(name, codec, nch):
    """{Brstm,Bcstm,Bfstm}BuildAndParseEqual{Pcm16,Pcm8}: from a Pcm16Format (PCM8 through EncodeSigned on the
    device) and from a Pcm8SignedFormat; the image equals the restatement, reading it back gives what was written"""
    target = TARGETS[name]
    pcm = _pcm16(nch, 20011, seed=nch)
    cfg = BxstmConfiguration(Codec=NwCodec(codec))
    fmt = Pcm16Format(pcm, 32000)
    img = _writer(target, cfg).GetFile(fmt)
    rows = _stored_rows(codec, pcm)
    assert img == ref.build_image(int(target), codec, 32000, rows)
    if codec == ref.PCM8:
        assert _writer(target, cfg).GetFile(Pcm8SignedFormat(rows, 32000)) == img
    back = _reader(target).ReadAnyFormat(img)
    parsed = ref.parse_image(img)
    if codec == ref.PCM16:
        assert isinstance(back, Pcm16Format)
        for a, b, c in zip(back.Channels, pcm, parsed["channels"]):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    else:
        assert isinstance(back, Pcm8SignedFormat)
        for a, b, c in zip(back.Channels, rows, parsed["channels"]):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert all(np.array_equal(a, ref.decode_signed(b)) for a, b in zip(back.ToPcm16().Channels, rows))
    assert back.SampleRate == 32000 and not back.Looping
    assert back.Tracks == AudioTrack.GetDefaultTrackList(nch)


@pytest.mark.parametrize("name", sorted(TARGETS))
@pytest.mark.parametrize("codec", [ref.PCM16, ref.PCM8])
def test_looping_truncates_at_loop_end(name, codec):
    target = TARGETS[name]
    pcm = _pcm16(3, 30000, seed=5)
    tracks = [AudioTrack(2, 0, 1, 0x70, 0x30), AudioTrack(1, 2, 0, 0x7f, 0x40)]
    fmt = Pcm16Format(pcm, 44100).WithLoop(True, 1234, 17777)
    fmt.Tracks = tracks
    cfg = BxstmConfiguration(Codec=NwCodec(codec), SamplesPerInterleave=1001 if codec == ref.PCM8 else 1000)
    img = _writer(target, cfg).GetFile(fmt)
    rows = _stored_rows(codec, pcm)
    expect = ref.build_image(int(target), codec, 44100, rows, True, 1234, 17777, spi=cfg.SamplesPerInterleave,
                             tracks=[dict(channel_count=t.ChannelCount, left=t.ChannelLeft, right=t.ChannelRight,
                                          volume=t.Volume, panning=t.Panning) for t in tracks])
    assert img == expect
    back = _reader(target).ReadAnyFormat(img)
    assert back.SampleCount == 17777 and back.Looping and (back.LoopStart, back.LoopEnd) == (1234, 17777)
    # BFSTM 0.3 (the default) carries no track info: the default list reads back
    assert back.Tracks == (AudioTrack.GetDefaultTrackList(3) if target == NwTarget.Cafe else tracks)
    for a, b in zip(back.Channels, rows):
        assert np.array_equal(a, b[:17777])


def _params(target, n, spi=0, looping=0):
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = int(target), 48000, n, -1
    p.samples_per_interleave = spi
    p.looping, p.loop_start, p.loop_end = looping, 10 if looping else 0, n - 7 if looping else 0
    return p


def _host_file(p, codec, rows, kind):
    L = _lib.NwLayoutC()
    assert _lib.lib().vga_nwstm_pcm_layout_for(C.byref(p), codec, len(rows), C.byref(L)) == 0
    out = np.zeros(L.file_size, dtype=np.uint8)
    ptrs = (C.c_void_p * len(rows))(*[r.ctypes.data for r in rows])
    assert _lib.lib().vga_nwstm_pcm_write(C.byref(p), codec, len(rows), None, ptrs, kind, out.ctypes.data_as(_lib.u8p)) == 0
    return out, L


@pytest.mark.parametrize("target", list(NwTarget))
@pytest.mark.parametrize("codec,kind", [(ref.PCM16, S16), (ref.PCM8, S16), (ref.PCM8, BYTES)])
def test_batched_device_calls_equal_single_file_calls(target, codec, kind):
    torch = _torch()
    nfiles, nch, n = 64, 2, 3001
    rng = np.random.default_rng(int(target) * 10 + codec)
    dtype = np.int16 if kind == S16 else np.uint8
    rows = (rng.integers(-32768, 32768, (nfiles * nch, n)) if kind == S16 else rng.integers(0, 256, (nfiles * nch, n))).astype(dtype)
    p = _params(target, n, spi=333 if codec == ref.PCM8 else 0, looping=1)
    singles = [_host_file(p, codec, [np.ascontiguousarray(rows[f * nch + c]) for c in range(nch)], kind)[0] for f in range(nfiles)]
    L = _host_file(p, codec, [np.ascontiguousarray(rows[c]) for c in range(nch)], kind)[1]
    pitch = n + 13
    d_rows = torch.zeros((nfiles * nch, pitch), dtype=torch.int16 if kind == S16 else torch.uint8, device="cuda")
    d_rows[:, :n] = torch.from_numpy(rows).cuda()
    fp = (L.file_size + 15) // 16 * 16 + 16
    d_files = torch.full((nfiles, fp), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().vga_nwstm_pcm_write_device(C.byref(p), codec, nch, nfiles, None, C.c_void_p(d_rows.data_ptr()), kind,
                                                 pitch, C.c_void_p(d_files.data_ptr()), fp, C.c_void_p(s)) == 0
    got = d_files.cpu().numpy()
    for f in range(nfiles):
        assert np.array_equal(got[f, :L.file_size], singles[f]), f
    info = parse_pcm(singles[0].tobytes())
    d_out = torch.full((nfiles * nch, pitch), 0x3C, dtype=d_rows.dtype, device="cuda")
    assert _lib.lib().vga_nwstm_pcm_read_device(C.byref(info), C.c_void_p(d_files.data_ptr()), fp, nfiles,
                                                C.c_void_p(d_out.data_ptr()), kind, pitch, C.c_void_p(s)) == 0
    back = d_out.cpu().numpy()[:, :info.sample_count]
    want = rows[:, :info.sample_count]
    if codec == ref.PCM8 and kind == S16:
        want = ref.decode_signed(ref.encode_signed(want))
    assert np.array_equal(back, want)
    # the host single-file read agrees
    outs = [np.zeros(info.sample_count, dtype=dtype) for _ in range(nch)]
    ptrs = (C.c_void_p * nch)(*[o.ctypes.data for o in outs])
    buf = singles[5]
    assert _lib.lib().vga_nwstm_pcm_read(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), ptrs, kind) == 0
    assert all(np.array_equal(outs[c], back[5 * nch + c]) for c in range(nch))


@pytest.mark.parametrize("codec,kind,big", [(ref.PCM16, S16, True), (ref.PCM16, S16, False), (ref.PCM8, S16, True),
                                            (ref.PCM8, BYTES, True)])
@pytest.mark.parametrize("shift", [0, 1, 2, 4, 8])
def test_every_granule_size(codec, kind, big, shift):
    """odd pitches, offsets and interleaves: from 16-byte granules down to the byte path"""
    torch = _torch()
    es = 2 if kind == S16 else 1
    nch, n = 3, 2000 + shift
    spi = {0: 256, 1: 255, 2: 258, 4: 260, 8: 264}[shift] if codec == ref.PCM8 else {0: 256, 1: 257, 2: 258, 4: 260, 8: 264}[shift]
    rng = np.random.default_rng(shift)
    rows = (rng.integers(-32768, 32768, (nch, n)) if kind == S16 else rng.integers(0, 256, (nch, n))).astype(np.int16 if es == 2 else np.uint8)
    p = _params(NwTarget.Cafe, n, spi=spi)
    p.endianness = int(big)
    want, L = _host_file(p, codec, [np.ascontiguousarray(r) for r in rows], kind)
    assert want.tobytes() == ref.build_image(2, codec, 48000, [ref.encode_signed(r) if (codec == ref.PCM8 and kind == S16) else r
                                                                for r in rows], spi=spi, big=big)
    pitch = n + (shift or 16)
    base = torch.zeros(nch * pitch * es + 64, dtype=torch.uint8, device="cuda")
    off = shift * es                                        # a row start that is only shift-aligned
    view = base[off:off + nch * pitch * es]
    host = np.zeros((nch, pitch), dtype=rows.dtype)
    host[:, :n] = rows
    view.copy_(torch.from_numpy(host.view(np.uint8).reshape(-1)).cuda())
    fbuf = torch.full((L.file_size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().vga_nwstm_pcm_write_device(C.byref(p), codec, nch, 1, None, C.c_void_p(view.data_ptr()), kind, pitch,
                                                 C.c_void_p(fbuf.data_ptr() + shift), L.file_size, C.c_void_p(s)) == 0
    assert np.array_equal(fbuf.cpu().numpy()[shift:shift + L.file_size], want)
    info = parse_pcm(want.tobytes())
    obuf = torch.full((nch * pitch * es + 64,), 0x3C, dtype=torch.uint8, device="cuda")
    assert _lib.lib().vga_nwstm_pcm_read_device(C.byref(info), C.c_void_p(fbuf.data_ptr() + shift), L.file_size, 1,
                                                C.c_void_p(obuf.data_ptr() + off), kind, pitch, C.c_void_p(s)) == 0
    got = obuf.cpu().numpy()[off:off + nch * pitch * es].view(rows.dtype).reshape(nch, pitch)[:, :n]
    expect = ref.decode_signed(ref.encode_signed(rows)) if (codec == ref.PCM8 and kind == S16) else rows
    assert np.array_equal(got, expect)


def test_codec_chains():
    """GC-ADPCM BRSTM -> read -> decode -> PCM16 BFSTM -> read equals the decoded PCM; PCM16 BCSTM -> read ->
    GC-ADPCM encode -> BRSTM equals the GC path on the same PCM"""
    pcm = Pcm16Format(_pcm16(2, 40000, seed=9), 48000)
    gc = BrstmWriter().GetFile(GcAdpcmFormat().EncodeFromPcm16(pcm))
    decoded = BrstmReader().ReadFormat(gc).ToPcm16()
    bfstm = BCFstmWriter(NwTarget.Cafe, BxstmConfiguration(Codec=NwCodec.Pcm16Bit)).GetFile(decoded)
    again = BCFstmReader().ReadAnyFormat(bfstm)
    assert all(np.array_equal(a, b) for a, b in zip(again.Channels, decoded.Channels))
    assert isinstance(BrstmReader().ReadAnyFormat(gc), GcAdpcmFormat)
    bcstm = BCFstmWriter(NwTarget.Ctr, BxstmConfiguration(Codec=NwCodec.Pcm16Bit)).GetFile(pcm)
    via = BrstmWriter().GetFile(GcAdpcmFormat().EncodeFromPcm16(BCFstmReader().ReadAnyFormat(bcstm)))
    assert via == gc

