"""BRSTM / BCSTM / BFSTM on the GPU: images equal the restatement in nwstm_ref.py byte for byte, the readers return
what was written, and the batched device path (encode -> build -> write -> read -> decode, all in HBM) equals the
host single-file calls."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import nwstm_ref as ref
from vgaudio_amd import _lib, device as dev, synth
from vgaudio_amd.gcadpcm import AudioTrack, GcAdpcmFormat, Pcm16Format
from vgaudio_amd.nwstm import (BCFstmReader, BCFstmWriter, BrstmReader, BrstmSeekTableType, BrstmTrackType, BrstmWriter,
                               BxstmConfiguration, Endianness, NwTarget, NwVersion)

pytestmark = pytest.mark.gpu

TARGETS = [NwTarget.Revolution, NwTarget.Ctr, NwTarget.Cafe]


def writer(target, cfg=None):
    return BrstmWriter(cfg) if target == NwTarget.Revolution else BCFstmWriter(target, cfg)


def reader(target):
    return BrstmReader() if target == NwTarget.Revolution else BCFstmReader()


def sine_format(nch, n, looping=False, loop_start=0, loop_end=0):
    """GenerateAdpcmSineWave: one sine per channel, encoded"""
    pcm = Pcm16Format([synth.sine(n, 200.0 + 150.0 * c) for c in range(nch)], 48000)
    fmt = GcAdpcmFormat().EncodeFromPcm16(pcm)
    return fmt.WithLoop(True, loop_start, loop_end) if looping else fmt


def expected_image(target, fmt, cfg):
    """the restatement's bytes for what the writer builds from `fmt`"""
    w = writer(target, cfg)
    L = w.Layout(fmt)
    built = fmt._clone(alignmentMultiple=L.channel.loop_alignment_multiple,
                       samplesPerSeekTableEntry=L.channel.samples_per_seek_table_entry)
    ch = built.Channels
    version = None if cfg.Version is None else cfg.Version.Version
    big = None if cfg.Endianness is None else cfg.Endianness == Endianness.BigEndian
    tracks = [dict(channel_count=t.ChannelCount, left=t.ChannelLeft, right=t.ChannelRight, volume=t.Volume,
                   panning=t.Panning) for t in built.Tracks]
    img = ref.build_image(int(target), built.SampleRate, len(ch), [c.GetAdpcmAudio().tobytes() for c in ch],
                          [c.Coefs.tolist() for c in ch], [c.Gain for c in ch],
                          [[c.StartContext.PredScale, c.StartContext.Hist1, c.StartContext.Hist2] for c in ch],
                          [[c.LoopContext.PredScale, c.LoopContext.Hist1, c.LoopContext.Hist2] for c in ch],
                          [c.GetSeekTable().tolist() for c in ch], built.Looping, built.LoopStart, built.LoopEnd,
                          built.SampleCount, spi=cfg.SamplesPerInterleave, spe=cfg.SamplesPerSeekTableEntry,
                          track_short=cfg.TrackType == BrstmTrackType.Short,
                          seek_short=cfg.SeekTableType == BrstmSeekTableType.Short, version=version, big=big,
                          tracks=tracks)
    return img, built


def check_read_back(target, img, built, cfg=None):
    got = reader(target).ReadFormat(img)
    # entries the file holds; BrstmReader may read more when both ADPC sizes round alike (the rest is padding)
    stored = writer(target, cfg or BxstmConfiguration()).Layout(built).seek_table_entry_count
    assert got.ChannelCount == built.ChannelCount and got.SampleRate == built.SampleRate
    assert (got.Looping, got.LoopStart) == (built.Looping, built.LoopStart)
    sc = built.LoopEnd if built.Looping else built.SampleCount
    assert got.Channels[0].SampleCount == sc
    if built.Looping:
        assert got.LoopEnd == built.LoopEnd
    assert got.Tracks == built.Tracks
    nb = ref.bytes_of(sc)
    R = ref.parse_image(img)
    for c, (g, b) in enumerate(zip(got.Channels, built.Channels)):
        assert np.array_equal(g.GetAdpcmAudio(), b.GetAdpcmAudio()[:nb])
        assert g.GetAdpcmAudio().tobytes() == R["audio"][c]
        assert np.array_equal(g.Coefs, b.Coefs)
        assert vars(g.StartContext) == vars(b.StartContext)
        if built.Looping:
            assert vars(g.LoopContext) == vars(b.LoopContext)
        seek = b.GetSeekTable()
        k = min(len(seek), len(g.GetSeekTable()), 2 * stored)
        assert np.array_equal(g.GetSeekTable()[:k], seek[:k])
        if target == NwTarget.Revolution:
            assert g.Gain == b.Gain
    return got


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("nch", [1, 2, 8])
def test_build_and_parse_equal(target, nch):
    cfg = BxstmConfiguration()
    fmt = sine_format(nch, 40000)
    img = writer(target, cfg).GetFile(fmt)
    want, built = expected_image(target, fmt, cfg)
    assert img == want
    check_read_back(target, img, built, cfg)


@pytest.mark.parametrize("target", TARGETS)
def test_loop_alignment_is_set(target):
    cfg = BxstmConfiguration(LoopPointAlignment=700)
    fmt = sine_format(2, 20000, True, 1288, 16288)
    img = writer(target, cfg).GetFile(fmt)
    want, built = expected_image(target, fmt, cfg)
    assert img == want
    got = check_read_back(target, img, built, cfg)
    assert (got.LoopStart, got.LoopEnd) == (1400, 16400)


GRID = [
    dict(SamplesPerInterleave=14, SamplesPerSeekTableEntry=2, LoopPointAlignment=14),
    dict(SamplesPerInterleave=14 * 64, SamplesPerSeekTableEntry=100, TrackType=BrstmTrackType.Short, LoopPointAlignment=700),
    dict(SamplesPerInterleave=14336, SamplesPerSeekTableEntry=14336, SeekTableType=BrstmSeekTableType.Short,
         LoopPointAlignment=2800),
    dict(SamplesPerInterleave=14 * 64, SamplesPerSeekTableEntry=100, LoopPointAlignment=1000),
]
LOOPS = [None, (0, 9000), (2800, 9001), (1234, 8000)]


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("g", range(len(GRID)))
def test_geometry_grid(target, g):
    for n in (1, 13, 14 * 64 * 2, 9001):
        for loop in LOOPS:
            if loop is not None and loop[1] > n:
                continue
            kw = dict(GRID[g])
            if target != NwTarget.Revolution:
                kw.pop("TrackType", None)
                kw.pop("SeekTableType", None)
            cfg = BxstmConfiguration(**kw)
            fmt = sine_format(3, n, loop is not None, *(loop or (0, 0)))
            img = writer(target, cfg).GetFile(fmt)
            want, built = expected_image(target, fmt, cfg)
            assert img == want, (n, loop, kw)
            check_read_back(target, img, built, cfg)


@pytest.mark.parametrize("target,version,endian", [
    (NwTarget.Ctr, NwVersion(2, 0), None), (NwTarget.Ctr, NwVersion(2, 2), Endianness.BigEndian),
    (NwTarget.Ctr, NwVersion(2, 3), None), (NwTarget.Cafe, NwVersion(0, 2), None),
    (NwTarget.Cafe, NwVersion(0, 4), Endianness.LittleEndian), (NwTarget.Cafe, NwVersion(0, 5), None)])
def test_versions_and_endianness(target, version, endian):
    cfg = BxstmConfiguration(Version=version, Endianness=endian)
    fmt = sine_format(3, 30000, True, 1000, 25000)
    img = writer(target, cfg).GetFile(fmt)
    want, built = expected_image(target, fmt, cfg)
    assert img == want
    check_read_back(target, img, built, cfg)


def test_custom_tracks():
    fmt = sine_format(4, 5000)
    fmt.Tracks = [AudioTrack(2, 3, 1, 10, 20), AudioTrack(1, 0, 0, 0x7f, 0x40), AudioTrack(1, 2, 0, 5, 6)]
    for target in TARGETS:
        cfg = BxstmConfiguration()
        img = writer(target, cfg).GetFile(fmt)
        want, built = expected_image(target, fmt, cfg)
        assert img == want
        got = reader(target).ReadFormat(img)
        if target != NwTarget.Cafe:                 # BFSTM 0.3 carries no track info
            assert got.Tracks == fmt.Tracks


def _device_pipeline(nfiles, nch, n, looping, loop_start, loop_end, target, cfg_kw):
    """synth -> coefs -> encode -> build channels -> write images, all device-resident"""
    L = _lib.lib()
    d = torch.device("cuda:0")
    rows = nfiles * nch
    pcm = dev.synth_pcm(rows, n, d)
    coefs = dev.gc_coefs(pcm, n)
    adpcm = dev.gc_encode(pcm, n, coefs)
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = int(target), 44100, n, -1
    p.looping, p.loop_start, p.loop_end = int(looping), loop_start, loop_end
    for k, v in cfg_kw.items():
        setattr(p, k, v)
    lay = _lib.NwLayoutC()
    _lib.check(L.vga_nwstm_layout_for(C.byref(p), nch, C.byref(lay)))
    cp = lay.channel
    out = dev.alloc_adpcm(rows, lay.channel_sample_count, d)
    ne = lay.channel_seek_entries
    seek = torch.zeros((rows, max(2 * ne, 8)), dtype=torch.int16, device=d)
    ctx = torch.zeros((rows, 3), dtype=torch.int16, device=d)
    wsb = L.vga_gcadpcm_build_channels_workspace_bytes(rows, C.byref(cp))
    ws = torch.empty(wsb, dtype=torch.uint8, device=d)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.vga_gcadpcm_build_channels_device(adpcm.data_ptr(), adpcm.stride(0), coefs.data_ptr(), rows, C.byref(cp),
                                                   out.data_ptr(), out.stride(0), None, 0, seek.data_ptr(), seek.stride(0),
                                                   ctx.data_ptr(), ws.data_ptr(), wsb, st))
    fpitch = (lay.file_size + 15) // 16 * 16 + 16
    files = torch.full((nfiles, fpitch), 0xAB, dtype=torch.uint8, device=d)
    _lib.check(L.vga_nwstm_write_device(C.byref(p), nch, nfiles, None, out.data_ptr(), out.stride(0), lay.channel_adpcm_bytes,
                                        coefs.data_ptr(), None, None, ctx.data_ptr(), seek.data_ptr(), seek.stride(0), ne,
                                        files.data_ptr(), fpitch, st))
    torch.cuda.synchronize()
    return p, lay, files, out, coefs, seek, ctx


@pytest.mark.parametrize("target", TARGETS)
@pytest.mark.parametrize("nfiles,nch,n,loop", [(1, 2, 30000, None), (7, 2, 48000, (1288, 40000)), (64, 1, 5001, None),
                                               (16, 3, 20000, (0, 20000)), (5, 2, 14 * 64 * 3, None)])
def test_batched_device_write_equals_host_and_reads_back(target, nfiles, nch, n, loop):
    cfg = dict(samples_per_interleave=14 * 64, loop_point_alignment=700) if nfiles == 7 else {}
    p, lay, files, out, coefs, seek, ctx = _device_pipeline(nfiles, nch, n, loop is not None, *(loop or (0, 0)), target, cfg)
    L = _lib.lib()
    fh = files.cpu().numpy()
    nb, ne = lay.channel_adpcm_bytes, lay.channel_seek_entries
    a_h, c_h, s_h, x_h = out.cpu().numpy(), coefs.cpu().numpy(), seek.cpu().numpy(), ctx.cpu().numpy()
    for f in range(nfiles):
        rows = range(f * nch, f * nch + nch)
        adpcm = [np.ascontiguousarray(a_h[r, :nb]) for r in rows]
        sk = [np.ascontiguousarray(s_h[r, :2 * ne]) for r in rows]
        img = np.zeros(lay.file_size, dtype=np.uint8)
        _lib.check(L.vga_nwstm_write(C.byref(p), nch, None, (_lib.u8p * nch)(*[a.ctypes.data_as(_lib.u8p) for a in adpcm]), nb,
                                     np.ascontiguousarray(c_h[f * nch:f * nch + nch]).ctypes.data_as(_lib.i16p), None, None,
                                     np.ascontiguousarray(x_h[f * nch:f * nch + nch]).ctypes.data_as(_lib.i16p),
                                     (_lib.i16p * nch)(*[s.ctypes.data_as(_lib.i16p) for s in sk]) if ne else None, ne,
                                     img.ctypes.data_as(_lib.u8p)))
        assert np.array_equal(fh[f, :lay.file_size], img), f
        assert (fh[f, lay.file_size:] == 0xAB).all()          # nothing written past the image
        start = [[int(a[0]) if nb else 0, 0, 0] for a in adpcm]
        loopc = [x_h[r].tolist() for r in rows]
        want = ref.build_image(int(target), 44100, nch, [a.tobytes() for a in adpcm], c_h[f * nch:f * nch + nch].tolist(),
                               [0] * nch, start, loopc, [s.tolist() for s in sk], lay.looping, lay.loop_start, lay.loop_end,
                               lay.sample_count, spi=lay.samples_per_interleave, spe=lay.samples_per_seek_table_entry,
                               version=lay.version if target != NwTarget.Revolution else None)
        assert img.tobytes() == want, f
    # read every image back on the device and decode: the PCM of the written channels
    info = _lib.NwInfoC()
    one = np.ascontiguousarray(fh[0, :lay.file_size])
    _lib.check(L.vga_nwstm_parse(one.ctypes.data_as(_lib.u8p), lay.file_size, C.byref(info)))
    back = dev.alloc_adpcm(nfiles * nch, info.sample_count, files.device)
    _lib.check(L.vga_nwstm_read_device(C.byref(info), files.data_ptr(), files.stride(0), nfiles, back.data_ptr(), back.stride(0),
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    ab = info.adpcm_bytes
    assert torch.equal(back[:, :ab], out[:, :ab])
    pcm_back, status = dev.gc_decode(back, coefs, info.sample_count)
    pcm_ref, _ = dev.gc_decode(out, coefs, info.sample_count)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(pcm_back[:, :info.sample_count], pcm_ref[:, :info.sample_count])


def test_read_then_decode_equals_pcm_of_written_channels():
    fmt = sine_format(2, 33333, True, 5000, 30000)
    for target in TARGETS:
        cfg = BxstmConfiguration(LoopPointAlignment=1000)
        img = writer(target, cfg).GetFile(fmt)
        _, built = expected_image(target, fmt, cfg)
        got = reader(target).ReadFormat(img)
        for g, b in zip(got.Channels, built.Channels):
            n = g.SampleCount
            assert np.array_equal(g.GetPcmAudio(), b.GetPcmAudio()[:n])


def test_brstm_to_bfstm_round_trip_keeps_audio():
    fmt = sine_format(2, 25000, True, 14336, 24000)
    a = BrstmWriter().GetFile(fmt)
    f1 = BrstmReader().ReadFormat(a)
    b = BCFstmWriter(NwTarget.Cafe).GetFile(f1)
    f2 = BCFstmReader().ReadFormat(b)
    assert (f2.Looping, f2.LoopStart, f2.LoopEnd) == (f1.Looping, f1.LoopStart, f1.LoopEnd)
    for x, y in zip(f1.Channels, f2.Channels):
        assert np.array_equal(x.GetAdpcmAudio(), y.GetAdpcmAudio())
        assert np.array_equal(x.GetPcmAudio(), y.GetPcmAudio())


def test_random_sweep_against_restatement():
    rng = random.Random(2026)
    for _ in range(12):
        target = rng.choice(TARGETS)
        nch = rng.choice([1, 2, 3, 6])
        n = rng.randint(1, 60000)
        loop = None
        if rng.random() < 0.5 and n > 20:
            s = rng.randint(0, n - 10)
            loop = (s, rng.randint(s + 5, n))
        kw = dict(SamplesPerInterleave=14 * rng.randint(1, 1200), SamplesPerSeekTableEntry=rng.randint(2, 20000),
                  LoopPointAlignment=rng.choice([1, 14, 700, 14336]))
        if target == NwTarget.Revolution:
            kw.update(TrackType=rng.choice(list(BrstmTrackType)), SeekTableType=rng.choice(list(BrstmSeekTableType)))
        cfg = BxstmConfiguration(**kw)
        fmt = sine_format(nch, n, loop is not None, *(loop or (0, 0)))
        try:
            img = writer(target, cfg).GetFile(fmt)
        except _lib.VgaError:
            continue                                 # zero-length loops the reference cannot align, and the like
        want, built = expected_image(target, fmt, cfg)
        assert img == want, (target, nch, n, loop, kw)
        check_read_back(target, img, built, cfg)
