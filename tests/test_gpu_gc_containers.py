"""HPS, IDSP and GENH on the GPU: images equal the restatement in gc_containers_ref.py byte for byte (the HPS block
contexts under each of the reference's Pcm provenances), the readers return what was written, batched device calls
equal single-file host calls, and conversions between containers keep the audio bit for bit."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import gc_containers_ref as ref
from vgaudio_amd import _lib, synth
from vgaudio_amd.dsp import DspReader, DspWriter
from vgaudio_amd.gcadpcm import GcAdpcmFormat, Pcm16Format
from vgaudio_amd.genh import GenhReader
from vgaudio_amd.hps import HpsReader, HpsWriter
from vgaudio_amd.idsp import IdspConfiguration, IdspReader, IdspWriter
from vgaudio_amd.nwstm import BCFstmReader, BCFstmWriter, NwTarget

pytestmark = pytest.mark.gpu

SAMPLES = 48000                                   # BuildParseTestOptions.Samples


def st():
    return torch.cuda.current_stream().cuda_stream


def sine_format(nch, n=SAMPLES, looping=False, ls=0, le=0):
    """GenerateAdpcmSineWave, optionally re-looped (AudioFormatBase.WithLoop)"""
    pcm = Pcm16Format([synth.sine(n, 200.0 + 150.0 * c) for c in range(nch)], 48000)
    fmt = GcAdpcmFormat().EncodeFromPcm16(pcm)
    return fmt.WithLoop(True, ls, le) if looping else fmt


def ctx(ch, attr):
    c = getattr(ch, attr)
    return [c.PredScale, c.Hist1, c.Hist2]


def expected_hps(fmt, hist):
    L = HpsWriter().Layout(fmt)
    built = fmt._clone(alignmentMultiple=L.channel.loop_alignment_multiple)
    return ref.hps_image(fmt.SampleRate, [c.GetAdpcmAudio().tobytes() for c in built.Channels], [c.Coefs.tolist() for c in built.Channels],
                         [c.Gain for c in fmt.Channels], [ctx(c, "StartContext") for c in fmt.Channels], hist, fmt.Looping,
                         fmt.UnalignedLoopStart, fmt.UnalignedLoopEnd, fmt.UnalignedSampleCount), built


def compare_audio(got, fmt):
    """BuildParseTests.BuildParseCompareAudio: the decoded audio and the loop equal"""
    a, b = got.ToPcm16(), fmt.ToPcm16()
    assert (got.Looping, got.LoopStart, got.SampleCount) == (fmt.Looping, fmt.LoopStart, fmt.SampleCount)
    for x, y in zip(a.Channels, b.Channels):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- HPS
@pytest.mark.parametrize("nch", [1, 2, 8])
def test_hps_build_and_parse_equal(nch):
    fmt = sine_format(nch)
    img = HpsWriter().GetFile(fmt)
    want, built = expected_hps(fmt, fmt.ToPcm16().Channels)        # no alignment: the decoded audio
    assert img == want
    compare_audio(HpsReader().ReadFormat(img), fmt)


@pytest.mark.parametrize("nch", [1, 2, 8])
@pytest.mark.parametrize("ls", [0, 114688])        # a multiple of every alignment here
def test_hps_aligned_loops(nch, ls):
    n = 300000
    fmt = sine_format(nch, n, True, ls, n)
    L = HpsWriter().Layout(fmt)
    assert not L.alignment_needed
    img = HpsWriter().GetFile(fmt)
    want, built = expected_hps(fmt, fmt.ToPcm16().Channels)
    assert img == want
    got = HpsReader().ReadFormat(img)
    compare_audio(got, fmt)
    for g, b in zip(got.Channels, built.Channels):                  # the loop block's header context
        if ls:
            assert ctx(g, "LoopContext") == ctx(b, "LoopContext")


@pytest.mark.parametrize("nch", [1, 2, 8])
def test_hps_unaligned_loop_from_pcm_uses_the_unaligned_decode(nch):
    n = 200000
    fmt = sine_format(nch, n, True, 1234, 100000)     # the aligned blocks still start inside the unaligned decode
    L = HpsWriter().Layout(fmt)
    assert L.alignment_needed
    unaligned = [c._pcm for c in fmt.Channels]                      # WithLoop decoded the unaligned audio for its context
    assert all(u is not None and len(u) == n for u in unaligned)
    img = HpsWriter().GetFile(fmt)
    want, built = expected_hps(fmt, unaligned)
    assert img == want
    aligned = fmt.WithAlignment(L.alignment)
    got = HpsReader().ReadFormat(img)
    compare_audio(got, aligned)
    # the block hist values differ from the aligned decode once past the loop
    zeros, _ = expected_hps(fmt, None)
    assert img != zeros


def test_hps_unaligned_loop_read_from_dsp_writes_zero_hist():
    n = 200000
    fmt = sine_format(2, n, True, 1234, 190000)
    from_dsp = DspReader().ReadFormat(DspWriter().GetFile(fmt))
    assert all(c.Pcm is None for c in from_dsp.Channels)            # the stored loop context needed no decode
    img = HpsWriter().GetFile(from_dsp)
    want, _ = expected_hps(from_dsp, None)
    assert img == want
    compare_audio(HpsReader().ReadFormat(img), from_dsp.WithAlignment(HpsWriter().Layout(from_dsp).alignment))


def test_hps_hist_index_past_the_pcm_is_out_of_range():
    # aligned sample count past the unaligned decode: the reference's GetHist throws IndexOutOfRangeException
    fmt = sine_format(1, 130000, True, 1234, 130000)     # aligned loop start 114688: still inside the original data
    L = HpsWriter().Layout(fmt)
    blocks = HpsWriter().BlockMap(fmt)
    assert L.alignment_needed and blocks[-1].start_sample - 1 >= 130000
    with pytest.raises(_lib.ArgumentOutOfRangeError):
        HpsWriter().GetFile(fmt)
    with pytest.raises(ref.CannotWrite):
        expected_hps(fmt, [c._pcm for c in fmt.Channels])


def _device_rows(rows, nf):
    nb = len(rows[0])
    pitch = (nb + 15) // 16 * 16
    t = torch.zeros((nf * len(rows), pitch), dtype=torch.uint8, device="cuda")
    for f in range(nf):
        for c, r in enumerate(rows):
            t[f * len(rows) + c, :nb] = torch.from_numpy(np.frombuffer(bytes(r), np.uint8).copy())
    return t, pitch


def test_hps_batched_device_write_and_read_equal_single_calls():
    nch, nf = 2, 3
    fmt = sine_format(nch, 150000, True, 57344, 150000)
    w = HpsWriter()
    single = w.GetFile(fmt)
    L = w.Layout(fmt)
    built = fmt._clone(alignmentMultiple=L.channel.loop_alignment_multiple)
    adpcm, pitch = _device_rows([c.GetAdpcmAudio() for c in built.Channels], nf)
    pcm = torch.from_numpy(np.stack(fmt.ToPcm16().Channels * nf)).cuda()
    co = torch.from_numpy(np.stack([c.Coefs for c in built.Channels] * nf)).cuda()
    start = torch.from_numpy(np.array([ctx(c, "StartContext") for c in fmt.Channels] * nf, np.int16)).cuda()
    fp = (L.file_size + 255) // 256 * 256
    files = torch.full((nf, fp), 0xAB, dtype=torch.uint8, device="cuda")
    p = HpsWriter._params(fmt)
    _lib.check(_lib.lib().vga_hps_write_device(C.byref(p), nch, nf, adpcm.data_ptr(), pitch, L.channel_adpcm_bytes, co.data_ptr(),
                                               None, start.data_ptr(), pcm.data_ptr(), pcm.shape[1], pcm.shape[1],
                                               files.data_ptr(), fp, st()))
    host = files.cpu().numpy()
    for f in range(nf):
        assert host[f, :L.file_size].tobytes() == single
    from vgaudio_amd.hps import parse
    info, blocks = parse(single)
    back = torch.zeros((nf * nch, pitch), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vga_hps_read_device(C.byref(info), blocks, files.data_ptr(), fp, nf, back.data_ptr(), pitch, st()))
    got = HpsReader().ReadFormat(single)
    b = back.cpu().numpy()
    for f in range(nf):
        for c in range(nch):
            assert np.array_equal(b[f * nch + c, :info.adpcm_bytes], got.Channels[c].GetAdpcmAudio())


# ---------------------------------------------------------------- IDSP
def expected_idsp(fmt, cfg):
    w = IdspWriter(cfg)
    L = w.Layout(fmt)
    mult = L.channel.loop_alignment_multiple if cfg.BlockSize else fmt.AlignmentMultiple
    built = fmt._clone(alignmentMultiple=mult)
    return ref.idsp_image(fmt.SampleRate, [c.GetAdpcmAudio().tobytes() for c in built.Channels], [c.Coefs.tolist() for c in built.Channels],
                          [c.Gain for c in fmt.Channels], [ctx(c, "StartContext") for c in fmt.Channels],
                          [ctx(c, "LoopContext") for c in built.Channels], fmt.Looping, fmt.UnalignedLoopStart,
                          fmt.UnalignedLoopEnd, fmt.UnalignedSampleCount, cfg.BlockSize, cfg.TrimFile), built


@pytest.mark.parametrize("nch", [1, 2, 3, 8])
@pytest.mark.parametrize("block_size", [0, 0x10, 0x38, 0x800])
@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("loop", [None, (0, 40000), (1234, 40000)])
def test_idsp_images_equal_restatement(nch, block_size, trim, loop):
    fmt = sine_format(nch, SAMPLES, loop is not None, *(loop or (0, 0)))
    cfg = IdspConfiguration(BlockSize=block_size, TrimFile=trim)
    img = IdspWriter(cfg).GetFile(fmt)
    want, built = expected_idsp(fmt, cfg)
    assert img == want
    got, gcfg = IdspReader().ReadWithConfig(img)
    assert gcfg.BlockSize == block_size
    R = ref.idsp_parse(img)
    for c in range(nch):
        assert got.Channels[c].GetAdpcmAudio().tobytes() == R["audio"][c]


@pytest.mark.parametrize("nch", [1, 2, 8])
def test_idsp_build_and_parse_equal(nch):
    fmt = sine_format(nch)
    compare_audio(IdspReader().ReadFormat(IdspWriter().GetFile(fmt)), fmt)


@pytest.mark.parametrize("loops,start_in,end_in,start_out,end_out,block_size", [
    (True, 1234, 2000, 1260, 2026, 0x10),
    (True, 1248, 2014, 1260, 2026, 0x10),
    (True, 1234, 2000, 1274, 2040, 0x38),
    (True, 1274, 2040, 1274, 2040, 0x38),
    (False, 0, 0, 0, 0, 0x10),
])
def test_idsp_aligns_loop_to_block(loops, start_in, end_in, start_out, end_out, block_size):
    audio = sine_format(2)
    audio = audio.WithLoop(loops, start_in, end_in)
    idsp = IdspWriter().GetFile(audio, IdspConfiguration(BlockSize=block_size))
    decoded = IdspReader().ReadFormat(idsp)
    assert (decoded.LoopStart, decoded.LoopEnd) == (start_out, end_out)


def test_idsp_batched_device_write_and_read_equal_single_calls():
    nch, nf = 3, 4
    fmt = sine_format(nch, 30000, True, 1000, 29000)
    cfg = IdspConfiguration(BlockSize=0x38)
    w = IdspWriter(cfg)
    single = w.GetFile(fmt)
    L = w.Layout(fmt)
    built = fmt._clone(alignmentMultiple=L.channel.loop_alignment_multiple)
    adpcm, pitch = _device_rows([c.GetAdpcmAudio() for c in built.Channels], nf)
    co = torch.from_numpy(np.stack([c.Coefs for c in built.Channels] * nf)).cuda()
    start = torch.from_numpy(np.array([ctx(c, "StartContext") for c in fmt.Channels] * nf, np.int16)).cuda()
    loop = torch.from_numpy(np.array([ctx(c, "LoopContext") for c in built.Channels] * nf, np.int16)).cuda()
    fp = (L.file_size + 255) // 256 * 256
    files = torch.full((nf, fp), 0xAB, dtype=torch.uint8, device="cuda")
    p = w._params(fmt)
    _lib.check(_lib.lib().vga_idsp_write_device(C.byref(p), nch, nf, adpcm.data_ptr(), pitch, L.channel_adpcm_bytes, co.data_ptr(),
                                                None, start.data_ptr(), loop.data_ptr(), files.data_ptr(), fp, st()))
    host = files.cpu().numpy()
    for f in range(nf):
        assert host[f, :L.file_size].tobytes() == single
    from vgaudio_amd.idsp import parse
    info = parse(single)
    back = torch.zeros((nf * nch, pitch), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().vga_idsp_read_device(C.byref(info), files.data_ptr(), fp, nf, back.data_ptr(), pitch, st()))
    got = IdspReader().ReadFormat(single)
    b = back.cpu().numpy()
    for f in range(nf):
        for c in range(nch):
            assert np.array_equal(b[f * nch + c, :info.adpcm_bytes], got.Channels[c].GetAdpcmAudio())


# ---------------------------------------------------------------- GENH
@pytest.mark.parametrize("nch", [1, 2])
@pytest.mark.parametrize("coef_type", [0, 1, 2, 3])
@pytest.mark.parametrize("looping", [False, True])
@pytest.mark.parametrize("n", [20000, 19950])      # a ragged last block of 37 bytes per channel, and one of 8
def test_genh_reads_audio_and_coefficients(nch, coef_type, looping, n):
    fmt = sine_format(nch, n)
    rows = [c.GetAdpcmAudio().tobytes() for c in fmt.Channels]
    data = ref.genh_image(48000, rows, [c.Coefs.tolist() for c in fmt.Channels], 0x8000 if nch == 1 else 0x40,
                          1400 if looping else -1, n, coef_type)
    got = GenhReader().ReadFormat(data)
    assert (got.ChannelCount, got.SampleRate, got.Looping, got.SampleCount) == (nch, 48000, looping, n)
    if looping:
        assert (got.LoopStart, got.LoopEnd) == (1400, n)
    for g, f in zip(got.Channels, fmt.Channels):
        assert np.array_equal(g.GetAdpcmAudio(), f.GetAdpcmAudio()) and np.array_equal(g.Coefs, f.Coefs)
    for x, y in zip(got.ToPcm16().Channels, fmt.ToPcm16().Channels):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- conversions
def test_dsp_to_hps_to_bfstm_and_idsp_to_dsp_bit_for_bit():
    fmt = sine_format(2, 120000, True, 57344, 120000)
    dsp = DspReader().ReadFormat(DspWriter().GetFile(fmt))
    hps = HpsReader().ReadFormat(HpsWriter().GetFile(dsp))
    compare_audio(hps, fmt)
    bf = BCFstmReader().ReadFormat(BCFstmWriter(NwTarget.Cafe).GetFile(hps))
    for x, y in zip(bf.ToPcm16().Channels, fmt.ToPcm16().Channels):
        assert np.array_equal(x[:len(y)], y)
    idsp = IdspReader().ReadFormat(IdspWriter().GetFile(fmt))
    back = DspReader().ReadFormat(DspWriter().GetFile(idsp))
    for g, f in zip(back.Channels, fmt.Channels):
        assert np.array_equal(g.GetAdpcmAudio(), f.GetAdpcmAudio())


# ---------------------------------------------------------------- full size
def test_full_size_batch_2048_stereo_60s():
    """2048 stereo files of 60 s written and read back on the device, checked by sampled digests"""
    nf, nch, n = 2048, 2, 60 * 48000
    L_ = _lib.lib()
    nb = L_.vga_gcadpcm_sample_count_to_byte_count(n)
    pitch = (nb + 15) // 16 * 16
    gen = torch.Generator(device="cuda").manual_seed(7)
    adpcm = torch.randint(0, 256, (nf * nch, pitch), dtype=torch.uint8, device="cuda", generator=gen)
    co = torch.zeros((nf * nch, 16), dtype=torch.int16, device="cuda")
    back = torch.empty_like(adpcm)
    picks = [0, 1, 777, 2047]

    def check_rows():
        for f in picks:
            for c in range(nch):
                r = f * nch + c
                assert hashlib.sha256(back[r, :nb].cpu().numpy().tobytes()).digest() == \
                    hashlib.sha256(adpcm[r, :nb].cpu().numpy().tobytes()).digest()

    # HPS
    hp = _lib.HpsParamsC(48000, n, 0, 0, 0)
    hl = _lib.HpsLayoutC()
    _lib.check(L_.vga_hps_layout_for(C.byref(hp), nch, C.byref(hl)))
    fp = (hl.file_size + 255) // 256 * 256
    files = torch.empty((nf, fp), dtype=torch.uint8, device="cuda")
    _lib.check(L_.vga_hps_write_device(C.byref(hp), nch, nf, adpcm.data_ptr(), pitch, nb, co.data_ptr(), None, None, None, 0, 0,
                                       files.data_ptr(), fp, st()))
    from vgaudio_amd.hps import parse as hps_parse
    for f in picks:
        one = files[f, :hl.file_size].cpu().numpy().tobytes()
        R = ref.hps_parse(one)
        assert [hashlib.sha256(a).digest() for a in R["audio"]] == \
            [hashlib.sha256(adpcm[f * nch + c, :nb].cpu().numpy().tobytes()).digest() for c in range(nch)]
    info, blocks = hps_parse(files[0, :hl.file_size].cpu().numpy().tobytes())
    _lib.check(L_.vga_hps_read_device(C.byref(info), blocks, files.data_ptr(), fp, nf, back.data_ptr(), pitch, st()))
    check_rows()
    del files
    # IDSP
    ip = _lib.IdspParamsC(48000, n, 0, 0, 0, 0x10, 1)
    il = _lib.IdspLayoutC()
    _lib.check(L_.vga_idsp_layout_for(C.byref(ip), nch, C.byref(il)))
    fp = (il.file_size + 255) // 256 * 256
    files = torch.empty((nf, fp), dtype=torch.uint8, device="cuda")
    _lib.check(L_.vga_idsp_write_device(C.byref(ip), nch, nf, adpcm.data_ptr(), pitch, nb, co.data_ptr(), None, None, None,
                                        files.data_ptr(), fp, st()))
    from vgaudio_amd.idsp import parse as idsp_parse
    info = idsp_parse(files[0, :il.file_size].cpu().numpy().tobytes())
    back.zero_()
    _lib.check(L_.vga_idsp_read_device(C.byref(info), files.data_ptr(), fp, nf, back.data_ptr(), pitch, st()))
    check_rows()
