"""DSP, ADX and HCA file readers on the GPU: round trips through the product writers, batched device reads against host
reads (pitches that are and are not multiples of 16, image offsets of every residue mod 16), the two ADX paths, the whole
read -> crypt -> decode chain in HBM, encryption, corrupted CRCs and the full BASELINE shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

import container_readers_ref as ref
from oracle import pyoracle as po
from vgaudio_amd import _lib, synth
from vgaudio_amd.adx import AdxConfiguration, AdxReader, AdxWriter
from vgaudio_amd.criadx import CriAdxFormat, CriAdxKey, CriAdxParameters, CriAdxType
from vgaudio_amd.crihca import CriHcaEncryption, CriHcaFormat, CriHcaKey, CriHcaParameters, CriHcaQuality
from vgaudio_amd.dsp import DspConfiguration, DspReader, DspWriter
from vgaudio_amd.gcadpcm import GcAdpcmFormat, Pcm16Format
from vgaudio_amd.hca import HcaConfiguration, HcaReader, HcaWriter

pytestmark = pytest.mark.gpu
L = _lib.lib


def st():
    return torch.cuda.current_stream().cuda_stream


def pcm16(nch, n, looping=False, ls=0, le=0, seed=0):
    f = Pcm16Format([synth.sine(n, 170.0 + 90.0 * c + seed) for c in range(nch)], 48000)
    if looping:
        f.Looping, f.LoopStart, f.LoopEnd = True, ls, le
    return f


def _u8(data):
    return np.frombuffer(bytes(data), dtype=np.uint8)


# ---------------------------------------------------------------- round trips through the product writers
@pytest.mark.parametrize("nch,n,looping", [(1, 5003, False), (2, 30000, True), (3, 14 * 700, False)])
def test_dsp_round_trip(nch, n, looping):
    fmt = GcAdpcmFormat().EncodeFromPcm16(pcm16(nch, n))
    if looping:
        fmt = fmt.WithLoop(True, n // 4, n - 10)
    img = DspWriter(DspConfiguration(SamplesPerInterleave=14 * 32)).GetFile(fmt)
    back = DspReader().ReadFormat(img)
    assert back.ChannelCount == nch and back.Looping == fmt.Looping
    for a, b in zip(fmt.Channels, back.Channels):         # a looping file is trimmed to its loop end (TrimFile)
        got = b.GetAdpcmAudio()
        assert np.array_equal(a.GetAdpcmAudio()[:len(got)], got) and np.array_equal(a.Coefs, b.Coefs)
    rows = np.stack([c.GetAdpcmAudio() for c in back.Channels])
    coefs = np.stack([c.Coefs for c in back.Channels]).astype(np.int16)
    want = po.gc_decode_batch(rows, coefs, back.Channels[0].SampleCount)
    got = np.stack(back.ToPcm16().Channels)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("nch,n,looping,version,type_", [(1, 4001, False, 4, CriAdxType.Linear), (2, 48000, True, 4, CriAdxType.Linear),
                                                          (3, 20000, True, 3, CriAdxType.Exponential), (2, 9000, False, 4, CriAdxType.Fixed)])
def test_adx_round_trip(nch, n, looping, version, type_):
    src = pcm16(nch, n, looping, n // 3 + 5, n - 200)        # room for the 3 frames the writer adds behind the loop end
    fmt = CriAdxFormat().EncodeFromPcm16(src, CriAdxParameters(Version=version, Type=type_))
    img = AdxWriter(AdxConfiguration(Version=version, Type=type_)).GetFile(fmt)
    back, cfg = AdxReader().ReadWithConfig(img)
    assert cfg.FrameSize == 18 and cfg.Type == type_ and cfg.EncryptionKey is None
    # the writer trims a looping file to its loop end (TrimFile): the file says how many samples it holds
    assert back.AlignmentSamples == fmt.AlignmentSamples and back.SampleCount == AdxWriter().Layout(fmt).sample_count
    assert (back.Looping, back.LoopStart, back.LoopEnd) == (fmt.Looping, fmt.LoopStart, fmt.LoopEnd)
    for a, b in zip(fmt.Channels, back.Channels):
        m = min(len(a.Audio), len(b.Audio))
        assert m > 0 and np.array_equal(a.Audio[:m], b.Audio[:m])
    got = np.stack(back.ToPcm16().Channels)
    p = po.adx_params(version=version, type=type_, padding=back.AlignmentSamples, sample_rate=48000)
    want = po.adx_decode_batch(np.stack([c.Audio for c in back.Channels]), back.UnalignedSampleCount, p)
    assert np.array_equal(got, want)
    keep = fmt.UnalignedLoopEnd if looping else got.shape[1]        # a trimmed file carries the audio up to its loop end
    assert np.array_equal(got[:, :keep], np.stack(fmt.ToPcm16().Channels)[:, :keep])


@pytest.mark.parametrize("nch,n,looping", [(1, 30000, False), (2, 100000, True), (6, 20000, False)])
def test_hca_round_trip(nch, n, looping):
    src = pcm16(nch, n, looping, 5000, n - 3000)
    fmt = CriHcaFormat().EncodeFromPcm16(src, CriHcaParameters(Quality=CriHcaQuality.High))
    img = HcaWriter().GetFile(fmt)
    r = HcaReader()
    back = r.ReadFormat(img)
    assert r.BadCrcFrames == 0
    assert np.array_equal(np.asarray(back.AudioData), np.asarray(fmt.AudioData))
    assert back.Hca.SampleCount == fmt.Hca.SampleCount and back.Hca.Looping == looping
    rc, want = po.hca_decode(po.HcaInfo.from_buffer_copy(back.Hca.c), np.asarray(back.AudioData).reshape(-1))
    assert rc == 0
    assert np.array_equal(np.stack(back.ToPcm16().Channels), want)


# ---------------------------------------------------------------- batched device reads against host reads
def _batch(img, nfiles, offset, pitch_extra, vary=None, seed=0):
    """nfiles copies of `img` at `offset` in a device buffer, file_pitch = len + pitch_extra.  vary = (lo, hi): every 7th
    byte of img[lo:hi] is changed in every file but the first, so that rows read from the wrong file show"""
    rng = np.random.default_rng(seed)
    fp = len(img) + pitch_extra
    host = np.zeros(offset + fp * nfiles + 64, np.uint8)
    imgs = []
    for f in range(nfiles):
        a = np.frombuffer(img, np.uint8).copy()
        if vary is not None and f > 0:                       # file 0 stays as it is
            lo, hi = vary
            a[lo + f:hi:7] = rng.integers(0, 256, len(a[lo + f:hi:7]), dtype=np.uint8)
        imgs.append(a)
        host[offset + f * fp:offset + f * fp + len(a)] = a
    return torch.from_numpy(host).cuda(), fp, imgs


def _host_rows(read, info, img, nrows, row_bytes):
    rows = [np.zeros(max(row_bytes, 1), np.uint8) for _ in range(nrows)]
    buf = _u8(img)
    _lib.check(read(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), (_lib.u8p * nrows)(*[r.ctypes.data_as(_lib.u8p) for r in rows])))
    return [r[:row_bytes] for r in rows]


@pytest.mark.parametrize("offset", range(16))
def test_adx_device_read_equals_host_read_every_residue(offset):
    rng = np.random.default_rng(offset)
    nch = 1 + offset % 3
    fmt = CriAdxFormat().EncodeFromPcm16(pcm16(nch, 3000 + 37 * offset))
    img = AdxWriter().GetFile(fmt)
    info = _lib.AdxFileInfoC()
    _lib.check(L().vga_adx_parse(_u8(img).ctypes.data_as(_lib.u8p), len(img), C.byref(info)))
    nf = 3
    # vary the audio per file so that rows of different files differ
    imgs = []
    for f in range(nf):
        a = bytearray(img)
        for k in range(info.audio_offset, info.audio_offset + info.audio_bytes * nch, 5):
            a[k] = rng.integers(0, 256)
        imgs.append(bytes(a))
    for pitch_extra in (offset, 16 - len(img) % 16 + 32):
        fp = len(img) + pitch_extra
        host = np.zeros(offset + fp * nf + 16, np.uint8)
        for f, a in enumerate(imgs):
            host[offset + f * fp:offset + f * fp + len(a)] = np.frombuffer(a, np.uint8)
        d = torch.from_numpy(host).cuda()
        want = [r for a in imgs for r in _host_rows(L().vga_adx_read, info, a, nch, info.audio_bytes)]
        for row_pitch in (info.audio_bytes + (16 - info.audio_bytes % 16) % 16, info.audio_bytes + 3):
            for general in (0, 1):
                out = torch.full((nf * nch, row_pitch), 0xAA, dtype=torch.uint8, device="cuda")
                old = L().vga_testing_adx_read_general_this_thread(general)
                try:
                    _lib.check(L().vga_adx_read_device(C.byref(info), d.data_ptr() + offset, fp, nf, out.data_ptr(), row_pitch, st()))
                finally:
                    L().vga_testing_adx_read_general_this_thread(old)
                o = out.cpu().numpy()
                for r in range(nf * nch):
                    assert np.array_equal(o[r, :info.audio_bytes], want[r]), (offset, pitch_extra, row_pitch, general, r)
                    assert (o[r, info.audio_bytes:] == 0xAA).all()                      # nothing past the row is written


@pytest.mark.parametrize("offset", range(16))
@pytest.mark.parametrize("nch", [1, 2, 3])
def test_dsp_device_read_equals_host_read(offset, nch):
    _dsp_device_read_equals_host_read(nch, 14 * 300 + offset, offset)


@pytest.mark.parametrize("offset", range(16))
@pytest.mark.parametrize("nch", [2, 3])
def test_dsp_device_read_short_last_block(offset, nch):
    """interleave 64 bytes, last block 8, files 16 bytes apart: at offset 0 the read moves 16-byte granules, and the last
    block, shorter than one, goes byte by byte"""
    _dsp_device_read_equals_host_read(nch, 14 * 8 * 37 + 1, offset, pitch_to_16=True)


def _dsp_device_read_equals_host_read(nch, n, offset, pitch_to_16=False):
    fmt = GcAdpcmFormat().EncodeFromPcm16(pcm16(nch, n))
    img = DspWriter(DspConfiguration(SamplesPerInterleave=14 * 8)).GetFile(fmt)
    info = _lib.DspInfoC()
    _lib.check(L().vga_dsp_parse(_u8(img).ctypes.data_as(_lib.u8p), len(img), C.byref(info)))
    for c in range(nch):
        assert np.array_equal(_host_rows(L().vga_dsp_read, info, img, nch, info.adpcm_bytes)[c], fmt.Channels[c].GetAdpcmAudio())
    nf = 4
    extra = -len(img) % 16 if pitch_to_16 else offset + 3
    d, fp, imgs = _batch(img, nf, offset, extra, vary=(info.audio_offset, info.audio_offset + info.data_length), seed=offset)
    want = [r for a in imgs for r in _host_rows(L().vga_dsp_read, info, a, nch, info.adpcm_bytes)]
    assert not np.array_equal(want[0], want[nch])                     # the files differ
    for row_pitch in ((info.adpcm_bytes + 15) // 16 * 16, info.adpcm_bytes + 1):
        out = torch.full((nf * nch, row_pitch), 0xAA, dtype=torch.uint8, device="cuda")
        _lib.check(L().vga_dsp_read_device(C.byref(info), d.data_ptr() + offset, fp, nf, out.data_ptr(), row_pitch, st()))
        o = out.cpu().numpy()
        for r in range(nf * nch):
            assert np.array_equal(o[r, :info.adpcm_bytes], want[r]), (row_pitch, r)
            assert (o[r, info.adpcm_bytes:] == 0xAA).all()


def _hca_batch_check(img, info, offset, nf=3):
    """nf varied copies of an HCA image at `offset`: device read against host reads, bad CRCs against ref.crc16"""
    H = info.hca
    nbytes = H.frame_count * H.frame_size
    lo = info.frames_offset
    d, fp, imgs = _batch(img, nf, offset, offset, vary=(lo + nbytes // 2, lo + nbytes), seed=offset)
    want, want_bad = [], []
    for a in imgs:
        fr = np.zeros(nbytes, np.uint8)
        bad = C.c_int(-1)
        _lib.check(L().vga_hca_read(a.ctypes.data_as(_lib.u8p), len(a), C.byref(info), fr.ctypes.data_as(_lib.u8p), C.byref(bad)))
        assert np.array_equal(fr, a[lo:lo + nbytes])
        assert bad.value == ref.bad_crc_frames(fr.reshape(H.frame_count, H.frame_size))
        want.append(fr)
        want_bad.append(bad.value)
    for pitch in ((nbytes + 8 + 15) // 16 * 16, (nbytes + 8 + 3) // 4 * 4 + 4):
        out = torch.full((nf, pitch), 0xAA, dtype=torch.uint8, device="cuda")
        bad = torch.full((nf,), -1, dtype=torch.int32, device="cuda")
        _lib.check(L().vga_hca_read_device(C.byref(info), d.data_ptr() + offset, fp, nf, out.data_ptr(), pitch, bad.data_ptr(), st()))
        o = out.cpu().numpy()
        for f in range(nf):
            assert np.array_equal(o[f, :nbytes], want[f]) and (o[f, nbytes:nbytes + 8] == 0).all()
            assert (o[f, (nbytes + 8 + 3) // 4 * 4:] == 0xAA).all()
        assert bad.cpu().tolist() == want_bad
    return want_bad


@pytest.mark.parametrize("offset", range(16))
def test_hca_device_read_equals_host_read(offset):
    fmt = CriHcaFormat().EncodeFromPcm16(pcm16(2, 20000 + offset * 1000))
    img = HcaWriter().GetFile(fmt)
    info = _lib.HcaFileInfoC()
    _lib.check(L().vga_hca_parse(_u8(img).ctypes.data_as(_lib.u8p), len(img), C.byref(info)))
    H = info.hca
    nbytes = H.frame_count * H.frame_size
    assert np.array_equal(np.frombuffer(img, np.uint8)[info.frames_offset:info.frames_offset + nbytes], np.asarray(fmt.AudioData).reshape(-1))
    bad = _hca_batch_check(img, info, offset)
    assert bad[0] == 0 and max(bad) > 0                            # file 0 keeps its frames; the varied frames fail their CRC


@pytest.mark.parametrize("frame_size,offset", [(4097, 3), (5000, 1), (12345, 6), (32767, 13)])
def test_hca_frames_larger_than_4096_bytes(frame_size, offset):
    """frames up to the largest size a file can declare: the CRC of every frame is still checked (against ref.crc16)"""
    rng = np.random.default_rng(frame_size)
    fc = 5
    frames = ref.hca_frames(fc, frame_size, rng)
    frames[1, 100] ^= 1                                             # one frame with a bad CRC
    img = ref.hca_image([ref.hca_fmt(2, 48000, fc), ref.hca_comp(frame_size, 1, 15, 1, 0, 100, 60, 20, 5), ref.hca_pad()],
                        frames.tobytes())
    info = _lib.HcaFileInfoC()
    _lib.check(L().vga_hca_parse(_u8(img).ctypes.data_as(_lib.u8p), len(img), C.byref(info)))
    assert info.hca.frame_size == frame_size
    r = HcaReader()
    back = r.ReadFormat(img)
    assert r.BadCrcFrames == 1 == ref.bad_crc_frames(frames)
    assert np.array_equal(np.asarray(back.AudioData), frames)
    _hca_batch_check(img, info, offset)


def test_hca_corrupted_crc_is_counted_not_rejected():
    fmt = CriHcaFormat().EncodeFromPcm16(pcm16(2, 40000))
    img = bytearray(HcaWriter().GetFile(fmt))
    info = HcaReader().ReadMetadata(bytes(img))
    fs = info.hca.frame_size
    img[info.frames_offset + 5 * fs + 17] ^= 0x40                     # one byte of frame 5, after its CRC was written
    r = HcaReader()
    back = r.ReadFormat(bytes(img))
    assert r.BadCrcFrames == 1
    assert np.asarray(back.AudioData)[5, 17] == np.asarray(fmt.AudioData)[5, 17] ^ 0x40


# ---------------------------------------------------------------- encryption
ADX_CANDIDATES = [CriAdxKey(0x1234, 0x5A7B, 0x0C5D), CriAdxKey(0x4F3D, 0x58B1, 0x5C4F), CriAdxKey(0x1111, 0x3333, 0x7777)]


@pytest.mark.parametrize("enc", [8, 9])
def test_adx_encrypted_files(enc):
    src = pcm16(2, 30000)
    fmt = CriAdxFormat().EncodeFromPcm16(src)
    key = ADX_CANDIDATES[1]
    img = AdxWriter(AdxConfiguration(EncryptionType=enc, EncryptionKey=key)).GetFile(fmt)
    plain = np.stack(fmt.ToPcm16().Channels)
    with_key, cfg = AdxReader(EncryptionKey=key).ReadWithConfig(img)
    assert cfg.EncryptionType == enc and cfg.EncryptionKey is key
    found, cfg2 = AdxReader(Keys=ADX_CANDIDATES).ReadWithConfig(img)
    assert cfg2.EncryptionKey is not None and cfg2.EncryptionKey.KeyCode == key.KeyCode
    if enc == 8:                          # type 9 masks the scale's top bits (:33): only type 8 gives the plain audio back
        assert np.array_equal(np.stack(with_key.ToPcm16().Channels), plain)
        assert all(np.array_equal(a.Audio, b.Audio) for a, b in zip(fmt.Channels, found.Channels))
    for a, b in zip(with_key.Channels, found.Channels):
        assert np.array_equal(a.Audio, b.Audio)
    none, cfg3 = AdxReader(Keys=[ADX_CANDIDATES[2]]).ReadWithConfig(img)     # no candidate matches: left as it is
    assert cfg3.EncryptionKey is None
    raw = AdxReader().ReadMetadata(img)
    enc_rows = _host_rows(L().vga_adx_read, raw, img, 2, raw.audio_bytes)
    assert all(np.array_equal(a.Audio, b) for a, b in zip(none.Channels, enc_rows))


def test_hca_encrypted_files():
    fmt = CriHcaFormat().EncodeFromPcm16(pcm16(2, 30000))
    plain_frames = np.asarray(fmt.AudioData).copy()
    plain_pcm = np.stack(fmt.ToPcm16().Channels)
    # type 1
    f1 = CriHcaFormat(plain_frames.copy(), fmt.Hca)
    img1 = HcaWriter(HcaConfiguration(EncryptionKey=CriHcaKey(CriHcaKey.Type1))).GetFile(f1)
    back, cfg = HcaReader().ReadWithConfig(img1)
    assert back.Hca.EncryptionType == 0 and cfg.EncryptionKey.KeyType == 1
    assert np.array_equal(np.asarray(back.AudioData), plain_frames)
    # type 56 with candidates
    keys = [CriHcaKey(0x0123456789ABCDEF), CriHcaKey(0x1122334455667788), CriHcaKey(0x0F1E2D3C4B5A6978)]   # made-up codes
    f56 = CriHcaFormat(plain_frames.copy(), fmt.Hca)
    f56.Hca.EncryptionType = 0
    img56 = HcaWriter(HcaConfiguration(EncryptionKey=keys[2])).GetFile(f56)
    back, cfg = HcaReader(Keys=keys).ReadWithConfig(img56)
    assert cfg.EncryptionKey is keys[2] and back.Hca.EncryptionType == 0
    assert np.array_equal(np.asarray(back.AudioData), plain_frames)
    assert np.array_equal(np.stack(back.ToPcm16().Channels), plain_pcm)
    back, cfg = HcaReader(EncryptionKey=keys[2]).ReadWithConfig(img56)
    assert np.array_equal(np.asarray(back.AudioData), plain_frames)
    with pytest.raises(_lib.InvalidDataError):
        HcaReader(Keys=keys[:1]).ReadFormat(img56)
    raw, cfg = HcaReader(Decrypt=False).ReadWithConfig(img56)              # Decrypt = false: untouched
    assert raw.Hca.EncryptionType == 56 and cfg.EncryptionKey is None
    info = HcaReader().ReadMetadata(img56)
    nbytes = info.hca.frame_count * info.hca.frame_size
    assert np.array_equal(np.asarray(raw.AudioData).reshape(-1), np.frombuffer(img56, np.uint8)[info.frames_offset:info.frames_offset + nbytes])


# ---------------------------------------------------------------- the whole chain in HBM
def test_adx_chain_in_hbm_equals_host_path():
    nf, nch, n = 5, 2, 24000
    key = ADX_CANDIDATES[0]
    imgs, want = [], []
    for f in range(nf):
        fmt = CriAdxFormat().EncodeFromPcm16(pcm16(nch, n, seed=13 * f))
        img = AdxWriter(AdxConfiguration(EncryptionType=8, EncryptionKey=key)).GetFile(fmt)
        imgs.append(img)
        want.append(np.stack(AdxReader(Keys=ADX_CANDIDATES).ReadFormat(img).ToPcm16().Channels))
    info = AdxReader().ReadMetadata(imgs[0])
    fp = (len(imgs[0]) + 15) // 16 * 16
    d = torch.zeros(nf * fp, dtype=torch.uint8, device="cuda")
    for f, img in enumerate(imgs):
        d[f * fp:f * fp + len(img)] = torch.from_numpy(_u8(img).copy()).cuda()
    pitch = (info.audio_bytes + 15) // 16 * 16
    rows = torch.zeros((nf * nch, pitch), dtype=torch.uint8, device="cuda")
    _lib.check(L().vga_adx_read_device(C.byref(info), d.data_ptr(), fp, nf, rows.data_ptr(), pitch, st()))
    keys = (_lib.AdxKeyC * len(ADX_CANDIDATES))(*[k.c for k in ADX_CANDIDATES])
    for f in range(nf):                                    # the key search and the crypt pass run per file (channel order)
        idx = C.c_int(-1)
        base = rows.data_ptr() + f * nch * pitch
        _lib.check(L().vga_adx_find_key_device(base, pitch, info.audio_bytes, nch, info.revision, 18, keys, len(keys), C.byref(idx), st()))
        assert idx.value == 0
        _lib.check(L().vga_adx_crypt_device(base, pitch, info.audio_bytes, nch, C.byref(keys[idx.value]), info.revision, 18, st()))
    p = _lib.AdxParams()
    L().vga_adx_default_params(C.byref(p))
    p.sample_rate, p.padding, p.version, p.type = info.sample_rate, info.inserted_samples, info.version, info.type
    ns = info.sample_count - info.inserted_samples
    pcm = torch.zeros((nf * nch, ns), dtype=torch.int16, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L().vga_adx_decode_device(rows.data_ptr(), pitch, info.audio_bytes, nf * nch, ns, C.byref(p), pcm.data_ptr(), ns,
                                         status.data_ptr(), st()))
    got = pcm.cpu().numpy()
    for f in range(nf):
        assert np.array_equal(got[f * nch:(f + 1) * nch], want[f])


def test_hca_chain_in_hbm_equals_host_path():
    nf = 4
    fmts = CriHcaFormat.EncodeBatchFromPcm16([pcm16(2, 50000, seed=7 * f) for f in range(nf)])
    imgs = [HcaWriter(HcaConfiguration(EncryptionKey=CriHcaKey(CriHcaKey.Type1))).GetFile(CriHcaFormat(np.asarray(f.AudioData).copy(), f.Hca))
            for f in fmts]
    want = [np.stack(HcaReader().ReadFormat(img).ToPcm16().Channels) for img in imgs]
    info = HcaReader().ReadMetadata(imgs[0])
    H = info.hca
    fp = len(imgs[0]) + 7
    d = torch.zeros(nf * fp, dtype=torch.uint8, device="cuda")
    for f, img in enumerate(imgs):
        d[f * fp:f * fp + len(img)] = torch.from_numpy(_u8(img).copy()).cuda()
    pitch = (H.frame_count * H.frame_size + 8 + 15) // 16 * 16
    frames = torch.zeros((nf, pitch), dtype=torch.uint8, device="cuda")
    bad = torch.zeros(nf, dtype=torch.int32, device="cuda")
    _lib.check(L().vga_hca_read_device(C.byref(info), d.data_ptr(), fp, nf, frames.data_ptr(), pitch, bad.data_ptr(), st()))
    dec = CriHcaKey(CriHcaKey.Type1).DecryptionTable
    _lib.check(L().vga_hca_crypt_device(frames.data_ptr(), pitch, nf, H.frame_count, H.frame_size, dec.ctypes.data_as(_lib.u8p), st()))
    ws = L().vga_hca_decode_workspace_bytes(C.byref(H), nf)
    work = torch.zeros(max(ws, 1), dtype=torch.uint8, device="cuda")
    n = H.sample_count
    pcm = torch.zeros((nf, 2, n), dtype=torch.int16, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(L().vga_hca_decode_device(C.byref(H), frames.data_ptr(), pitch, nf, pcm.data_ptr(), 2 * n, n, work.data_ptr(), ws,
                                         status.data_ptr(), st()))
    torch.cuda.synchronize()
    assert bad.cpu().tolist() == [0] * nf and int(status.item()) == 0
    got = pcm.cpu().numpy()
    for f in range(nf):
        assert np.array_equal(got[f], want[f])


# ---------------------------------------------------------------- full size
def _tile_images(header, rows_dev, nch, frame_size, audio_offset, image_bytes):
    """images built on the device: one header each, the rows' frames interleaved one frame per channel"""
    nrows, row = rows_dev.shape
    nf = nrows // nch
    fp = (image_bytes + 15) // 16 * 16 + 16
    files = torch.zeros((nf, fp), dtype=torch.uint8, device="cuda")
    files[:, :len(header)] = torch.from_numpy(np.frombuffer(header, np.uint8).copy()).cuda()
    k = row // frame_size
    inter = rows_dev[:, :k * frame_size].reshape(nf, nch, k, frame_size).permute(0, 2, 1, 3).reshape(nf, -1)
    files[:, audio_offset:audio_offset + inter.shape[1]] = inter
    return files, fp


def test_full_size_adx_batch():
    """configs[2]: 4096 channels x 48 kHz x 60 s, as 2048 stereo files read back in one call"""
    nf, nch, n = 2048, 2, 60 * 48000
    ap = _lib.AdxFileParamsC(48000, n, 0, 0, 0, 0, 18, 4, 3, 500, 0, 1)
    al = _lib.AdxFileLayoutC()
    _lib.check(L().vga_adx_file_layout_for(C.byref(ap), nch, C.byref(al)))
    ab = al.frame_count * 18
    small = np.zeros(al.file_size, np.uint8)
    zero = [np.zeros(ab, np.uint8) for _ in range(nch)]
    _lib.check(L().vga_adx_write((_lib.u8p * nch)(*[z.ctypes.data_as(_lib.u8p) for z in zero]), ab, np.zeros(nch, np.int16).ctypes.data_as(_lib.i16p),
                                 nch, C.byref(ap), small.ctypes.data_as(_lib.u8p)))
    info = _lib.AdxFileInfoC()
    _lib.check(L().vga_adx_parse(small.ctypes.data_as(_lib.u8p), len(small), C.byref(info)))
    g = torch.Generator(device="cuda").manual_seed(5)
    rows = torch.randint(0, 256, (nf * nch, ab), dtype=torch.uint8, device="cuda", generator=g)
    files, fp = _tile_images(small[:info.audio_offset].tobytes(), rows, nch, 18, info.audio_offset, len(small))
    pitch = (ab + 15) // 16 * 16
    out = torch.empty((nf * nch, pitch), dtype=torch.uint8, device="cuda")
    _lib.check(L().vga_adx_read_device(C.byref(info), files.data_ptr(), fp, nf, out.data_ptr(), pitch, st()))
    assert torch.equal(out[:, :ab], rows)


def test_full_size_hca_batch():
    """configs[3]: 1024 stereo streams x 48 kHz x 60 s, quality High"""
    ns, n = 1024, 60 * 48000
    info = _lib.HcaInfoC()
    hp = _lib.HcaParamsC(2, 0, 0, 2, 48000, n, 0, 0, 0)
    _lib.check(L().vga_hca_encoder_initialize(C.byref(hp), C.byref(info)))
    fb = info.frame_count * info.frame_size
    hdr = np.zeros(info.header_size, np.uint8)
    _lib.check(L().vga_hca_file_header(C.byref(info), None, 1.0, 0, 0, hdr.ctypes.data_as(_lib.u8p)))
    img = np.concatenate([hdr, np.zeros(fb, np.uint8)])
    fi = _lib.HcaFileInfoC()
    _lib.check(L().vga_hca_parse(img.ctypes.data_as(_lib.u8p), len(img), C.byref(fi)))
    g = torch.Generator(device="cuda").manual_seed(6)
    frames = torch.randint(0, 256, (ns, fb), dtype=torch.uint8, device="cuda", generator=g)
    fp = (len(img) + 15) // 16 * 16 + 3
    files = torch.zeros((ns, fp), dtype=torch.uint8, device="cuda")
    files[:, :info.header_size] = torch.from_numpy(hdr).cuda()
    files[:, info.header_size:info.header_size + fb] = frames
    pitch = (fb + 8 + 15) // 16 * 16
    out = torch.empty((ns, pitch), dtype=torch.uint8, device="cuda")
    bad = torch.empty(ns, dtype=torch.int32, device="cuda")
    _lib.check(L().vga_hca_read_device(C.byref(fi), files.data_ptr(), fp, ns, out.data_ptr(), pitch, bad.data_ptr(), st()))
    assert torch.equal(out[:, :fb], frames)
    b = bad.cpu().numpy()
    assert (b > info.frame_count * 0.99).all() and (b <= info.frame_count).all()   # random frames: almost every CRC is wrong


def test_crypt_pass_still_refreshes_crcs():
    """the crypt pass and the reader share one CRC helper: a frame the pass rewrites reads back with a good CRC"""
    fmt = CriHcaFormat().EncodeFromPcm16(pcm16(1, 20000))
    frames = np.asarray(fmt.AudioData).copy()
    CriHcaEncryption.Crypt(fmt.Hca, frames, CriHcaKey(CriHcaKey.Type1), False)
    for k in range(frames.shape[0]):
        assert ref.crc16(frames[k, :-2]) == (int(frames[k, -2]) << 8 | int(frames[k, -1]))
