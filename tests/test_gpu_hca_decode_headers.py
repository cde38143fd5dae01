"""HCA headers the encoder never writes (tests/hca_headers_ref.py) through the decode kernels on the GPU: every family
through vga_hca_decode_batch (several streams a call; 1, 3, 16 and 64 frames a workgroup on a subset) and through the
in-HBM chain vga_hca_parse -> vga_hca_read_device -> vga_hca_decode_device.  PCM equals the C oracle's bit for bit;
where the reference throws IndexOutOfRangeException (the oracle's -6) the call returns VGA_ERR_OUT_OF_RANGE."""
import ctypes as C

import numpy as np
import pytest
import torch

import hca_headers_ref as hh
from oracle import pyoracle as po
from vgaudio_amd import _lib

pytestmark = pytest.mark.gpu
L = _lib.lib
FAMILIES = hh.families()
STREAMS = 3


def st():
    return torch.cuda.current_stream().cuda_stream


def _hinfo(info):
    h = _lib.HcaInfoC()
    for k in hh.FIELDS:
        setattr(h, k, getattr(info, k))
    return h


def decode_batch(info, streams):
    """vga_hca_decode_batch over [stream][frame_count, frame_size] frames: (rc, [nch, n] per stream)"""
    nch, n = info.channel_count, max(info.sample_count, 1)
    frames = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in streams]
    pcm = [np.zeros((nch, n), np.int16) for _ in streams]
    fp = (_lib.u8p * len(frames))(*[f.ctypes.data_as(_lib.u8p) for f in frames])
    pp = (C.POINTER(C.c_int16) * (len(frames) * nch))(*[p[c].ctypes.data_as(C.POINTER(C.c_int16)) for p in pcm for c in range(nch)])
    rc = L().vga_hca_decode_batch(C.byref(_hinfo(info)), fp, len(frames), pp)
    return rc, [p[:, :info.sample_count] for p in pcm]


def expected(info, streams):
    """the oracle per stream: (library rc, [pcm]) -- OUT_OF_RANGE when any stream throws"""
    outs = [po.hca_decode(info, np.ascontiguousarray(s).reshape(-1)) for s in streams]
    for rc, _ in outs:
        assert rc in (0, -6), rc
    if any(rc == -6 for rc, _ in outs):
        return _lib.VGA_ERR_OUT_OF_RANGE, None
    return 0, [np.asarray(p) for _, p in outs]


def _cases(family, seed):
    rng = np.random.default_rng(seed)
    for k, h in enumerate(FAMILIES[family]):
        e = h.expected()
        if e["frame_size"] < 8 or e["hfr_group_count"] > 8 or e["total_band_count"] > 128:
            continue
        streams = [hh.frames_for(h, rng, "mixed", intensity_max=15 if (k + s) % 4 == 0 else 14) for s in range(STREAMS)]
        yield h, h.info(), streams


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_decode_batch_matches_oracle(family):
    for h, info, streams in _cases(family, 300 + len(family)):
        want_rc, want = expected(info, streams)
        runs = (1, 3, 16, 64) if family in ("bands", "frame_size") else (0,)
        for run in runs:
            old = L().vga_testing_hca_frames_per_group_this_thread(run) if run else None
            try:
                rc, got = decode_batch(info, streams)
            finally:
                if run:
                    L().vga_testing_hca_frames_per_group_this_thread(old)
            assert rc == want_rc, (h, run, rc, L().vga_last_error())
            if rc == 0:
                for s in range(STREAMS):
                    assert np.array_equal(got[s], want[s]), (h, run, s)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_in_hbm_chain_matches_oracle(family):
    """file images of the family -> parse -> read on the device -> decode on the device; status bit 32 where the
    reference throws on intensity 15"""
    for h, info, streams in _cases(family, 400 + len(family)):
        imgs = [h.image(s.tobytes()) for s in streams]
        fi = _lib.HcaFileInfoC()
        buf = np.frombuffer(imgs[0], np.uint8)
        rc = L().vga_hca_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(fi))
        if rc:
            continue                                            # refusals: test_hca_decode_headers_host
        H = fi.hca
        want_rc, want = expected(info, streams)
        ws = L().vga_hca_decode_workspace_bytes(C.byref(H), STREAMS)
        if ws == 0:                                             # make_device_info refuses: up front, no launch
            assert want_rc == _lib.VGA_ERR_OUT_OF_RANGE, h
            continue
        fp = len(imgs[0]) + 5
        d = torch.zeros(STREAMS * fp, dtype=torch.uint8, device="cuda")
        for f, img in enumerate(imgs):
            d[f * fp:f * fp + len(img)] = torch.from_numpy(np.frombuffer(img, np.uint8).copy()).cuda()
        pitch = (H.frame_count * H.frame_size + 8 + 15) // 16 * 16
        frames = torch.zeros((STREAMS, pitch), dtype=torch.uint8, device="cuda")
        _lib.check(L().vga_hca_read_device(C.byref(fi), d.data_ptr(), fp, STREAMS, frames.data_ptr(), pitch, None, st()))
        work = torch.zeros(ws, dtype=torch.uint8, device="cuda")
        n, nch = H.sample_count, H.channel_count
        pcm = torch.zeros((STREAMS, nch, n), dtype=torch.int16, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(L().vga_hca_decode_device(C.byref(H), frames.data_ptr(), pitch, STREAMS, pcm.data_ptr(), nch * n, n,
                                             work.data_ptr(), ws, status.data_ptr(), st()))
        torch.cuda.synchronize()
        s = int(status.item())
        if want_rc:
            assert s & 32, h
            continue
        assert s == 0, (h, s)
        got = pcm.cpu().numpy()
        for f in range(STREAMS):
            assert np.array_equal(got[f], want[f]), (h, f)


def test_largest_lds_footprint_decodes_exactly():
    """8 channels, 128 coded bands each, 65535-byte frames: the frames kernel's LDS comes to 160 976 of 163 840 bytes
    a CU, with 32-bit chunk offsets; it decodes exactly (or would be refused up front, never reach the kernel unchecked)"""
    rng = np.random.default_rng(7)
    h = hh.comp("largest", 8, fs=0xFFFF, total=128, base=128, stereo=0, per_hfr=0, frame_count=2, direct=True)
    info = h.info()
    assert info.frame_size == 0xFFFF
    streams = [hh.frames_for(h, rng, "mixed") for _ in range(2)]
    want_rc, want = expected(info, streams)
    assert want_rc == 0
    rc, got = decode_batch(info, streams)
    assert rc == 0, L().vga_last_error()
    for s in range(2):
        assert np.array_equal(got[s], want[s]), s


def test_intensity_15_is_refused_with_out_of_range():
    """one secondary intensity of 15 in one frame of one stream: the whole call is VGA_ERR_OUT_OF_RANGE (the reference
    throws IndexOutOfRangeException at that frame, CriHcaDecoder.cs:157); 14 decodes"""
    from oracle.pyref import crihca as pyref
    info, frames = hh.encoder_frames(2, 1024 * 6, "Lowest", seed=3)
    h = pyref.HcaInfo()
    for k in hh.FIELDS:
        setattr(h, k, getattr(info, k))
    for value in (14, 15):
        fr = frames.copy()
        f = pyref.Frame(h)
        pyref._unpack_frame(f, pyref.BitReader(bytes(fr[3])))
        f.channels[1].intensity = [1, 2, 3, value, 4, 5, 6, 7]
        fr[3] = np.frombuffer(pyref.pack_frame(f), np.uint8)
        want_rc, want = expected(info, [frames, fr])
        rc, got = decode_batch(info, [frames, fr])
        assert rc == want_rc == (_lib.VGA_ERR_OUT_OF_RANGE if value == 15 else 0)
        if rc == 0:
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
