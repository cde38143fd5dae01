"""The PCM *_device entry points of include/vgaudio_hip_pcm.h on a busy caller stream, the way
test_gpu_device_streams.py tests those of vgaudio_hip.h: inputs poisoned and then loaded behind a GPU delay on the
caller's stream, the call must return while the stream is still busy, and the outputs must equal the reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nwstm_pcm_ref as ref
from test_gpu_device_streams import Case, _eq, _ok, _run_on_busy_stream, _warm, delay  # noqa: F401  (delay: fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    return torch


def _L():
    from vgaudio_amd import _lib
    return _lib.lib()


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _params(n):
    from vgaudio_amd import _lib
    p = _lib.NwParamsC()
    p.target, p.sample_rate, p.sample_count, p.endianness = 2, 48000, n, -1
    p.samples_per_interleave = 999
    return p


def _pcm(k, nch, n):
    rng = np.random.default_rng(k)
    return rng.integers(-32768, 32768, (nch, n)).astype(np.int16)


def row_pcm8_encode(k):
    torch = _torch()
    x = _pcm(k, 5, 1003)
    src, dst = torch.from_numpy(x).cuda(), torch.zeros((5, 1003), dtype=torch.uint8, device="cuda")
    want = ((x.astype(np.int32) + 0x8000) >> 8).astype(np.uint8)
    return Case([src], [dst], lambda s: _L().vga_pcm8_encode_device(_vp(src), 1003, 1003, 5, 0, _vp(dst), 1003, C.c_void_p(s)),
                lambda: _eq(dst, want, "pcm8 encode"))


def row_pcm8_decode(k):
    torch = _torch()
    x = np.random.default_rng(k).integers(0, 256, (5, 1003)).astype(np.uint8)
    src, dst = torch.from_numpy(x).cuda(), torch.zeros((5, 1003), dtype=torch.int16, device="cuda")
    return Case([src], [dst], lambda s: _L().vga_pcm8_decode_device(_vp(src), 1003, 1003, 5, 1, _vp(dst), 1003, C.c_void_p(s)),
                lambda: _eq(dst, ref.decode_signed(x), "pcm8 decode signed"))


def _nw_image(k, nfiles=4, nch=2, n=3001):
    x = _pcm(k, nfiles * nch, n)
    imgs = [ref.build_image(2, ref.PCM16, 48000, [x[f * nch + c] for c in range(nch)], spi=999) for f in range(nfiles)]
    return x, imgs


def row_nwstm_pcm_write(k):
    torch = _torch()
    x, imgs = _nw_image(k)
    size = len(imgs[0])
    fp = (size + 15) // 16 * 16
    src = torch.from_numpy(x).cuda()
    dst = torch.zeros((4, fp), dtype=torch.uint8, device="cuda")
    p = _params(3001)
    want = np.zeros((4, fp), dtype=np.uint8)
    for f, im in enumerate(imgs):
        want[f, :size] = np.frombuffer(im, dtype=np.uint8)

    def check():
        _eq(dst[:, :size], want[:, :size], "nwstm pcm write")
    return Case([src], [dst], lambda s: _L().vga_nwstm_pcm_write_device(C.byref(p), 1, 2, 4, None, _vp(src), 0, 3001, _vp(dst),
                                                                        fp, C.c_void_p(s)), check)


def row_nwstm_pcm_read(k):
    torch = _torch()
    from vgaudio_amd.nwstm import parse_pcm
    x, imgs = _nw_image(k)
    size = len(imgs[0])
    files = torch.from_numpy(np.frombuffer(b"".join(imgs), dtype=np.uint8).copy()).cuda()
    info = parse_pcm(imgs[0])
    dst = torch.zeros((8, 3001), dtype=torch.int16, device="cuda")
    return Case([files], [dst], lambda s: _L().vga_nwstm_pcm_read_device(C.byref(info), _vp(files), size, 4, _vp(dst), 0, 3001,
                                                                         C.c_void_p(s)), lambda: _eq(dst, x, "nwstm pcm read"))


def _wave8(x):
    """8-bit WAVE data chunk bytes of int16 rows (Pcm8Codec.Encode, then frames of nch bytes)"""
    return ((x.astype(np.int32) + 0x8000) >> 8).astype(np.uint8).T.reshape(-1)


def row_wave_write_pcm8(k):
    torch = _torch()
    from vgaudio_amd import _lib
    x = _pcm(k, 3, 1001)
    p = _lib.WaveParamsC(22050, 1001, 0, 0, 0)
    size = _L().vga_wave_pcm8_file_size(C.byref(p), 3)
    src = torch.from_numpy(x).cuda()
    dst = torch.zeros(size, dtype=torch.uint8, device="cuda")
    want_data = _wave8(x)

    def check():
        got = dst.cpu().numpy()
        assert bytes(got[:4]) == b"RIFF" and np.array_equal(got[size - len(want_data):], want_data)
    return Case([src], [dst], lambda s: _L().vga_wave_write_pcm8_device(_vp(src), 0, 1001, 3, C.byref(p), _vp(dst), C.c_void_p(s)),
                check)


def row_wave_deinterleave_pcm8(k):
    torch = _torch()
    x = _pcm(k, 3, 1001)
    data = torch.from_numpy(_wave8(x).copy()).cuda()
    dst = torch.zeros((3, 1001), dtype=torch.int16, device="cuda")
    want = (((x.astype(np.int32) + 0x8000) >> 8) - 0x80) << 8
    return Case([data], [dst], lambda s: _L().vga_wave_deinterleave_pcm8_device(_vp(data), 1001, 3, _vp(dst), 0, 1001, C.c_void_p(s)),
                lambda: _eq(dst, want.astype(np.int16), "wave pcm8 deinterleave"))


ROWS = {
    "vga_pcm8_encode_device": row_pcm8_encode,
    "vga_pcm8_decode_device": row_pcm8_decode,
    "vga_nwstm_pcm_write_device": row_nwstm_pcm_write,
    "vga_nwstm_pcm_read_device": row_nwstm_pcm_read,
    "vga_wave_write_pcm8_device": row_wave_write_pcm8,
    "vga_wave_deinterleave_pcm8_device": row_wave_deinterleave_pcm8,
}


def test_table_covers_the_pcm_header():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vgaudio_hip_pcm.h")).read(), flags=re.S)
    assert set(ROWS) == set(re.findall(r"\b(vga_\w+_device)\s*\(", text))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ROWS))
def test_pcm_device_entry_point_on_a_busy_stream(name, delay):  # noqa: F811
    torch = _torch()
    S = torch.cuda.Stream()
    _warm(ROWS[name](0), S)
    case = ROWS[name](1)
    rc = _run_on_busy_stream(name, case, S, delay)
    S.synchronize()
    _ok(rc)
    case.check()
    torch.cuda.synchronize()
