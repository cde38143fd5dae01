"""vga_nwwav_bank_read_device on a busy caller stream, by the method of tests/test_gpu_device_streams.py: poisoned
buffers, a bounded GPU delay, the real inputs copied late on the same stream, then the call -- which must return while the
stream is still busy and must give the right bytes once it has drained."""
import numpy as np
import pytest

import nwwav_ref as ref
from test_gpu_device_streams import Case, _ok, _run_on_busy_stream, _warm, delay  # noqa: F401  (delay is a fixture)
from test_gpu_nwwav import host_order, make_bank

pytestmark = pytest.mark.gpu


def bank_case():
    import torch
    from vgaudio_amd import _lib
    from vgaudio_amd.nwwav import NwWaveBank
    files = make_bank(5, 48, [None] * 5 + [40000])
    bank = NwWaveBank([img for img, _ in files])
    assert bank.adpcm_bytes and bank.pcm16_samples and bank.pcm8_bytes
    d_adpcm = torch.zeros(bank.adpcm_bytes, dtype=torch.uint8, device="cuda")
    d_pcm16 = torch.zeros(bank.pcm16_samples, dtype=torch.int16, device="cuda")
    d_pcm8 = torch.zeros(bank.pcm8_bytes, dtype=torch.uint8, device="cuda")
    want = [np.zeros(bank.pcm8_bytes, np.uint8), np.zeros(bank.pcm16_samples * 2, np.uint8), np.zeros(bank.adpcm_bytes, np.uint8)]
    r = 0
    for img, _ in files:
        s = ref.read_image(img)
        for c in range(s["nch"]):
            a = host_order(s, c)
            at = int(bank.offsets[r]) * (2 if s["codec"] == ref.PCM16 else 1)
            want[s["codec"]][at:at + len(a)] = a
            r += 1

    def call(stream):
        return _lib.lib().vga_nwwav_bank_read_device(bank._h, bank.d_files.data_ptr(), d_adpcm.data_ptr(), d_pcm16.data_ptr(),
                                                     d_pcm8.data_ptr(), stream)

    def check():
        assert np.array_equal(d_pcm8.cpu().numpy(), want[0])
        assert np.array_equal(d_pcm16.cpu().numpy().view(np.uint8), want[1])
        assert np.array_equal(d_adpcm.cpu().numpy(), want[2])

    return Case([bank.d_files], [d_adpcm, d_pcm16, d_pcm8], call, check), bank


def test_bank_read_on_a_busy_stream(delay):
    import torch
    case, bank = bank_case()
    S = torch.cuda.Stream()
    _warm(case, S)
    rc = _run_on_busy_stream("vga_nwwav_bank_read_device", case, S, delay)
    S.synchronize()
    _ok(rc)
    case.check()
    bank.close()

