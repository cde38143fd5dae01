"""vga_nwwav_bank_* on the device (include/vgaudio_hip_nwwav.h): banks of RWAV / CWAV / FWAV / CSTP / FSTP images built by
tests/nwwav_ref.py go from one device buffer to the packed GC-ADPCM / PCM16 / PCM8 layouts in one launch.  Everything is
compared byte for byte with the restated reference reader, and the decoded GC-ADPCM rows with the CPU oracle's decoder:
the feature moves bytes, so there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import nwwav_ref as ref
from test_nwwav_host import payload

pytestmark = pytest.mark.gpu

CANARY = 4096                                     # bytes on each side of every output
GUARD = 256


def make_bank(seed, count, lengths=None, **kw):
    rng = np.random.default_rng(seed)
    make = payload(rng)
    out = []
    for i in range(count):
        if lengths is not None:
            kw["n"] = lengths[i % len(lengths)]
        out.append(ref.random_file(rng, make, **kw))
    return out


def host_order(s, c):
    """channel c of a restated structure as the bank stores it: PCM16 in host order, the rest as in the file"""
    a = np.frombuffer(s["audio"][c], dtype=np.uint8)
    if s["codec"] == ref.PCM16 and s["big"]:
        a = a.reshape(-1, 2)[:, ::-1].reshape(-1)
    return a


def read_with_canaries(bank):
    """vga_nwwav_bank_read_device into buffers with CANARY bytes around them -> three host arrays (canaries checked)"""
    import torch
    from vgaudio_amd import _lib
    sizes = (bank.pcm8_bytes, bank.pcm16_samples * 2, bank.adpcm_bytes)       # by NwCodec
    bufs = [torch.full((CANARY + s + CANARY,), 0xC7, dtype=torch.uint8, device="cuda") for s in sizes]
    ptr = [b.data_ptr() + CANARY if s else None for b, s in zip(bufs, sizes)]
    assert all(p is None or p % 16 == 0 for p in ptr)
    _lib.check(_lib.lib().vga_nwwav_bank_read_device(bank._h, bank.d_files.data_ptr(), ptr[2], ptr[1], ptr[0],
                                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = []
    for b, s in zip(bufs, sizes):
        h = b.cpu().numpy()
        assert (h[:CANARY] == 0xC7).all() and (h[CANARY + s:] == 0xC7).all(), "a byte outside an output was written"
        out.append(h[CANARY:CANARY + s])
    return out


def check_bank(files, align=1):
    """every row against the restated reader; every other byte of the outputs is zero"""
    from vgaudio_amd.nwwav import NwWaveBank
    bank = NwWaveBank([img for img, _ in files], align=align)
    structs = [ref.read_image(img) for img, _ in files]
    outs = read_with_canaries(bank)
    assert bank.channels == sum(s["nch"] for s in structs)
    covered = [np.zeros(len(o), dtype=bool) for o in outs]
    r = 0
    for f, s in enumerate(structs):
        for c in range(s["nch"]):
            assert (bank.file[r], bank.channel[r], bank.codec[r], bank.sample_counts[r]) == (f, c, s["codec"], s["sample_count"])
            want = host_order(s, c)
            at = int(bank.offsets[r]) * (2 if s["codec"] == ref.PCM16 else 1)
            assert at % 16 == 0
            got = outs[s["codec"]][at:at + len(want)]
            assert np.array_equal(got, want), f"file {f} (kind {s['kind']}) channel {c}: {int((got != want).sum())} bytes differ"
            covered[s["codec"]][at:at + len(want)] = True
            r += 1
    for o, cov in zip(outs, covered):
        assert not o[~cov].any(), "round-up padding or guard bytes are not zero"
    if bank.gc_channels:
        assert not outs[2][-GUARD:].any() and not covered[2][-GUARD:].any()
    bank.close()
    return bank, structs, outs


def test_random_bank_of_mixed_files():
    # 0 samples, rows under 16 bytes, rows around one and two pieces of 16 KiB for every codec, a few long ones
    lengths = [0, 1, 5, 13, 14, 27] + [None] * 14 + [8190, 16384, 16385, 18724, 28672, 28673, 32768, 37449, 57344] + [None] * 7
    files = make_bank(21, 260, lengths)
    rng = np.random.default_rng(22)
    make = payload(rng)
    for n, kind, codec in ((300000, ref.RWAV, ref.GCADPCM), (450000, ref.FWAV, ref.GCADPCM), (250001, ref.CWAV, ref.PCM16),
                           (333333, ref.RWAV, ref.PCM8), (120000, ref.FSTP, ref.GCADPCM), (90001, ref.CSTP, ref.PCM16)):
        files.insert(int(rng.integers(0, len(files))), ref.random_file(rng, make, kind=kind, codec=codec, n=n, nch=int(rng.integers(1, 3))))
    bank, structs, _ = check_bank(files)
    assert {s["kind"] for s in structs} == set(range(5)) and {s["codec"] for s in structs} == {0, 1, 2}
    assert {s["big"] for s in structs if s["codec"] == ref.PCM16} == {False, True}
    # every source alignment, for every codec, among the plain (wave) rows
    for codec in range(3):
        seen = {(int(bank.file_offsets[f]) + o) % 16 for f, s in enumerate(structs) if s["codec"] == codec and s["kind"] < ref.CSTP
                for o in s["audio_offsets"]}
        assert seen == set(range(16)), (codec, seen)


@pytest.mark.parametrize("align", [1, 16, 64])
def test_file_alignment_in_the_buffer(align):
    check_bank(make_bank(30 + align, 40), align=align)


def test_gc_rows_are_the_ragged_decoders_layout():
    """the GC-ADPCM rows sit at vga_gcadpcm_ragged_offsets of their sample counts, the sizes agree"""
    from vgaudio_amd import _lib
    from vgaudio_amd.nwwav import NwWaveBank
    files = make_bank(41, 80)
    bank = NwWaveBank([img for img, _ in files])
    L = _lib.lib()
    counts = [s for s, c in zip(bank.sample_counts, bank.codec) if c == ref.GCADPCM]
    assert list(bank.gc_sample_counts) == counts and bank.gc_channels == len(counts) > 10
    ragged = C.c_void_p()
    _lib.check(L.vga_gcadpcm_ragged_create((C.c_int * len(counts))(*counts), len(counts), C.byref(ragged)))
    offs = np.zeros(len(counts), dtype=np.int64)
    _lib.check(L.vga_gcadpcm_ragged_offsets(ragged, None, offs.ctypes.data_as(C.POINTER(C.c_int64))))
    assert list(offs) == [int(o) for o, c in zip(bank.offsets, bank.codec) if c == ref.GCADPCM]
    assert L.vga_gcadpcm_ragged_adpcm_bytes(ragged) == bank.adpcm_bytes
    assert L.vga_gcadpcm_ragged_channels(ragged) == L.vga_nwwav_bank_codec_channels(bank._h, ref.GCADPCM)
    L.vga_gcadpcm_ragged_destroy(ragged)
    structs = [ref.read_image(img) for img, _ in files]
    gc = [ch for s in structs if s["codec"] == ref.GCADPCM for ch in s["channels"][:s["nch"]]]
    assert bank.gc_coefs.tolist() == [ch["coefs"] for ch in gc]
    assert bank.gc_hist1.tolist() == [ch["start"][1] for ch in gc] and bank.gc_hist2.tolist() == [ch["start"][2] for ch in gc]
    assert bank.gc_gain.tolist() == [ch["gain"] for ch in gc]
    bank.close()


def test_bank_read_then_decode_against_the_oracle():
    from oracle import pyoracle
    from vgaudio_amd.nwwav import NwWaveBank
    files = make_bank(51, 120, [None] * 9 + [20000, 16384 * 2, 70001])
    bank = NwWaveBank([img for img, _ in files])
    pcm = bank.decode_to_pcm16()
    seen = set()
    for f, (img, given) in enumerate(files):
        s = ref.read_image(img)
        assert len(pcm[f]) == s["nch"]
        for c in range(s["nch"]):
            if s["codec"] == ref.GCADPCM:
                ch = s["channels"][c]
                want = pyoracle.gc_decode(np.frombuffer(s["audio"][c], dtype=np.uint8), np.array(ch["coefs"], dtype=np.int16),
                                          s["sample_count"], ch["start"][1], ch["start"][2])
            elif s["codec"] == ref.PCM16:                       # the builder's input, read in the file's byte order
                want = np.frombuffer(given["audio"][c], dtype=">i2" if s["big"] else "<i2").astype(np.int16)
            else:                                               # Pcm8Codec.DecodeSigned
                want = np.frombuffer(given["audio"][c], dtype=np.int8).astype(np.int16) << 8
            assert pcm[f][c].dtype == np.int16 and np.array_equal(pcm[f][c], want), (f, c, s["kind"], s["codec"])
            seen.add(s["codec"])
    assert seen == {0, 1, 2}
    bank.close()


@pytest.mark.parametrize("kind", range(5))
@pytest.mark.parametrize("codec", range(3))
def test_bank_of_one_file(kind, codec):
    check_bank(make_bank(60 + kind * 3 + codec, 1, kind=kind, codec=codec))


@pytest.mark.parametrize("kind,codec,nch,n", [(ref.RWAV, ref.GCADPCM, 2, 30000), (ref.CWAV, ref.PCM16, 1, 4099),
                                              (ref.FSTP, ref.GCADPCM, 3, 9000), (ref.CSTP, ref.PCM8, 2, 5001)])
def test_bank_of_equally_shaped_files_matches_reading_each_file(kind, codec, nch, n):
    """one shape throughout, as the batched stream readers take: the bank's bytes are those of one read per file"""
    from test_nwwav_host import parse, read
    files = make_bank(70 + kind, 12, kind=kind, codec=codec, nch=nch, n=n, big=kind != ref.CWAV)
    bank, structs, outs = check_bank(files)
    r = 0
    for img, _ in files:
        rc, info, _msg = parse(img)
        assert rc == 0
        for row in read(img, info):
            want = np.frombuffer(row, dtype=np.uint8)
            if codec == ref.PCM16 and info.endianness == 1:
                want = want.reshape(-1, 2)[:, ::-1].reshape(-1)
            at = int(bank.offsets[r]) * (2 if codec == ref.PCM16 else 1)
            assert np.array_equal(outs[codec][at:at + len(want)], want)
            r += 1


def test_argument_errors():
    import torch
    from vgaudio_amd import _lib
    from vgaudio_amd.nwwav import NwWaveBank
    L = _lib.lib()
    with pytest.raises(_lib.ArgumentError):
        NwWaveBank([])                                           # an empty bank
    h = C.c_void_p()
    assert L.vga_nwwav_bank_create(None, None, 3, C.byref(h)) == _lib.VGA_ERR_ARGUMENT and not h
    infos = (_lib.NwWavInfoC * 1)()                              # an info nothing parsed
    assert L.vga_nwwav_bank_create(infos, (C.c_int64 * 1)(0), 1, C.byref(h)) == _lib.VGA_ERR_ARGUMENT
    files = make_bank(80, 6)
    bank = NwWaveBank([img for img, _ in files])
    d = torch.zeros(max(bank.adpcm_bytes, bank.pcm16_samples * 2, bank.pcm8_bytes) + 64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    assert L.vga_nwwav_bank_read_device(None, bank.d_files.data_ptr(), p, p, p, s) == _lib.VGA_ERR_ARGUMENT
    assert L.vga_nwwav_bank_read_device(bank._h, None, p, p, p, s) == _lib.VGA_ERR_ARGUMENT
    assert L.vga_nwwav_bank_read_device(bank._h, bank.d_files.data_ptr(), p + 8, p, p, s) == _lib.VGA_ERR_ARGUMENT
    if bank.adpcm_bytes:
        assert L.vga_nwwav_bank_read_device(bank._h, bank.d_files.data_ptr(), None, p, p, s) == _lib.VGA_ERR_ARGUMENT
    torch.cuda.synchronize()
    bank.close()


def test_python_readers_return_the_formats():
    from vgaudio_amd import _lib
    from vgaudio_amd.gcadpcm import GcAdpcmFormat, Pcm16Format
    from vgaudio_amd.nwwav import BCFwavReader, BrwavReader
    from vgaudio_amd.pcm8 import Pcm8SignedFormat
    for kind in range(5):
        for codec, cls in ((ref.GCADPCM, GcAdpcmFormat), (ref.PCM16, Pcm16Format), (ref.PCM8, Pcm8SignedFormat)):
            img, given = make_bank(90 + kind, 1, kind=kind, codec=codec, n=500)[0]
            reader = BrwavReader() if kind == ref.RWAV else BCFwavReader()
            fmt = reader.ReadFormat(img)
            assert isinstance(fmt, cls) and len(fmt.Channels) == given["nch"] and fmt.SampleRate == given["sample_rate"]
            assert bool(fmt.Looping) == given["looping"]
            with pytest.raises(_lib.InvalidDataError):
                (BCFwavReader() if kind == ref.RWAV else BrwavReader()).ReadFormat(img)
