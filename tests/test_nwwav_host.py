"""vga_nwwav_parse / vga_nwwav_read (include/vgaudio_hip_nwwav.h) on the host: RWAV, CWAV, FWAV, CSTP and FSTP images
laid out by tests/nwwav_ref.py, every field and every channel's bytes against its restated reference reader.  CPU only;
the bank calls need a device and are in tests/test_gpu_nwwav.py."""
import ctypes as C
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

import nwwav_ref as ref
from vgaudio_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = _lib.VGA_ERR_INVALID_DATA


def payload(rng):
    """GC-ADPCM payloads and coefficients from the CPU oracle"""
    from oracle import pyoracle

    def make(n, h1, h2):
        pcm = rng.integers(-8000, 8000, n, dtype=np.int16)
        coefs = pyoracle.gc_calculate_coefficients(pcm) if n else np.zeros(16, dtype=np.int16)
        return pyoracle.gc_encode(pcm, coefs, hist1=h1, hist2=h2).tobytes(), coefs
    return make


def parse(img):
    buf = np.frombuffer(bytes(img), dtype=np.uint8) if len(img) else np.zeros(1, dtype=np.uint8)
    info = _lib.NwWavInfoC()
    rc = _lib.lib().vga_nwwav_parse(buf.ctypes.data_as(_lib.u8p), len(img), C.byref(info))
    return rc, info, _lib.lib().vga_last_error().decode()


def read(img, info):
    buf = np.frombuffer(bytes(img), dtype=np.uint8)
    outs = [np.zeros(info.channel_bytes, dtype=np.uint8) for _ in range(info.channel_count)]
    ptrs = (_lib.u8p * len(outs))(*[o.ctypes.data_as(_lib.u8p) for o in outs])
    assert _lib.lib().vga_nwwav_read(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info), ptrs) == 0
    return [o.tobytes() for o in outs]


def files(seed, count, **kw):
    rng = np.random.default_rng(seed)
    make = payload(rng)
    return [ref.random_file(rng, make, **kw) for _ in range(count)]


def check_fields(img, given):
    s = ref.read_image(img)
    rc, I, msg = parse(img)
    assert rc == 0, msg
    assert (I.kind, I.endianness, I.version, I.file_size) == (s["kind"], int(s["big"]), s["version"], s["file_size"])
    assert (I.codec, I.looping, I.loop_start, I.sample_count, I.sample_rate, I.channel_count) == \
        (s["codec"], int(s["looping"]), s["loop_start"], s["sample_count"], s["sample_rate"], s["nch"])
    assert I.channel_bytes == ref.samples_to_bytes(s["sample_count"], s["codec"]) == len(s["audio"][0])
    assert (I.has_loop_start_unaligned, I.loop_start_unaligned) == \
        ((1, s["loop_start_unaligned"]) if "loop_start_unaligned" in s else (0, 0))
    nch = s["nch"]
    if s["codec"] == ref.GCADPCM:
        for c, ch in enumerate(s["channels"][:nch]):
            assert list(I.coefs[c]) == ch["coefs"] and I.gain[c] == ch["gain"]
            assert list(I.start_context[c]) == ch["start"] and list(I.loop_context[c]) == ch["loop"]
    else:
        assert not any(any(I.coefs[c]) or I.gain[c] or any(I.start_context[c]) or any(I.loop_context[c]) for c in range(nch))
    if s["kind"] >= ref.CSTP:
        first = s["regions"][0]
        assert (I.prefetch_count, I.prefetch_start_sample, I.prefetch_size, I.prefetch_audio_offset) == \
            (len(s["regions"]), first["start_sample"], first["size"], first["audio"])
        assert (I.stream_looping, I.stream_sample_count) == (int(s["stream_looping"]), s["stream_sample_count"])
        for k in ("interleave_count", "interleave_size", "samples_per_interleave", "last_block_size_without_padding",
                  "last_block_samples", "last_block_size"):
            assert getattr(I, k) == s[k], k
    else:
        assert list(I.audio_offset[:nch]) == s["audio_offsets"]
        assert I.prefetch_count == I.prefetch_size == I.interleave_size == 0
    # and against what the builder was given
    assert (s["kind"], s["codec"], s["nch"], s["sample_count"], s["sample_rate"], s["looping"]) == \
        (given["kind"], given["codec"], given["nch"], given["sample_count"], given["sample_rate"], given["looping"])
    assert read(img, I) == s["audio"] == given["audio"]
    return I


@pytest.mark.parametrize("kind", range(5))
def test_parse_and_read_random_files(kind):
    seen = set()
    for img, given in files(100 + kind, 60, kind=kind):
        I = check_fields(img, given)
        seen.add((I.codec, I.endianness, I.has_loop_start_unaligned, min(I.channel_count, 2), I.looping))
    assert {c for c, *_ in seen} == {0, 1, 2}
    if kind in (ref.CWAV, ref.FWAV):
        assert {(e, u) for _, e, u, *_ in seen} == {(0, 0), (0, 1), (1, 0), (1, 1)}   # both byte orders, both sides of the version
    if kind >= ref.CSTP:
        assert {e for _, e, *_ in seen} == {0, 1}


def test_every_channel_count_and_source_alignment():
    rng = np.random.default_rng(7)
    make = payload(rng)
    for nch in range(1, 9):
        for kind in range(5):
            for align in (0, 5, 15):
                img, given = ref.random_file(rng, make, kind=kind, nch=nch, gaps=[align] * nch)
                check_fields(img, given)


def test_empty_and_one_sample_files():
    rng = np.random.default_rng(8)
    make = payload(rng)
    for kind in range(5):
        for codec in range(3):
            for n in (0, 1, 13, 14, 15):
                check_fields(*ref.random_file(rng, make, kind=kind, codec=codec, n=n))


def test_prefetch_reads_the_first_of_several_regions_and_a_short_last_block():
    rng = np.random.default_rng(9)
    chans = [rng.integers(0, 256, 100, dtype=np.uint8).tobytes() for _ in range(3)]
    later = [bytes(40)] * 3
    img = ref.build_prefetch(ref.FSTP, True, 0x00040000, ref.PCM8, 32000, [(77, chans), (500, later)], 32, nch=3, gap=5)
    rc, I, msg = parse(img)
    assert rc == 0, msg
    assert (I.prefetch_count, I.prefetch_start_sample, I.prefetch_size, I.sample_count, I.looping) == (2, 77, 300, 100, 0)
    assert read(img, I) == chans                              # blocks of 32, 32, 32 and 4 bytes per channel
    assert ref.read_image(img)["audio"] == chans


def _wave(kind=ref.CWAV, big=False, nch=2, n=50, codec=ref.PCM16):
    rng = np.random.default_rng(3)
    return ref.random_file(rng, payload(rng), kind=kind, codec=codec, nch=nch, n=n, big=big)[0]


def _patched(img, at, data):
    b = bytearray(img)
    b[at:at + len(data)] = data
    return bytes(b)


def test_reject_paths_carry_the_references_messages():
    cwav, rwav, cstp = _wave(), _wave(ref.RWAV), _wave(ref.CSTP, codec=ref.GCADPCM)
    info_off, data_off = struct.unpack_from("<i", cwav, 0x18)[0], struct.unpack_from("<i", cwav, 0x24)[0]
    rinfo, rdata = struct.unpack_from(">i", rwav, 0x10)[0], struct.unpack_from(">i", rwav, 0x18)[0]
    cases = [
        (_patched(cwav, 0, b"XWAV"), "File has no CSTM or FSTM header"),
        (_patched(rwav, 0, b"RWAX"), "File has no RWAV header"),
        (_patched(cwav, 4, b"\x00\x00"), "File has no byte order mark"),
        (_patched(rwav, 4, b"\xff\xfe"), "Expected 65279, but got 65534 at offset 0x4"),
        (cwav[:-1], "Actual file length is less than stated length"),
        (rwav[:-1], "Actual file length is less than stated length"),
        (_patched(cwav, 0x14, struct.pack("<H", 0x4001)), "File has no INFO block"),
        (_patched(cwav, info_off, b"INFX"), "Unknown or invalid INFO block"),
        (_patched(rwav, rinfo, b"INFX"), "Unknown or invalid INFO block"),
        (_patched(cwav, info_off + 4, b"\x01\x00\x00\x00"), "INFO block size in main header doesn't match size in INFO header"),
        (_patched(rwav, rinfo + 4, b"\x00\x00\x00\x01"), "HEAD block size in RWAV header doesn't match size in HEAD header"),
        (_patched(cwav, 0x20, struct.pack("<H", 0x4001)), "Unknown or invalid SEEK block"),   # the DATA entry becomes a SEEK one
        (_patched(cwav, 0x20, struct.pack("<H", 0x1234)), "File has no DATA block"),
        (_patched(cwav, data_off, b"DATX"), "Unknown or invalid DATA block"),
        (_patched(rwav, rdata, b"DATX"), "Unknown or invalid DATA block"),
        (_patched(cwav, data_off + 4, b"\x01\x00\x00\x00"), "DATA block size in main header doesn't match size in DATA header"),
        (_patched(rwav, rdata + 4, b"\x00\x00\x00\x01"), "DATA block size in main header doesn't match size in DATA header"),
    ]
    pinfo, pdat = struct.unpack_from("<i", cstp, 0x18)[0], struct.unpack_from("<i", cstp, 0x24)[0]
    cases += [
        (_patched(cstp, pinfo + 8, b"\x00\x00"), "Could not read stream info."),
        (_patched(cstp, pinfo + 24, b"\x00\x00"), "Could not read channel info."),
        (_patched(cstp, pdat + 8, struct.pack("<i", 0)), "the prefetch block holds no region"),
        (_patched(cstp, pdat + 8, struct.pack("<i", 1 << 20)), "file ends inside the prefetch regions"),
        (_patched(cstp, pdat + 16, struct.pack("<i", 1 << 24)), "Specified length is greater than the number of bytes remaining in the Stream"),
    ]
    for img, message in cases:
        rc, _, msg = parse(img)
        assert rc == INVALID and msg == message, (rc, msg, message)
    for magic in (b"RSTM", b"CSTM", b"FSTM"):
        rc, _, msg = parse(_patched(cwav, 0, magic))
        assert rc == _lib.VGA_ERR_INVALID_OP and "vga_nwstm_parse" in msg
    assert parse(b"")[0] == INVALID and parse(b"CWA")[0] == INVALID


def test_offsets_outside_the_image_are_invalid_data():
    cwav = _wave(nch=2, n=4000)
    rc, I, _ = parse(cwav)
    assert rc == 0
    info_off = struct.unpack_from("<i", cwav, 0x18)[0]
    assert parse(_patched(cwav, info_off + 8 + 12, struct.pack("<i", 1 << 28)))[0] == INVALID     # sample count
    assert parse(_patched(cwav, info_off + 8 + 12, struct.pack("<i", -5)))[0] == INVALID
    assert parse(_patched(cwav, info_off + 8 + 20, struct.pack("<i", 3)))[0] == INVALID           # more channels than offsets
    assert parse(_patched(cwav, info_off + 8 + 20, struct.pack("<i", 1 << 20)))[0] == INVALID
    assert parse(_patched(cwav, info_off + 8 + 20, struct.pack("<i", 0)))[0] == INVALID
    assert parse(_patched(cwav, info_off + 8, b"\x07"))[0] == INVALID                             # codec


def test_the_stream_parser_still_refuses_what_the_wave_parser_reads():
    """vga_nwstm_parse keeps its answer for wave and prefetch files; vga_nwwav_parse is a family of its own"""
    cwav = _wave()
    buf = np.frombuffer(cwav, dtype=np.uint8)
    old = _lib.NwInfoC()
    assert _lib.lib().vga_nwstm_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(old)) == _lib.VGA_ERR_INVALID_OP
    assert "are not read here" in _lib.lib().vga_last_error().decode()
    assert parse(cwav)[0] == 0
    rwav = np.frombuffer(_wave(ref.RWAV), dtype=np.uint8)
    assert _lib.lib().vga_nwstm_parse(rwav.ctypes.data_as(_lib.u8p), len(rwav), C.byref(old)) == INVALID
    assert parse(rwav.tobytes())[0] == 0


def test_truncations_and_corruptions_through_the_library():
    rng = np.random.default_rng(11)
    for img, _ in files(12, 25, n=200):
        for _ in range(40):
            assert parse(img[:int(rng.integers(0, len(img)))])[0] in (0, INVALID)
            bad = bytearray(img)
            bad[int(rng.integers(0, len(img)))] = int(rng.integers(0, 256))
            rc, I, _msg = parse(bytes(bad))
            assert rc in (0, INVALID)
            if rc == 0:
                read(bad, I)


def test_parser_under_address_sanitizer(tmp_path):
    """random truncations and single-byte corruptions never read outside the image: the parser alone, compiled for the
    host with AddressSanitizer, over heap blocks of exactly the image's size"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    exe = str(tmp_path / "nwwav_parse_fuzz")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "host", "nwwav_parse_fuzz.cpp"), "-o", exe], check=True)
    corpus = tmp_path / "images.bin"
    with open(corpus, "wb") as f:
        for img, _ in files(13, 60, n=150):
            f.write(struct.pack("<I", len(img)) + img)
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(corpus), "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    parsed, rejected = (int(v) for v in r.stdout.split()[:2])
    assert parsed > 60 and rejected > 1000
