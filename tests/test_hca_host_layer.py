"""The HIP-free HCA host layer (vgaudio_amd/csrc/hca_host.hpp) on its own: tests/host/hca_host_driver.cpp includes the
header with a set_error of its own and is built twice with g++.  As a shared library its results are compared with the
loaded product library's, with the parent's order of status tests and with pyref's streaming shell; as a stand-alone
program under AddressSanitizer and UBSan it runs the table of tests/hca_init_cases.py and the headers the decoder must
refuse (tests/hca_headers_ref.py) as a child process.  CPU only."""
import ctypes as C
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hca_headers_ref as hh
import hca_init_cases as T
import test_hca_ragged_decode_host as ragged
from oracle.pyref import crihca as pyref
from vgaudio_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "hca_host_driver.cpp")
CSRC = os.path.join(HERE, "..", "vgaudio_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("hca_host.hpp", "hca_info.hpp", "hca_tables_host.inc")]
SO = os.path.join(HERE, "host", "libhca_host_driver.so")
# as the product is built (vgaudio_amd/build.py): C# int arithmetic wraps, nothing contracts into an FMA
FLAGS = ["-std=c++17", "-Wall", "-fwrapv", "-ffp-contract=off", "-fno-fast-math"]
DEVICE_INFO_BYTES = 44 + 32 + 32 + 128
CASES = T.cases() + [T.NEGATIVE_COUNT]

ARG, RANGE, DATA, OP, DEVICE = (_lib.VGA_ERR_ARGUMENT, _lib.VGA_ERR_OUT_OF_RANGE, _lib.VGA_ERR_INVALID_DATA,
                                _lib.VGA_ERR_INVALID_OP, _lib.VGA_ERR_DEVICE)
# headers the decoder is handed by files, and the code make_device_info gave for each on the parent of the change that
# moved it into the header (0: the reference decodes them, CriHcaDecoder.cs:119, :149)
HOSTILE = [
    (hh.dec("negative_stereo", 2, total=50, base=60), 0),
    (hh.dec("negative_stereo_mono", 1, total=50, base=60), 0),
    (hh.comp("bands_beyond_total", 2, total=20, base=25, stereo=4, per_hfr=8), 0),
    (hh.comp("coded_above_128", 2, total=128, base=120, stereo=20), RANGE),
    (hh.comp("tracks_with_stereo", 4, tracks=2, stereo=20), RANGE),
    (hh.comp("hfr_groups_9", 2, total=128, base=20, stereo=0, per_hfr=12), ARG),
    (hh.comp("frame_size_7", 2, fs=7, direct=True), ARG),
    (hh.comp("frame_size_0x10000", 2, fs=0x10000, direct=True), ARG),
]
# status_to_error in the parent's order of tests: 16, 4, 8, 1, 32, 2
STATUS = [
    (1, DATA, "Invalid frame header"),
    (2, DATA, "scale-factor delta out of range (frame state would be stale in the reference)"),
    (4, DATA, "Bitrate is set too low."),
    (8, OP, "evaluation boundary search failed (NotImplementedException in the reference)"),
    (16, DEVICE, "internal: the encoder's bit-cost table could not be built"),
    (32, RANGE, "Index was outside the bounds of the array (intensity 15)"),
    (1 | 32, DATA, "Invalid frame header"),
    (1 | 2, DATA, "Invalid frame header"),
]


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + [SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.hh_last_error.restype = C.c_char_p
    L.hh_encoder_initialize.argtypes = [vp, vp]
    L.hh_make_device_info.argtypes = [vp, vp, C.c_int]
    L.hh_decode_classes.argtypes = [vp, C.c_int, ip]
    L.hh_stream_counts.argtypes = [vp, ip, C.c_int]
    L.hh_bitrate_too_low.argtypes = [vp]
    L.hh_frames_pitch.argtypes = [vp]
    L.hh_frames_pitch.restype = C.c_longlong
    return L


def product_init(p):
    cp, h = _lib.HcaParamsC(*p), _lib.HcaInfoC()
    rc = _lib.lib().vga_hca_encoder_initialize(C.byref(cp), C.byref(h))
    return rc, h, _lib.lib().vga_last_error().decode() if rc else ""


def host_init(host, p):
    cp, h = _lib.HcaParamsC(*p), _lib.HcaInfoC()
    rc = host.hh_encoder_initialize(C.byref(cp), C.byref(h))
    return rc, h, host.hh_last_error().decode() if rc else ""


def both_device_infos(host, h):
    """((rc, message, bytes) of the product, the same of the header)"""
    a, b = (C.c_uint8 * DEVICE_INFO_BYTES)(), (C.c_uint8 * DEVICE_INFO_BYTES)()
    rca = _lib.lib().vga_testing_hca_device_info(C.byref(h), a, DEVICE_INFO_BYTES)
    rcb = host.hh_make_device_info(C.byref(h), b, DEVICE_INFO_BYTES)
    return ((rca, _lib.lib().vga_last_error().decode() if rca else "", bytes(a)),
            (rcb, host.hh_last_error().decode() if rcb else "", bytes(b)))


def both_classes(host, infos):
    arr = (_lib.HcaInfoC * max(len(infos), 1))(*infos)
    out = (C.c_int * max(len(infos), 1))()
    n = host.hh_decode_classes(arr, len(infos), out)
    return ragged.classes(infos), (n, list(out[:len(infos)]))


def hostile_info(header):
    info = _lib.HcaInfoC()
    for k, v in header.expected().items():
        setattr(info, k, v)
    return info


def test_initialize_and_device_info_equal_the_product_librarys(host):
    good = []
    for p in CASES:
        want, got = product_init(p), host_init(host, p)
        assert (got[0], got[2], bytes(got[1])) == (want[0], want[2], bytes(want[1])), p
        if want[0]:
            continue
        product, header = both_device_infos(host, want[1])
        assert header == product, p
        if product[0] == 0:
            good.append(want[1])
    assert len(good) > 300
    product, header = both_classes(host, good)
    assert header == product and product[0] > 10


def test_hostile_headers_are_refused_with_the_products_codes(host):
    for header, code in HOSTILE:
        product, mine = both_device_infos(host, hostile_info(header))
        assert product[0] == code and mine == product, header


def test_classes_of_the_ragged_decoders_stream_sets(host):
    info = ragged.info
    sets = [[info(n=n) for n in (1, 1000, 1024, 48000, 48001, 2_880_000)],
            [info(n=50_000), info(n=50_000, loop=(3000, 40_000))],
            [info(), info(quality="Middle"), info(quality="Highest"), info(nch=1), info(nch=6)],
            [info(quality="Low"), info(quality="Low"), info(), info(nch=1), info(), info(quality="Low"), info(nch=1),
             info(quality="Low", n=77)],
            []]
    ath = [_lib.HcaInfoC.from_buffer_copy(info(rate=r)) for r in (48000, 44100, 32000)]
    for h in ath:
        h.use_ath_curve = 1
    sets.append(ath + [info(rate=r) for r in (48000, 44100, 32000)])
    rng = np.random.default_rng(3)                            # the streams of test_classes_are_the_rule_as_stated
    rule = []
    for _ in range(120):
        n = int(rng.integers(1, 400_000))
        loop = None
        if rng.random() < 0.3 and n > 10:
            a = int(rng.integers(0, n - 1))
            loop = (a, int(rng.integers(a + 1, n + 1)))
        h = info(nch=int(rng.choice([1, 2, 2, 3, 4, 6, 8])), n=n, rate=int(rng.choice([48000, 44100, 22050])),
                 quality=str(rng.choice(list(ragged.QUALITY))), loop=loop)
        if rng.random() < 0.2:
            h.use_ath_curve = 1
        rule.append(h)
    sets.append(rule)
    for infos in sets:
        product, header = both_classes(host, infos)
        assert header == product, len(infos)
    assert both_classes(host, sets[3])[1] == (3, [0, 0, 1, 2, 1, 0, 2, 0])
    bad = info()
    bad.channel_count = 9                                     # refused as vga_testing_hca_decode_classes refuses it
    product, header = both_classes(host, [info(), bad])
    assert header[0] == product[0] == ARG


def test_status_to_error_keeps_the_parents_order(host):
    assert host.hh_status_to_error(0) == 0
    for status, code, message in STATUS:
        assert (host.hh_status_to_error(status), host.hh_last_error().decode()) == (code, message), status


def test_the_shared_rules(host):
    """the bit budget and the frames pitch, once: against the expressions the call sites held"""
    for p in CASES:
        rc, h, _ = product_init(p)
        if rc:
            continue
        low = h.frame_size * 8 < 48 + 3 * h.channel_count + 16
        assert host.hh_bitrate_too_low(C.byref(h)) == int(low), p
        assert host.hh_frames_pitch(C.byref(h)) == (h.frame_count * h.frame_size + 8 + 15) // 16 * 16, p
    for nch in (0, 9, -1):                                   # not this rule's to refuse: make_device_info's VGA_ERR_ARGUMENT
        h = ragged.info()
        h.channel_count, h.frame_size = nch, 1
        assert host.hh_bitrate_too_low(C.byref(h)) == 0
        assert both_device_infos(host, h)[1][0] == ARG


# (nch, samples, quality, loop): what the streaming shell's counters are walked over
STREAMS = [
    (1, 1, "High", None), (1, 1024, "High", None), (1, 1025, "High", None), (2, 5000, "High", None),
    (2, 99_999, "Lowest", (0, 50_000)),                      # frames of 256 bytes: the loop padding inserts 7 frames
    (2, 20_000, "High", (3000, 12_000)),                     # loop_end < sample_count
]


def pyref_frames_per_call(nch, n, quality, loop):
    """oracle.pyref.crihca.Encoder.encode with encode_frame stubbed: its counters alone"""
    kw = dict(looping=True, loop_start=loop[0], loop_end=loop[1]) if loop else {}
    enc = pyref.Encoder(pyref.Params(nch, 48000, n, quality=quality, **kw))
    enc.encode_frame = lambda pcm: b""
    block = [[0] * 1024 for _ in range(nch)]
    counts = []
    while enc.frames_processed < enc.hca.frame_count:
        counts.append(len(enc.encode(block)))
    with pytest.raises(RuntimeError):
        enc.encode(block)
    return enc.hca, counts


@pytest.mark.parametrize("nch,n,quality,loop", STREAMS)
def test_stream_counters_walk_like_the_references_encoder(host, nch, n, quality, loop):
    want_info, want = pyref_frames_per_call(nch, n, quality, loop)
    p = (ragged.QUALITY[quality], 0, 0, nch, 48000, n) + ((1,) + loop if loop else (0, 0, 0))
    rc, h, _ = host_init(host, p)
    assert rc == 0 and (h.frame_count, h.inserted_samples, h.sample_count) == \
        (want_info.frame_count, want_info.inserted_samples, want_info.sample_count)
    counts = (C.c_int * (len(want) + 1))()
    host.hh_stream_counts(C.byref(h), counts, len(want) + 1)
    assert list(counts[:len(want)]) == want
    assert sum(want) == h.frame_count and counts[len(want)] == -1      # every frame, then the shell's guard refuses
    if loop == (0, 50_000):
        assert h.inserted_samples > 128 + 2 * 1024 and want[0] > 2


def test_host_layer_under_address_and_ub_sanitizer(tmp_path):
    """the header alone, compiled for the host with AddressSanitizer and UBSan, over the Initialize table (what the product
    library returned, field by field) and the hostile headers (the codes above); a child process"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    exe = str(tmp_path / "hca_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-DHCA_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
                   + FLAGS + [SRC, "-o", exe], check=True)
    cases = tmp_path / "cases.bin"
    refused = 0
    with open(cases, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for p in CASES:
            rc, h, _ = product_init(p)
            refused += rc != 0
            f.write(struct.pack("<10i", *p, rc) + bytes(h))
        f.write(struct.pack("<i", len(HOSTILE)))
        for header, code in HOSTILE:
            f.write(bytes(hostile_info(header)) + struct.pack("<i", code))
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    initialized, refused_there, device_infos = (int(v) for v in r.stdout.split()[:3])
    assert (initialized, refused_there) == (len(CASES) - refused, refused) and device_infos > 300
