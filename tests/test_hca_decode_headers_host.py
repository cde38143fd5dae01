"""HCA headers the encoder never writes (tests/hca_headers_ref.py), on the CPU: the parser's fields against what
HcaReader derives, the C oracle against pyref (the same PCM, or both throw at the same frame), and the decoder's lane
emulator (tests/host/hca_decode_emulator.cpp, built from the kernels' own hca_decode_core.hpp) against the C oracle
bit for bit.  Where the reference throws IndexOutOfRangeException the oracle returns -6, the library
VGA_ERR_OUT_OF_RANGE."""
import ctypes as C

import numpy as np
import pytest

import hca_headers_ref as hh
from oracle import pyoracle as po
from oracle.pyref import crihca as pyref
from test_host_hca_decode_core import DEVICE_INFO_BYTES, emu  # noqa: F401  (fixture)
from vgaudio_amd import _lib

FAMILIES = hh.families()
ORACLE_OUT_OF_RANGE = -6


def parse(img):
    buf = np.frombuffer(bytes(img), np.uint8)
    info = _lib.HcaFileInfoC()
    rc = _lib.lib().vga_hca_parse(buf.ctypes.data_as(_lib.u8p), len(buf), C.byref(info))
    return rc, info


def device_info(info):
    """(rc, DeviceInfo bytes) from the product's vga_testing_hca_device_info"""
    out = (C.c_uint8 * DEVICE_INFO_BYTES)()
    pinfo = _lib.HcaInfoC()
    for name, _ in _lib.HcaInfoC._fields_:
        setattr(pinfo, name, getattr(info, name))
    return _lib.lib().vga_testing_hca_device_info(C.byref(pinfo), out, DEVICE_INFO_BYTES), out


def parse_refusal(e):
    """what vga_hca_parse refuses (include/vgaudio_hip.h), 0 for the rest"""
    if e["frame_count"] > 0 and e["frame_size"] < 2:
        return _lib.VGA_ERR_INVALID_DATA
    if (not 1 <= e["channel_count"] <= 8 or not 8 <= e["frame_size"] <= 0xFFFF or e["total_band_count"] > 128
            or e["base_band_count"] + e["stereo_band_count"] > 128 or e["hfr_group_count"] > 8):
        return _lib.VGA_ERR_INVALID_OP
    return 0


def reference_throws_up_front(e):
    """GetChannelTypes too short for the channels (CriHcaFrame.cs:20-29), or a channel coding more than 128 bands
    (CriHcaPacking.cs:89-95): IndexOutOfRangeException before any PCM"""
    cpt = e["channel_count"] // e["track_count"]
    if e["stereo_band_count"] != 0 and cpt != 1 and cpt < e["channel_count"]:
        return True
    types = hh.channel_types(e)[:e["channel_count"]]
    coded = [e["base_band_count"] if t == pyref.STEREO_SECONDARY else e["base_band_count"] + e["stereo_band_count"] for t in types]
    return max(coded) > 128


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_parse_gives_the_fields_hca_reader_derives(family):
    rng = np.random.default_rng(len(family))
    for h in FAMILIES[family]:
        e = h.expected()
        frames = ref_frames(e, rng)
        rc, I = parse(h.image(frames))
        want = parse_refusal(e)
        assert rc == want, (h, rc, _lib.lib().vga_last_error())
        if rc:
            continue
        for k in hh.FIELDS:
            assert getattr(I.hca, k) == e[k], (h, k, getattr(I.hca, k), e[k])


def ref_frames(e, rng):
    return rng.integers(0, 256, e["frame_count"] * max(e["frame_size"], 0), dtype=np.uint8)


def test_parse_of_frame_sizes_above_32767_is_refused():
    """comp / dec read FrameSize with ReadInt16: 32768..65535 come out negative, and the frames cannot be read"""
    for fs in (0x8000, 0xFFFF):
        for h in (hh.comp("fs", 2, fs=fs), hh.dec("fs", 2, fs=fs)):
            assert h.expected()["frame_size"] < 0
            assert parse(h.image(b""))[0] == _lib.VGA_ERR_INVALID_DATA


def test_negative_hfr_band_counts_round_like_math_ceiling():
    """comp bands past the total: HfrBandCount < 0, HfrGroupCount = ceil(HfrBandCount / BandsPerHfrGroup) rounds towards
    zero (-1 / 8 -> 0, -9 / 8 -> -1) and the frames carry no HFR scales"""
    for (t, b, s, per, groups) in ((20, 15, 6, 8, 0), (20, 25, 4, 8, -1), (20, 30, 0, 1, -10)):
        h = hh.comp("neg", 2, total=t, base=b, stereo=s, per_hfr=per)
        assert h.expected()["hfr_group_count"] == groups
        rc, I = parse(h.image(bytes(h.frame_count * 0x200)))
        assert rc == 0 and I.hca.hfr_group_count == groups and I.hca.hfr_band_count == t - b - s


def _pyref_frames(e):
    return 2 if e["channel_count"] <= 2 else 1


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_oracle_matches_pyref(family):
    """the C oracle and pyref on every header of the family: the same PCM over the first frames, or the same throw at
    the same frame (pyref's IndexError, the oracle's -6, with the frames before it decoded alike)"""
    rng = np.random.default_rng(100 + len(family))
    for k, h in enumerate(FAMILIES[family]):
        e = h.expected()
        if e["frame_size"] < 8 or e["hfr_group_count"] > 8:
            continue
        frames = hh.frames_for(h, rng, "mixed", intensity_max=15 if k % 2 else 14)
        n = _pyref_frames(e)
        status, got = hh.reference_decode(h, frames, n)
        rc, want = hh.oracle_frames(h.info(), frames)
        if status == "IndexError":
            assert rc == ORACLE_OUT_OF_RANGE, (h, got)
            if got > 0:
                assert np.array_equal(want[:, :got * 1024], status_pcm(h, frames, got)), h
        else:
            assert rc in (0, ORACLE_OUT_OF_RANGE), (h, rc)
            if rc == 0 or not np.all(want[:, n * 1024:] == 0):
                assert np.array_equal(want[:, :n * 1024], got), h


def status_pcm(h, frames, count):
    status, pcm = hh.reference_decode(h, frames, count)
    assert status == "ok"
    return pcm


def test_intensity_15_throws_in_oracle_and_pyref():
    """an encoder frame of 2 ch 'Lowest' with intensity 15 on the secondary: IntensityRatioTable[15] throws
    (CriHcaDecoder.cs:157); 14 decodes"""
    info, frames = hh.encoder_frames(2, 1024 * 4, "Lowest")
    h = pyref.HcaInfo()
    for k in hh.FIELDS:
        setattr(h, k, getattr(info, k))
    for value, throws in ((14, False), (15, True)):
        fr = frames.copy()
        fr[2] = np.frombuffer(pyref.pack_frame(_unpacked(h, fr[2], value)), np.uint8)
        rc, _ = po.hca_decode(info, fr.reshape(-1))
        assert rc == (ORACLE_OUT_OF_RANGE if throws else 0)
        status, at = hh.reference_decode(info, fr, 3)
        assert (status == "IndexError") == throws and (not throws or at == 2)


def _unpacked(h, raw, intensity):
    """frame state of `raw` as pyref unpacks it, with the secondary's intensities replaced"""
    f = pyref.Frame(h)
    pyref._unpack_frame(f, pyref.BitReader(bytes(raw)))
    f.channels[1].intensity = [intensity] * 8
    return f


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_emulator_matches_oracle(emu, family):  # noqa: F811
    """the kernels' lane logic on every header the library takes, at 1, 3 and 16 frames a workgroup; the headers the
    reference throws on up front are refused with VGA_ERR_OUT_OF_RANGE, intensity 15 is flagged (status bit 32)"""
    rng = np.random.default_rng(200 + len(family))
    for k, h in enumerate(FAMILIES[family]):
        e = h.expected()
        if e["frame_size"] < 8 or e["hfr_group_count"] > 8 or e["total_band_count"] > 128:
            continue
        info = h.info()
        rc, d = device_info(info)
        if reference_throws_up_front(e):
            assert rc == _lib.VGA_ERR_OUT_OF_RANGE, h
            frames = hh.frames_for(h, rng, "structured")
            assert hh.oracle_frames(info, frames)[0] == ORACLE_OUT_OF_RANGE, h
            continue
        assert rc == 0, (h, _lib.lib().vga_last_error())
        frames = hh.frames_for(h, rng, "mixed", intensity_max=15 if k % 3 == 0 else 14)
        orc, want = po.hca_decode(info, frames.reshape(-1))
        for group in (1, 3, 16):
            flags, got = emu_run(emu, d, info, frames, group)
            if orc == ORACLE_OUT_OF_RANGE:
                assert flags & 32, h
                break
            assert orc == 0 and flags == 0, (h, orc, flags)
            assert np.array_equal(got, want), (h, group)


def emu_run(emu, d, info, frames, group):  # noqa: F811
    fbytes = info.frame_count * info.frame_size
    pitch = (fbytes + 8 + 15) // 16 * 16
    stream = np.zeros(pitch, np.uint8)
    stream[:fbytes] = np.asarray(frames, np.uint8).reshape(-1)
    rb = emu.emu_record_bytes(d)
    records = np.zeros(info.frame_count * rb, np.uint8)
    u8p = C.POINTER(C.c_uint8)
    flags = emu.emu_hca_scan(d, stream.ctypes.data_as(u8p), pitch, records.ctypes.data_as(u8p))
    assert flags >= 0
    pcm = np.zeros((info.channel_count, max(info.sample_count, 1)), np.int16)
    if flags:
        return flags, None
    rc = emu.emu_hca_frames(d, stream.ctypes.data_as(u8p), pitch, records.ctypes.data_as(u8p),
                            pcm.ctypes.data_as(C.POINTER(C.c_int16)), pcm.shape[1], group)
    assert rc == 0
    return flags, pcm[:, :info.sample_count]


def layout_bytes(d, nch, frame_size, wide):
    """make_decode_layout's record size for one offset width"""
    coded = np.frombuffer(bytes(d), np.int32, 27)[19:19 + nch]
    chunks = sum((int(c) + 15) // 16 for c in coded)
    per_piece = 4 if wide else 8
    header_at = nch * 144 + 16 * ((8 * chunks + per_piece - 1) // per_piece)
    return (header_at + 16 + 63) // 64 * 64


def test_offset_width_follows_the_layout_formula(emu):  # noqa: F811
    """the scan's chunk offsets are 16-bit unless a frame could move the position past 65535 bits; both widths occur
    in the frame-size family and decode exactly there (test_emulator_matches_oracle)"""
    seen = set()
    for h in FAMILIES["frame_size"]:
        e = h.expected()
        rc, d = device_info(h.info())
        assert rc == 0
        coded = np.frombuffer(bytes(d), np.int32, 27)[19:19 + e["channel_count"]]
        max_pos = e["frame_size"] * 8 + 8 * int(coded.sum()) * 12 + 35 + e["channel_count"] * 1500
        wide = max_pos >= 65536
        assert emu.emu_record_bytes(d) == layout_bytes(d, e["channel_count"], e["frame_size"], wide), h
        if layout_bytes(d, e["channel_count"], e["frame_size"], True) != layout_bytes(d, e["channel_count"], e["frame_size"], False):
            seen.add(wide)
    assert seen == {False, True}


def test_device_info_scales_the_ath_curve_and_types_the_channels():
    """the product's header derivation for headers the encoder never writes: the ATH curve of v1.3 files
    (CriHcaFrame.ScaleAthCurve) and the 4 / 5 channel-config variants (GetChannelTypes)"""
    t = pyref.Tables.get()
    for h in FAMILIES["ath"] + FAMILIES["config"]:
        e = h.expected()
        rc, d = device_info(h.info())
        assert rc == 0, h
        words = np.frombuffer(bytes(d), np.int32, 27)
        ath = np.frombuffer(bytes(d), np.uint8, 128, 27 * 4)
        want_ath = pyref.Frame._scale_ath(e["sample_rate"], t) if e["use_ath_curve"] else [0] * 128
        assert list(ath) == list(want_ath), h
        types = hh.channel_types(e)[:e["channel_count"]]
        assert list(words[11:11 + e["channel_count"]]) == types, h
