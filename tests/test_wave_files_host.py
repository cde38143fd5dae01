"""include/vgaudio_hip_files/wave_files.h without a GPU: the header's functions are exported and in the ctypes table with the
header's argument counts and are declared in no other header, vga_wave_files_layout_for (host code) against a model
(tests/wave_files_cases.py) for packed and explicit offsets, the packed rows against vga_adx_ragged_layout_for and
vga_hca_ragged_layout_for, the work items' tiling of every image and row in both forms, that the cases reach every form, every
refusal with its file and the per-file call's code and message, that the GPU file's table of cases names every function the
header declares, the per-file host calls after their move into wave_file_host.hpp against the oracle, and the HIP-free host
layer (vgaudio_amd/csrc/wave_files_host.hpp) on its own under AddressSanitizer and UBSan."""
import ast
import ctypes as C
import os
import platform
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import wave_files_cases as wc
from oracle import pyoracle as po
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.wave import WaveFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "wave_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_wave_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "wave_files_host_driver.cpp")

NAMES = ["vga_wave_files_layout_for", "vga_wave_files_create", "vga_wave_files_create_from_infos", "vga_wave_files_destroy",
         "vga_wave_files_totals_of", "vga_wave_files_offsets", "vga_wave_read_device_v", "vga_wave_write_device_v",
         "vga_wave_files_write_items_for", "vga_wave_files_read_items_for", "vga_wave_files_stats",
         "vga_wave_files_force_general_this_thread"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
HEADER_ITEM, TILE, GENERAL = wc.HEADER_ITEM, wc.TILE, wc.GENERAL
i64p = C.POINTER(C.c_int64)


def L():
    return _lib.lib()


def last_error():
    L().vga_last_error.restype = C.c_char_p
    return L().vga_last_error().decode()


def header_size(f):
    return 12 + 8 + (40 if f.channels > 2 else 16) + (8 + 0x3c if f.params.looping else 0) + 8


def image_sizes(files):
    return [header_size(f) + f.channels * f.params.sample_count * f.bits // 8 for f in files]


def the_sets():
    """name -> (files, pcm offsets, image offsets): packed; rows at any sample boundary and images at odd bytes"""
    files = wc.files_of(wc.cases())
    sizes = image_sizes(files)
    return {"packed": (files, None, None),
            "explicit": (files, wc.explicit_pcm_offsets(wc.counts_of(files)), wc.image_offsets_at(sizes, 5)),
            "rows_only": (files, wc.explicit_pcm_offsets(wc.counts_of(files), start=8, gap=3), None)}


_infos = []


def the_infos():
    """the parsed headers of the read side's images"""
    if not _infos:
        images, rows = wc.read_side()
        _infos.append(([wc.parse(i) for i in images], [len(i) for i in images]))
    return _infos[0]


# ---------------------------------------------------------------- the header against the library and the ctypes table
def test_header_functions_are_exported_with_the_headers_argument_counts():
    declared = _declared(HEADER)
    assert sorted(declared) == sorted(NAMES)
    lib = C.CDLL(_lib.SO_PATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert not [n for n in declared if n not in _lib.SIGNATURES]
    wrong = {n: (len(_lib.SIGNATURES[n][1]), c) for n, c in declared.items() if len(_lib.SIGNATURES[n][1]) != c}
    assert not wrong, f"(ctypes, header) argument counts differ: {wrong}"


def test_the_new_names_are_declared_in_the_new_header_only():
    inc = os.path.join(ROOT, "include")
    seen = 0
    for d, _, files in os.walk(inc):
        for f in sorted(files):
            if f.endswith(".h") and os.path.join(d, f) != HEADER:
                seen += 1
                assert not [n for n in NAMES if n in _declared(os.path.join(d, f))], f
    assert seen >= 10 and os.path.dirname(HEADER) != os.path.join(inc, "vgaudio_hip")


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    for name in ("vga_wave_write_device_v", "vga_wave_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once",
                "test_offsets_past_4_gib"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source and "FarBuffer" in source


# ---------------------------------------------------------------- the per-file host calls: moved, and still the oracle's
def test_the_moved_per_file_size_and_header_are_the_oracles():
    """vga_wave_file_size, vga_wave_pcm8_file_size and the header bytes of empty files (which the _write_ calls assemble on the
    host, no GPU) after the move into wave_file_host.hpp"""
    u8p = C.POINTER(C.c_uint8)
    for nch in (1, 2, 3, 6, 8, 33, 255):
        for loop in (None, (0, 0)):
            f16, f8 = wc.wave_file(nch, 16, 0, loop), wc.wave_file(nch, 8, 0, loop)
            rc, want = po.wave_write([np.zeros(0, np.int16)] * nch, 44100, loop is not None, 0, 0)
            assert rc == 0
            assert L().vga_wave_file_size(C.byref(f16.params), nch) == len(want) == header_size(f16)
            got = np.zeros(len(want), np.uint8)
            ptrs = (C.POINTER(C.c_int16) * nch)()
            assert L().vga_wave_write_pcm16(ptrs, nch, C.byref(f16.params), got.ctypes.data_as(u8p)) == 0
            assert np.array_equal(got, want), (nch, loop)
            want8 = wc.wave8([np.zeros(0, np.int16)] * nch, 44100, loop is not None, 0, 0)
            assert L().vga_wave_pcm8_file_size(C.byref(f8.params), nch) == len(want8)
            got8 = np.zeros(len(want8), np.uint8)
            assert L().vga_wave_write_pcm8((C.c_void_p * nch)(), 0, nch, C.byref(f8.params), got8.ctypes.data_as(u8p)) == 0
            assert got8.tobytes() == want8, (nch, loop)
    f = wc.wave_file(3, 16, 1000, (5, 900))
    assert L().vga_wave_file_size(C.byref(f.params), 3) == header_size(f) + 6000
    assert L().vga_wave_pcm8_file_size(C.byref(f.params), 3) == header_size(f) + 3000
    for nch, n, code in ((0, 10, ARG), (0x8000, 10, ARG), (2, -1, ARG), (0x7FFF, 0x7FFFFFF, RANGE)):
        bad = wc.wave_file(nch, 16, n)
        assert L().vga_wave_file_size(C.byref(bad.params), nch) == code and L().vga_wave_pcm8_file_size(C.byref(bad.params), nch) == code


def test_the_moved_reader_checks_keep_their_codes_and_order():
    images, _ = wc.read_side()
    u8p = C.POINTER(C.c_uint8)
    image = np.ascontiguousarray(images[-2])
    info = wc.parse(image)
    assert info.bits_per_sample == 16
    out = (C.POINTER(C.c_int16) * 2)()
    call = lambda i, n: L().vga_wave_read_pcm16(image.ctypes.data_as(u8p), n, C.byref(i), out)
    assert call(info, len(image) - 2) == ARG and last_error() == "info does not describe this file"
    info.bits_per_sample = 8
    assert call(info, len(image)) == ARG and "only 16-bit" in last_error()
    assert L().vga_wave_read_pcm8(image.ctypes.data_as(u8p), len(image), C.byref(info), (C.c_void_p * 2)(), 7) == ARG
    assert "sample kind" in last_error()                              # the sample kind is looked at first, as before
    info.data_size = 27
    assert L().vga_wave_read_pcm8(image.ctypes.data_as(u8p), len(image), C.byref(info), (C.c_void_p * 2)(), 0) == DATA
    assert last_error() == "The input array length (27) must be divisible by the number of outputs."
    info.bits_per_sample = 16
    assert L().vga_wave_read_pcm8(image.ctypes.data_as(u8p), len(image), C.byref(info), (C.c_void_p * 2)(), 0) == ARG
    assert "only 8-bit" in last_error()


# ---------------------------------------------------------------- the cases
def test_the_cases_reach_what_they_are_for():
    cases = wc.cases()
    assert 24 <= len(cases) <= 40
    assert {c[0] for c in cases} >= set(wc.CHANNELS) and {c[1] for c in cases} == {16, 8}
    assert {c[2] for c in cases} >= {0, 1, 7, 8, 9}
    assert any(c[3] for c in cases) and any(c[3] is None for c in cases)
    for nch in wc.CHANNELS:
        deltas = set()
        for c in cases:
            if c[0] == nch and c[2] > 9:
                span = wc.form_and_span(nch, c[1])[1]
                deltas.add(c[2] - span if c[2] < 2 * span else c[2] - 2 * span)
        assert deltas == {-1, 0, 1, 3}, (nch, deltas)
    first16, first8 = wc.first_general_channels(16), wc.first_general_channels(8)
    assert first8 == 2 * first16 - 1 and (first16 - 1) * 2 * 8 <= wc.SPAN_BYTES < first16 * 2 * 8
    assert (first16, 16) in {c[:2] for c in cases} and (first8, 8) in {c[:2] for c in cases}
    assert any(c[1] == 8 and c[0] * c[2] % 2 for c in cases), "an odd 8-bit data size"
    infos, sizes = the_infos()
    assert infos[-2].data_size_declared == infos[-2].data_size + 7 and infos[-2].sample_count == 98
    assert (infos[-3].data_size, infos[-3].sample_count, infos[-3].channel_count) == (3, 0, 2)
    assert infos[-1].data_offset == 68 + 8 + 0x3c + 34 and infos[-1].looping and infos[-1].channel_count == 3


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("name", sorted(the_sets()))
def test_layout_is_the_model(name):
    files, po_, io_ = the_sets()[name]
    fc, po2, io2, tot = WaveFileSet.layout(files, po_, io_)
    sizes = image_sizes(files)
    assert sizes == [WaveFileSet.file_size(f) for f in files]
    m = wc.model(wc.counts_of(files), sizes, po_, io_)
    assert (tot.files, tot.channels) == (len(files), m["channels"]) and len(po2) == m["channels"]
    assert list(fc) == m["first_channel"] and list(po2) == m["pcm_off"] and list(io2) == m["image_off"]
    assert (tot.pcm_samples, tot.image_bytes) == (m["pcm_samples"], m["image_bytes"])
    if io_ is None:
        assert all(o % 16 == 0 for o in io2) and tot.image_bytes == io2[-1] + wc.up(sizes[-1], 16) + 256
    # outputs one at a time
    arr = (_lib.WaveFileC * len(files))(*files)
    f = L().vga_wave_files_layout_for
    only, one = _lib.WaveFilesTotalsC(), np.zeros(m["channels"], np.int64)
    pp = np.ascontiguousarray(po_, dtype=np.int64).ctypes.data_as(i64p) if po_ is not None else None
    ip = np.ascontiguousarray(io_, dtype=np.int64).ctypes.data_as(i64p) if io_ is not None else None
    assert f(arr, len(files), pp, ip, None, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), pp, ip, None, one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, po2)
    assert f(arr, len(files), pp, ip, None, None, None, None) == ARG


def test_packed_rows_are_the_ragged_objects_rows():
    """offset for offset what vga_adx_ragged_layout_for and vga_hca_ragged_layout_for give for the same counts"""
    from vgaudio_amd.criadx import CriAdxParameters, RaggedAdx
    from vgaudio_amd.crihca import RaggedHca
    files = wc.files_of(wc.cases())
    counts = [n for per in wc.counts_of(files) for n in per]
    _, got, _, tot = WaveFileSet.layout(files)
    want, _, rt = RaggedAdx.layout(CriAdxParameters(FrameSize=18), counts)
    assert list(got) == list(want) and 0 in counts and any(n % 8 for n in counts)
    assert rt.pcm_samples <= tot.pcm_samples + 128                      # the caller allocates the larger of the two totals
    stereo = [wc.wave_file(2, 16, n) for n in (0, 1, 900, 5000, 30001, 1024 * 7, 9)]
    p = _lib.HcaParamsC(2, 0, 0, 2, 48000, 0, 0, 0, 0)
    infos = []
    for f in stereo:
        p.sample_count = f.params.sample_count
        h = _lib.HcaInfoC()
        _lib.check(L().vga_hca_encoder_initialize(C.byref(p), C.byref(h)))
        assert (h.channel_count, h.sample_count) == (2, f.params.sample_count)
        infos.append(h)
    _, rows, _ = RaggedHca.layout(infos)
    _, got, _, _ = WaveFileSet.layout(stereo)
    assert list(got) == list(rows)


def test_an_empty_set_needs_no_gpu():
    fc, po_, io_, tot = WaveFileSet.layout([])
    assert len(fc) == len(po_) == len(io_) == 0 and (tot.files, tot.channels, tot.pcm_samples, tot.image_bytes) == (0, 0, 128, 256)
    s = WaveFileSet([])
    assert s.files == s.channels == 0 and s.stats() == (0, 0, 0, 0)
    assert L().vga_wave_write_device_v(s._h, None, None, None) == 0
    assert L().vga_wave_read_device_v(s._h, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == []
    s.close()
    r = WaveFileSet.from_infos([])
    assert r.files == 0 and L().vga_wave_read_device_v(r._h, None, None, None) == 0
    r.close()
    assert WaveFileSet.write_items([]) == [] and WaveFileSet.read_items([]) == []


# ---------------------------------------------------------------- the work items: tiling and forms
def check_write_items(files, items, general, what):
    per = {}
    for it in items:
        per.setdefault(it.file, []).append(it)
    seen = set()
    for f, file in enumerate(files):
        mine = per.pop(f)
        head = [i for i in mine if i.form == HEADER_ITEM]
        data = [i for i in mine if i.form != HEADER_ITEM]
        hs, frame = header_size(file), file.channels * file.bits // 8
        total = frame * file.params.sample_count
        assert len(head) == 1 and (head[0].begin, head[0].end) == (0, hs), (what, f)
        if total:
            check_tiling([(i.begin - hs, i.end - hs) for i in data], total, (what, f))     # header + items: every byte once
        else:
            assert not data
        tile = frame * 8 <= wc.SPAN_BYTES and not general
        for i in data:
            assert i.form == (TILE if tile else GENERAL) and i.x == f, (what, f)
            if tile:
                assert i.span % 8 == 0 and i.span == wc.SPAN_BYTES // frame // 8 * 8 and i.y % i.span == 0
                assert (i.begin, i.end) == (hs + i.y * frame, hs + min(i.y + i.span, file.params.sample_count) * frame)
            else:
                assert i.span == 0 and i.begin == hs + i.y * wc.CHUNK_BYTES
            seen.add(i.form)
    assert not per
    return seen


@pytest.mark.parametrize("name", sorted(the_sets()))
def test_writer_work_items_tile_every_image(name):
    files, po_, io_ = the_sets()[name]
    own = check_write_items(files, WaveFileSet.write_items(files, po_, io_), False, name)
    forced = check_write_items(files, WaveFileSet.write_items(files, po_, io_, general=True), True, name)
    assert own == {TILE, GENERAL} and forced == {GENERAL}, "the cases reach both forms"
    forms = [i.form for i in WaveFileSet.write_items(files, po_, io_)]
    assert forms == sorted(forms)                                      # the launch order: headers, tile items, general items
    big = wc.wave_file(1, 16, 3 * 2048 * 8 + 5)                        # a general file of several chunks
    items = [i for i in WaveFileSet.write_items([big], general=True) if i.form == GENERAL]
    assert [i.y for i in items] == [0, 1, 2, 3] and items[-1].end - items[-1].begin == 10


@pytest.mark.parametrize("which", ["packed", "odd"])
def test_reader_work_items_tile_every_row(which):
    infos, sizes = the_infos()
    offs = wc.image_offsets_at(sizes, 1) if which == "odd" else None
    seen = set()
    for general in (False, True):
        items = WaveFileSet.read_items(infos, None, offs, general)
        assert not [i for i in items if i.form == HEADER_ITEM]
        rows, row0, n = {}, [], 0
        for i in infos:
            row0.append(n)
            n += i.channel_count
        for it in items:
            info = infos[it.file]
            frame = info.channel_count * info.bits_per_sample // 8
            tile = frame * 8 <= wc.SPAN_BYTES and not general
            assert it.form == (TILE if tile else GENERAL)
            if tile:                                                   # a tile item serves every row of its file
                assert it.x == it.file and it.span == wc.SPAN_BYTES // frame // 8 * 8 and it.y % it.span == 0
                assert (it.begin, it.end) == (it.y * 2, min(it.y + it.span, info.sample_count) * 2)
                for c in range(info.channel_count):
                    rows.setdefault(row0[it.file] + c, []).append((it.begin, it.end))
            else:
                assert row0[it.file] <= it.x < row0[it.file] + info.channel_count and it.begin == it.y * wc.CHUNK_BYTES
                rows.setdefault(it.x, []).append((it.begin, it.end))
            seen.add(it.form)
        for f, info in enumerate(infos):
            for c in range(info.channel_count):
                if info.sample_count:
                    check_tiling(rows.pop(row0[f] + c), info.sample_count * 2, (which, f, c))
        assert not rows
    assert seen == {TILE, GENERAL}


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code and message
GOOD = [(2, 16, 100, None), (1, 8, 33, (1, 30)), (3, 16, 9, None)]
REFUSED = {                                                  # name -> (case, code, the per-file call refuses it too)
    "channels_0": ((0, 16, 100, None), ARG, True),
    "channels_32768": ((0x8000, 16, 1, None), ARG, True),
    "negative_samples": ((2, 8, -1, None), ARG, True),
    "too_large": ((0x7FFF, 16, 0x7FFFFFF, None), RANGE, True),
    "too_large_8": ((0x7FFF, 8, 0x7FFFFFF, None), RANGE, True),
    "bits_24": ((2, 24, 100, None), ARG, False),
    "bits_0": ((2, 0, 100, None), ARG, False),
}


def refused_set(name, position):
    bad = wc.wave_file(*REFUSED[name][0])
    good = wc.files_of(GOOD)
    at = {"first": 0, "middle": 2, "last": len(good)}[position]
    return good[:at] + [bad] + good[at:], at


def per_file_refusal(f):
    """what the per-file writer says to this file alone (its checks come before any device work)"""
    if f.bits == 8:
        rc = L().vga_wave_write_pcm8_device(C.c_void_p(16), 0, 1 << 40, f.channels, C.byref(f.params), C.c_void_p(16), None)
    else:
        rc = L().vga_wave_write_pcm16_device(C.c_void_p(16), 1 << 40, f.channels, C.byref(f.params), C.c_void_p(16), None)
    return rc, last_error()


@pytest.mark.parametrize("position", ["first", "middle", "last"])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file_with_the_per_file_code_and_message(name, position):
    _, code, per_file_too = REFUSED[name]
    files, at = refused_set(name, position)
    arr, tot, out = (_lib.WaveFileC * len(files))(*files), _lib.WaveFilesTotalsC(), C.c_void_p()
    assert L().vga_wave_files_layout_for(arr, len(files), None, None, None, None, None, C.byref(tot)) == code
    message = last_error()
    assert message.startswith("file %d: " % at)
    if per_file_too:
        rc, per_file = per_file_refusal(files[at])
        assert rc == code and per_file and message == "file %d: %s" % (at, per_file)
    else:
        assert "bits" in message
    assert L().vga_wave_files_create(arr, len(files), None, None, C.byref(out)) == code and not out.value
    assert last_error() == message
    count = C.c_int64()
    assert L().vga_wave_files_write_items_for(arr, len(files), None, None, 0, None, 0, C.byref(count)) == code and last_error() == message
    with pytest.raises(_lib._EXC[code], match=r"file %d\b" % at):
        WaveFileSet.layout(files)


BAD_OFFSETS = {"negative": ("pcm", 0, -1), "overlap": ("pcm", 3, 101), "overlap_inside": ("pcm", 2, 150), "image_negative": ("image", 1, -5),
               "image_overlap": ("image", 1, 100)}


def bad_offsets(name):
    files = wc.files_of([(2, 16, 100, None), (2, 8, 100, None)])       # four rows of 100 samples; images of 444 and 244 bytes
    po_, io_ = [0, 100, 201, 301], [0, 444]
    which, at, value = BAD_OFFSETS[name]
    (po_ if which == "pcm" else io_)[at] = value
    return files, po_, io_


@pytest.mark.parametrize("name", sorted(BAD_OFFSETS))
def test_offsets_the_set_refuses(name):
    files, po_, io_ = bad_offsets(name)
    with pytest.raises(_lib.ArgumentError, match=r"file \d\b"):
        WaveFileSet.layout(files, po_, io_)
    tot = WaveFileSet.layout(files, [0, 100, 201, 301], [0, 444])[3]
    assert (tot.pcm_samples, tot.image_bytes) == (401 + 128, wc.up(444 + 244, 16) + 256)
    tot = WaveFileSet.layout(files, [301, 201, 100, 0], [245, 0])[3]    # any order, any boundary
    assert (tot.pcm_samples, tot.image_bytes) == (401 + 128, wc.up(245 + 444, 16) + 256)


# more than 2^62 bytes: a caller's row offset past 2^61 samples, an image offset past 2^62 bytes -> (which, index, value, file)
FAR_OFFSETS = {"pcm_2_61": ("pcm", 1, (1 << 61) + 1, 0), "pcm_2_61_last": ("pcm", 3, (1 << 62) - 1, 1),
               "image_2_62": ("image", 1, (1 << 62) + 1, 1), "image_2_62_first": ("image", 0, (1 << 63) - 1, 0)}


def far_offsets(name):
    files = wc.files_of([(2, 16, 100, None), (2, 8, 100, None)])
    po_, io_ = [0, 100, 201, 301], [0, 444]
    which, at, value, _ = FAR_OFFSETS[name]
    (po_ if which == "pcm" else io_)[at] = value
    return files, po_, io_


def far_infos():
    """the same two shapes as parsed infos (the read side takes the same offsets)"""
    out = []
    for bits in (16, 8):
        i = _lib.WaveInfoC()
        i.channel_count, i.bits_per_sample, i.sample_count, i.data_size, i.data_offset = 2, bits, 100, 200 * bits // 8, 44
        out.append(i)
    return out


def offsets_arg(values):
    return (C.c_int64 * len(values))(*values)


@pytest.mark.parametrize("name", sorted(FAR_OFFSETS))
def test_more_than_2_62_bytes_is_out_of_range_with_its_file(name):
    files, po_, io_ = far_offsets(name)
    file = FAR_OFFSETS[name][3]
    arr, tot, out, count = (_lib.WaveFileC * 2)(*files), _lib.WaveFilesTotalsC(), C.c_void_p(), C.c_int64()
    p, i = offsets_arg(po_), offsets_arg(io_)
    assert L().vga_wave_files_layout_for(arr, 2, p, i, None, None, None, C.byref(tot)) == RANGE
    message = last_error()
    assert message.startswith("file %d: " % file) and "2^62" in message
    assert L().vga_wave_files_create(arr, 2, p, i, C.byref(out)) == RANGE and not out.value and last_error() == message
    assert L().vga_wave_files_write_items_for(arr, 2, p, i, 0, None, 0, C.byref(count)) == RANGE and last_error() == message
    with pytest.raises(_lib.ArgumentOutOfRangeError, match=r"file %d\b" % file):
        WaveFileSet.layout(files, po_, io_)
    infos = far_infos()
    ptrs = (C.c_void_p * 2)(*[C.addressof(x) for x in infos])
    assert L().vga_wave_files_read_items_for(ptrs, 2, p, i, 0, None, 0, C.byref(count)) == RANGE and last_error() == message
    assert L().vga_wave_files_create_from_infos(ptrs, 2, p, i, C.byref(out)) == RANGE and not out.value and last_error() == message
    # the largest offsets a set takes: 2^61 samples, 2^62 bytes
    po_, io_ = [0, 100, 201, 1 << 61], [0, 1 << 62]
    tot = WaveFileSet.layout(files, po_, io_)[3]
    assert (tot.pcm_samples, tot.image_bytes) == ((1 << 61) + 100 + 128, (1 << 62) + wc.up(244, 16) + 256)


# more than 2^31 rows: refused before a row is placed, so files without samples show it at no cost in memory
def too_many_rows(kind):
    if kind == "write":
        one, per = wc.wave_file(0x7FFF, 16, 0), 0x7FFF
    else:
        one, per = _lib.WaveInfoC(), 0xFFFF
        one.channel_count, one.bits_per_sample, one.data_offset = per, 16, 44
    n = 0x7FFFFFFF // per + 1                                          # n - 1 files fit, file n - 1 is one too many
    return one, n


@pytest.mark.parametrize("kind", ["write", "read"])
def test_more_than_2_31_rows_is_refused_with_its_file(kind):
    one, n = too_many_rows(kind)
    tot, out, count = _lib.WaveFilesTotalsC(), C.c_void_p(), C.c_int64()
    message = "file %d: more than 2^31 rows" % (n - 1)
    if kind == "write":
        arr = (_lib.WaveFileC * n)(*([one] * n))
        assert L().vga_wave_files_layout_for(arr, n, None, None, None, None, None, C.byref(tot)) == ARG and last_error() == message
        assert L().vga_wave_files_create(arr, n, None, None, C.byref(out)) == ARG and not out.value and last_error() == message
        assert L().vga_wave_files_write_items_for(arr, n, None, None, 0, None, 0, C.byref(count)) == ARG and last_error() == message
    else:
        ptrs = (C.c_void_p * n)(*([C.addressof(one)] * n))
        assert L().vga_wave_files_read_items_for(ptrs, n, None, None, 0, None, 0, C.byref(count)) == ARG and last_error() == message
        assert L().vga_wave_files_create_from_infos(ptrs, n, None, None, C.byref(out)) == ARG and not out.value and last_error() == message
        one.channel_count = 0x10000                                    # no WAVE header says so
        assert L().vga_wave_files_read_items_for(ptrs, 1, None, None, 0, None, 0, C.byref(count)) == ARG
        assert last_error() == "file 0: info does not describe this file"


def bad_infos():
    """name -> (info, code, the per-file reader that refuses it, or None for the set's own refusals)"""
    infos, _ = the_infos()
    base16 = next(i for i in infos if i.bits_per_sample == 16 and i.channel_count == 2 and i.sample_count > 9)
    base8 = next(i for i in infos if i.bits_per_sample == 8 and i.channel_count == 2 and i.sample_count > 9)
    out = {}
    for name, (base, field, value, code, reader) in {
            "bits_24": (base16, "bits_per_sample", 24, ARG, "pcm16"), "samples_past_the_data": (base16, "sample_count", base16.sample_count + 1, ARG, "pcm16"),
            "offset_negative": (base16, "data_offset", -1, ARG, "pcm16"), "pcm8_not_divisible": (base8, "data_size", base8.data_size - 1, DATA, "pcm8"),
            "pcm8_samples_past_the_data": (base8, "sample_count", base8.sample_count + 1, ARG, "pcm8"),
            "pcm8_no_channels": (base8, "channel_count", 0, ARG, "pcm8"),
            "negative_channels": (base16, "channel_count", -2, ARG, None), "negative_samples": (base16, "sample_count", -1, ARG, None),
            "offset_past_2_gib": (base16, "data_offset", 1 << 31, RANGE, None), "offset_huge": (base8, "data_offset", (1 << 63) - 1, RANGE, None)}.items():
        i = _lib.WaveInfoC.from_buffer_copy(base)
        setattr(i, field, value)
        out[name] = (i, code, reader)
    return out


def test_infos_the_per_file_readers_refuse_are_refused_with_their_file():
    infos, _ = the_infos()
    good = infos[-2]                                                   # the stereo file of 98 samples
    junk = np.zeros(16, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8))
    for name, (bad, code, reader) in bad_infos().items():
        with pytest.raises(_lib._EXC[code], match=r"file 2: ") as e:
            WaveFileSet.read_items([good, good, bad, good])
        if reader:                                                      # the per-file call, given a file that ends with the data present
            size = bad.data_offset + bad.data_size
            if reader == "pcm16":
                rc = L().vga_wave_read_pcm16(junk, size, C.byref(bad), (C.POINTER(C.c_int16) * 4)())
            else:
                rc = L().vga_wave_read_pcm8(junk, size, C.byref(bad), (C.c_void_p * 4)(), 0)
            assert rc == code and str(e.value) == "file 2: " + last_error(), name
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        WaveFileSet.read_items([good, good], image_offsets=[0, -1])
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b.*overlaps"):
        WaveFileSet.read_items([good, good], pcm_offsets=[0, 98, 97, 400])
    count = C.c_int64()
    ptrs = (C.c_void_p * 2)(C.addressof(good), None)
    assert L().vga_wave_files_read_items_for(ptrs, 2, None, None, 0, None, 0, C.byref(count)) == ARG and last_error() == "file 1: null info"
    out = C.c_void_p()
    assert L().vga_wave_files_create_from_infos(None, 2, None, None, C.byref(out)) == ARG and not out.value


def test_null_arguments():
    tot = _lib.WaveFilesTotalsC()
    assert L().vga_wave_files_layout_for(None, 2, None, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_wave_files_layout_for(None, -1, None, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_wave_files_create(None, 0, None, None, None) == ARG
    assert L().vga_wave_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_wave_files_offsets(None, None, None, None) == ARG
    assert L().vga_wave_files_stats(None, None) == ARG
    L().vga_wave_files_destroy(None)
    assert L().vga_wave_write_device_v(None, None, None, None) == ARG
    assert L().vga_wave_read_device_v(None, None, None, None) == ARG
    files = (_lib.WaveFileC * 1)(wc.wave_file(2, 16, 100))
    items, count = (_lib.WaveFilesItemC * 1)(), C.c_int64()
    assert L().vga_wave_files_write_items_for(files, 1, None, None, 0, items, 1, C.byref(count)) == ARG and count.value == 2
    old = L().vga_wave_files_force_general_this_thread(1)
    assert old == 0 and L().vga_wave_files_force_general_this_thread(0) == 1


# ---------------------------------------------------------------- the headers alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, files, po_, io_ in cases:
            po_, io_ = list(po_) if po_ is not None else [], list(io_) if io_ is not None else []
            f.write(struct.pack("<4i", kind, len(files), len(po_), len(io_)))
            for x in files:
                if kind == 0:
                    f.write(struct.pack("<7i", x.channels, x.bits, *[getattr(x.params, k) for k, _ in x.params._fields_]))
                elif x is None:
                    f.write(struct.pack("<6q", 0, 0, 0, 0, 0, 1))
                else:
                    f.write(struct.pack("<6q", x.channel_count, x.bits_per_sample, x.sample_count, x.data_size, x.data_offset, 0))
            f.write(struct.pack("<%dq" % len(po_), *po_))
            f.write(struct.pack("<%dq" % len(io_), *io_))


def read_result(rd, kind):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc:
        return rc, msg, None
    nfiles, nrows = rd.take("2i")
    r = {"first_channel": rd.take("%di" % nfiles), "image_off": rd.take("%dq" % nfiles), "image_size": rd.take("%di" % nfiles),
         "row_off": rd.take("%dq" % nrows), "row_samples": rd.take("%di" % nrows), "totals": rd.take("2q"), "headers": [], "items": []}
    for _ in range(nfiles if kind == 0 else 0):
        size = rd.take("i")[0]
        r["headers"].append(bytes(rd.d[rd.at:rd.at + size]))
        rd.at += size
    for _ in range(2):
        count = rd.take("i")[0]
        r["items"].append([tuple(rd.take("3iIi2q")) for _ in range(count)])
    return rc, msg, r


def as_tuples(items):
    return [(i.form, i.file, i.x, i.y, i.span, i.begin, i.end) for i in items]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("wave_files_host")
    exe = str(tmp / "wave_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name, (files, po_, io_) in sorted(the_sets().items()):
        cases.append((0, files, po_, io_))
        names.append(("set", name))
    cases.append((0, [], None, None))
    names.append(("empty", ""))
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            cases.append((0, refused_set(name, position)[0], None, None))
            names.append(("refused", name, position))
    for name in sorted(BAD_OFFSETS):
        cases.append((0,) + bad_offsets(name))
        names.append(("offsets", name))
    for name in sorted(FAR_OFFSETS):
        files, po_, io_ = far_offsets(name)
        cases += [(0, files, po_, io_), (1, far_infos(), po_, io_)]
        names += [("far", name, "write"), ("far", name, "read")]
    for kind in ("write", "read"):
        one, n = too_many_rows(kind)
        cases.append((0 if kind == "write" else 1, [one] * n, None, None))
        names.append(("rows", kind))
    infos, sizes = the_infos()
    odd = wc.image_offsets_at(sizes, 1)
    rows = wc.explicit_pcm_offsets([[i.sample_count] * i.channel_count for i in infos])
    cases += [(1, infos, None, None), (1, infos, rows, odd), (1, [], None, None), (1, [infos[0], None], None, None)]
    names += [("infos", "packed"), ("infos", "odd"), ("infos", "empty"), ("infos", "null")]
    for name, (bad, _, _) in sorted(bad_infos().items()):
        cases.append((1, [infos[1], bad], None, None))
        names.append(("infos", "refused", name))
    write_cases(tmp / "cases.bin", cases)
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(cases), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rd = Reader(open(tmp / "results.bin", "rb").read())
    out = {}
    for name, case in zip(names, cases):
        out[name] = (case, read_result(rd, case[0]))
    assert rd.at == len(rd.d)
    return out


def test_host_layer_is_the_librarys_and_the_models(driver):
    _, _, _, images = wc.reference()
    for name, (files, po_, io_) in the_sets().items():
        _, (rc, msg, r) = driver[("set", name)]
        assert rc == 0, (name, msg)
        sizes = image_sizes(files)
        m = wc.model(wc.counts_of(files), sizes, po_, io_)
        assert r["first_channel"] == m["first_channel"] and r["row_off"] == m["pcm_off"] and r["image_off"] == m["image_off"]
        assert r["image_size"] == sizes and r["totals"] == [m["pcm_samples"], m["image_bytes"]]
        assert r["row_samples"] == [n for per in wc.counts_of(files) for n in per]
        for f, header in enumerate(r["headers"]):                      # the headers a set writes are the reference images' own
            assert header == images[f][:len(header)].tobytes() and len(header) == header_size(files[f]), (name, f)
        for general in (0, 1):
            assert r["items"][general] == as_tuples(WaveFileSet.write_items(files, po_, io_, general)), (name, general)
    _, (rc, msg, r) = driver[("empty", "")]
    assert rc == 0 and r["totals"] == [128, 256] and r["items"] == [[], []]
    infos, sizes = the_infos()
    for which in ("packed", "odd"):
        (_, _, po_, io_), (rc, msg, r) = driver[("infos", which)]
        assert rc == 0, msg
        m = wc.model([[i.sample_count] * i.channel_count for i in infos], sizes, po_, io_)
        assert r["image_off"] == m["image_off"] and r["image_size"] == sizes and r["row_off"] == m["pcm_off"]
        assert r["totals"] == [m["pcm_samples"], m["image_bytes"]]
        for general in (0, 1):
            assert r["items"][general] == as_tuples(WaveFileSet.read_items(infos, po_, io_, general)), (which, general)
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"] == [128, 256]


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            (_, files, _, _), (rc, msg, _) = driver[("refused", name, position)]
            at = refused_set(name, position)[1]
            arr, tot = (_lib.WaveFileC * len(files))(*files), _lib.WaveFilesTotalsC()
            assert L().vga_wave_files_layout_for(arr, len(files), None, None, None, None, None, C.byref(tot)) == rc == REFUSED[name][1]
            assert msg == last_error() and msg.startswith("file %d: " % at), (name, position, msg)
    for name in sorted(BAD_OFFSETS):
        _, (rc, msg, _) = driver[("offsets", name)]
        assert rc == ARG and re.match(r"file \d: ", msg), (name, msg)
    for name in sorted(FAR_OFFSETS):
        for side in ("write", "read"):
            _, (rc, msg, _) = driver[("far", name, side)]
            assert rc == RANGE and msg.startswith("file %d: " % FAR_OFFSETS[name][3]) and "2^62" in msg, (name, side, msg)
    for kind in ("write", "read"):
        _, (rc, msg, _) = driver[("rows", kind)]
        assert rc == ARG and msg == "file %d: more than 2^31 rows" % (too_many_rows(kind)[1] - 1), (kind, msg)
    for name, (_, code, _) in bad_infos().items():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == code and msg.startswith("file 1: "), (name, rc, msg)
    _, (rc, msg, _) = driver[("infos", "null")]
    assert rc == ARG and msg == "file 1: null info"
