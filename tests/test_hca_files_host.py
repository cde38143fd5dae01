"""include/vgaudio_hip/hca_files.h without a GPU: the header's functions are exported and in the ctypes table with the header's
argument counts, the cases of tests/hca_files_cases.py are files the oracle writes and reads, vga_hca_files_layout_for (host
code) against a model for packed and explicit frame offsets and against vga_hca_ragged_layout_for, the work items' tiling of
every image and stream in both forms, every refusal with its file and the per-file call's code and message, that the GPU
file's table of cases names every function the header declares, and the HIP-free host layer
(vgaudio_amd/csrc/hca_files_host.hpp) on its own under AddressSanitizer and UBSan."""
import ast
import ctypes as C
import functools
import os
import platform
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hca_files_cases as hc
from oracle import pyoracle as po
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.crihca import RaggedHca
from vgaudio_amd.hca import HcaFileSet, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "hca_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_hca_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "hca_files_host_driver.cpp")

NAMES = ["vga_hca_files_layout_for", "vga_hca_files_create", "vga_hca_files_create_from_infos", "vga_hca_files_destroy",
         "vga_hca_files_totals_of", "vga_hca_files_offsets", "vga_hca_write_device_v", "vga_hca_read_device_v",
         "vga_hca_files_write_items_for", "vga_hca_files_read_items_for", "vga_hca_files_stats", "vga_hca_files_force_general_this_thread"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
HEADER_ITEM, SPAN, GENERAL = 0, 1, 2
i64p = C.POINTER(C.c_int64)


def L():
    return _lib.lib()


def last_error():
    L().vga_last_error.restype = C.c_char_p
    return L().vga_last_error().decode()


def the_sets():
    """name -> (files, frame offsets): packed streams, streams in another order at residues 0, 4, 8, 12 mod 16"""
    files = hc.files_of(hc.CASES)
    return {"packed": (files, None), "explicit": (files, hc.explicit_frame_offsets(files)), "explicit_gaps": (files, hc.explicit_frame_offsets(files, 12))}


@functools.lru_cache(maxsize=None)
def the_infos():
    """the parsed headers of the oracle's images of the cases: (infos, image sizes, odd image offsets)"""
    _, enc = hc.key_tables()
    infos = []
    for i, case in enumerate(hc.CASES):
        rc, image = hc.oracle_image(case, hc.valid_frames(1000 + i, case[0], case[1]), enc)
        assert rc == 0, case
        infos.append(parse(image.tobytes()))
    sizes = [i.frames_offset + i.hca.frame_count * i.hca.frame_size for i in infos]
    return infos, sizes, hc.odd_image_offsets(sizes)


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
    for d, _, files in os.walk(inc):
        for f in sorted(files):
            if f.endswith(".h") and os.path.join(d, f) != HEADER:
                assert not [n for n in NAMES if n in _declared(os.path.join(d, f))], f
    assert "vga_hca_files" not in open(os.path.join(inc, "vgaudio_hip_testing.h")).read()


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    for name in ("vga_hca_write_device_v", "vga_hca_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the cases
def test_the_oracle_accepts_every_case_and_writes_the_librarys_header():
    dec, enc = hc.key_tables()
    for k, (kind, code) in enumerate(hc.KEYS):                         # the library's tables are the oracle's
        rc, odec, oenc = po.hca_key_tables(kind, code)
        assert rc == 0 and np.array_equal(odec, dec[k]) and np.array_equal(oenc, enc[k])
    assert np.array_equal(enc[hc.TYPE0], hc.identity()) and not np.array_equal(enc[hc.KEY_A], enc[hc.KEY_B])
    for i, case in enumerate(hc.CASES):
        f, frames = hc.hca_file(case), hc.valid_frames(1000 + i, case[0], case[1])
        assert hc.bad_count(frames, case[0]) == 0
        rc, image = hc.oracle_image(case, frames, enc)
        assert rc == 0 and len(image) == L().vga_hca_file_size(C.byref(f.hca)), case
        header = np.zeros(f.hca.header_size, np.uint8)
        assert L().vga_hca_file_header(C.byref(f.hca), f.comment, f.volume, f.encryption_type, f.encrypted_ids, header.ctypes.data_as(_lib.u8p)) == 0
        assert np.array_equal(header, image[:f.hca.header_size]), case
        rc, h, volume, enc_type, comment, _ = po.hcafile_read(image)
        assert rc == 0 and (h.frame_size, h.frame_count, h.header_size) == (case[0], case[1], f.hca.header_size), case
        assert enc_type == hc.enc_type_of(case) and volume == case[4] and bool(h.looping) == bool(case[3])
        assert comment == (hc.comment_of(case) or "")
        info = parse(image.tobytes())                                  # and the library's parser takes it for the read side
        assert (info.frames_offset, info.hca.frame_count, info.hca.frame_size) == (f.hca.header_size, case[1], case[0])
        if case[8] >= 0 and case[1]:                                   # a keyed file's frames come back under the inverse table
            back, bad = hc.oracle_read(image, info.frames_offset, case[0], case[1], dec[case[8]])
            assert bad == 0 and np.array_equal(back, frames)


def test_the_cases_reach_what_they_are_for():
    cases = hc.CASES
    assert {c[0] for c in cases} == {8, 9, 341, 682, 683, 4095, 4096, 4097, 32767} and hc.MAX_SPAN_FRAME == 4096
    for fs in (8, 341, 4096):
        assert {c[1] - hc.span_frames(fs) for c in cases if c[0] == fs} >= ({-1, 0, 1} if fs != 4096 else {-1, 0})
    assert {c[1] for c in cases} >= {0, 1} and (32767, 2) in {c[:2] for c in cases}
    assert {c[1] - hc.span_frames(c[0]) for c in cases if c[0] in (4095, 4097)} == {0, 1}
    files = hc.files_of(cases)
    assert {f.hca.header_size % 16 for f in files} >= {0, 1, 2, 3, 4, 7, 8, 15}
    assert {(bool(c[3]), c[4] != 1.0) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    assert {c[7] for c in cases} == {0, 1} and {c[8] for c in cases} == {-1, 0, 1, 2, 3}
    assert {bool(c[5]) for c in cases} == {False, True} and max(c[5] or 0 for c in cases) == 255
    assert sum(m for m in hc.model(files)["stream_bytes"]) < 1 << 20
    assert {o % 16 for o in hc.explicit_frame_offsets(files)} == {0, 4, 8, 12}
    assert {o % 16 for o in hc.odd_image_offsets([1] * len(files))} == {1, 2, 3, 5, 8, 15}
    for f, k in hc.BAD_FRAMES:
        assert 0 <= k < cases[f][1]
    bad_files = {f for f, _ in hc.BAD_FRAMES}
    assert {cases[f][8] >= 0 for f in bad_files} == {True, False} and len(bad_files) >= 3
    assert (10, hc.span_frames(682) - 1) in hc.BAD_FRAMES and (10, hc.span_frames(682)) in hc.BAD_FRAMES
    for f in (1, 5, 10):
        assert {k for g, k in hc.BAD_FRAMES if g == f} >= {0, cases[f][1] - 1}


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("name", sorted(the_sets()))
def test_layout_is_the_model(name):
    files, offs = the_sets()[name]
    fo, io, tot = HcaFileSet.layout(files, offs)
    m = hc.model(files, offs)
    assert list(fo) == m["frame_off"] and list(io) == m["image_off"]
    assert (tot.files, tot.total_frames, tot.frame_bytes, tot.image_bytes) == (len(files), m["total_frames"], m["frame_bytes"], m["image_bytes"])
    assert all(o % 16 == 0 for o in io) and tot.image_bytes == io[-1] + hc.up(m["image_size"][-1], 16) + 256
    # outputs one at a time
    arr = (_lib.HcaFileC * len(files))(*files)
    f = L().vga_hca_files_layout_for
    only, one = _lib.HcaFilesTotalsC(), np.zeros(len(files), np.int64)
    po_ = np.ascontiguousarray(offs, dtype=np.int64).ctypes.data_as(i64p) if offs is not None else None
    assert f(arr, len(files), po_, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), po_, one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, fo)
    assert f(arr, len(files), po_, None, None, None) == ARG


def test_packed_frames_are_one_ragged_objects_output():
    p = _lib.HcaParamsC(2, 0, 0, 2, 48000, 0, 0, 0, 0)
    infos = []
    for n in (0, 1, 900, 5000, 30001, 1024 * 7):
        p.sample_count = n
        h = _lib.HcaInfoC()
        _lib.check(L().vga_hca_encoder_initialize(C.byref(p), C.byref(h)))
        infos.append(h)
    infos[3].frame_count = 0                                           # a header without frames takes no room
    want, _, rt = RaggedHca.layout(infos)
    got, _, tot = HcaFileSet.layout([(h, None, 1.0, 0, 0, -1) for h in infos])
    assert list(got) == list(want) and tot.frame_bytes == rt.frame_bytes and tot.total_frames == rt.total_frames
    assert any(h.frame_count * h.frame_size % 4 for h in infos)


def test_an_empty_set_needs_no_gpu():
    fo, io, tot = HcaFileSet.layout([])
    assert len(fo) == len(io) == 0 and (tot.files, tot.total_frames, tot.frame_bytes, tot.image_bytes) == (0, 0, 8, 256)
    s = HcaFileSet([])
    assert s.files == 0 and s.stats() == (0, 0, 0, 0)
    assert L().vga_hca_write_device_v(s._h, None, None, None) == 0
    assert L().vga_hca_read_device_v(s._h, None, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == []
    s.close()
    r = HcaFileSet.from_infos([])
    assert r.files == 0 and L().vga_hca_read_device_v(r._h, None, None, None, None) == 0
    r.close()
    assert HcaFileSet.write_items([]) == [] and HcaFileSet.read_items([]) == []


# ---------------------------------------------------------------- the work items: tiling and forms
def check_items(files, items, general, read, what):
    m = hc.model(files)
    per = {}
    for it in items:
        per.setdefault(it.file, []).append(it)
    forms = set()
    for f, file in enumerate(files):
        fs, fc, hs = file.hca.frame_size, file.hca.frame_count, 0 if read else file.hca.header_size
        mine = per.pop(f, [])
        head = [i for i in mine if i.form == HEADER_ITEM]
        body = [i for i in mine if i.form != HEADER_ITEM]
        if read:
            assert not head
        else:
            assert len(head) == 1 and (head[0].begin, head[0].end) == (0, hs), (what, f)
        if fs * fc == 0:
            assert not body
            continue
        want = GENERAL if general or not m["span"][f] else SPAN
        assert {i.form for i in body} == {want}, (what, f)
        forms.add(want)
        check_tiling([(i.begin - hs, i.end - hs) for i in body], hc.up(fs * fc, 4) if read else fs * fc, (what, f))
        check_tiling([(i.first_frame, i.first_frame + i.frames) for i in body], fc, (what, f))
        for i in body:                                                 # whole frames, a span's worth at most, or one frame
            assert i.begin == hs + i.first_frame * fs and i.frames == min(hc.span_frames(fs), fc - i.first_frame)
            assert i.frames * fs <= hc.SPAN_BYTES or i.frames == 1
    assert not per
    return forms


def test_write_items_tile_every_image_once():
    for name, (files, offs) in the_sets().items():
        own = check_items(files, HcaFileSet.write_items(files, offs), False, False, name)
        forced = check_items(files, HcaFileSet.write_items(files, offs, general=True), True, False, name)
        assert own == {SPAN, GENERAL} and forced == {GENERAL}
    items = HcaFileSet.write_items(the_sets()["packed"][0])
    forms = [i.form for i in items]                                    # launch order: headers, span items, general items
    assert forms == sorted(forms)


def test_read_items_tile_every_stream_once():
    infos, sizes, odd = the_infos()
    files = hc.files_of(hc.CASES)
    for offs in (None, odd):
        for fo in (None, hc.explicit_frame_offsets(files)):
            own = check_items(files, HcaFileSet.read_items(infos, offs, fo), False, True, "read")
            forced = check_items(files, HcaFileSet.read_items(infos, offs, fo, general=True), True, True, "read")
            assert own == {SPAN, GENERAL} and forced == {GENERAL}
    count = C.c_int64()
    ptrs = (C.c_void_p * len(infos))(*[C.addressof(i) for i in infos])
    room = (_lib.HcaFilesItemC * 2)()
    assert L().vga_hca_files_read_items_for(ptrs, len(infos), None, None, 0, room, 2, C.byref(count)) == ARG and count.value > 2


# ---------------------------------------------------------------- refusals
def changed(case, **fields):
    f = hc.hca_file(case)
    for k, v in fields.items():
        setattr(f.hca if hasattr(f.hca, k) else f, k, v)
    return f


# name -> (the file, code, the per-file call that refuses it alone with the same words | None: the set's own)
def refused_files():
    base = hc.CASES[10]
    return {
        "file_too_large": (changed(base, frame_count=0x7FFFFFF0), RANGE, "size"),
        "negative_frames": (changed(base, frame_count=-1), RANGE, "size"),
        "negative_frame_size": (changed(base, frame_size=-5), RANGE, "size"),
        "header_size_7": (changed(base, header_size=7), RANGE, "header"),
        "header_size_0x8000": (changed(base, header_size=0x8000), RANGE, "header"),
        "chunks_do_not_fit": (changed(base, header_size=64), OP, "header"),
    }


def per_file_answer(f, which):
    if which == "size":
        rc = L().vga_hca_file_size(C.byref(f.hca))
    else:
        out = np.zeros(0x8000, np.uint8)
        rc = L().vga_hca_file_header(C.byref(f.hca), f.comment, f.volume, f.encryption_type, f.encrypted_ids, out.ctypes.data_as(_lib.u8p))
    return rc, last_error()


def refused_set(name, position):
    files = hc.files_of(hc.CASES[:3])
    at = {"first": 0, "middle": 1, "last": 2}[position]
    files[at] = refused_files()[name][0]
    return files, at


def layout_rc(files, offs=None):
    arr, tot = (_lib.HcaFileC * max(len(files), 1))(*files), _lib.HcaFilesTotalsC()
    keep = np.ascontiguousarray(offs, dtype=np.int64) if offs is not None else None
    return L().vga_hca_files_layout_for(arr, len(files), keep.ctypes.data_as(i64p) if offs is not None else None, None, None, C.byref(tot))


def create_rc(files, tables, ntables, offs=None):
    arr, h = (_lib.HcaFileC * max(len(files), 1))(*files), C.c_void_p()
    keep = np.ascontiguousarray(offs, dtype=np.int64) if offs is not None else None
    rc = L().vga_hca_files_create(arr, len(files), keep.ctypes.data_as(i64p) if offs is not None else None,
                                  tables.ctypes.data_as(_lib.u8p) if tables is not None else None, ntables, C.byref(h))
    assert (rc == 0) == bool(h)
    if h:
        L().vga_hca_files_destroy(h)
    return rc


def test_a_refused_file_is_named_with_the_per_file_calls_code_and_message():
    _, enc = hc.key_tables()
    for name, (f, code, which) in sorted(refused_files().items()):
        rc, words = per_file_answer(f, which)
        assert rc == code and words, name
        for position in ("first", "middle", "last"):
            files, at = refused_set(name, position)
            assert layout_rc(files) == code and last_error() == "file %d: %s" % (at, words), (name, position)
            assert create_rc(files, enc, 4) == code and last_error() == "file %d: %s" % (at, words)
            arr, count = (_lib.HcaFileC * 3)(*files), C.c_int64()
            assert L().vga_hca_files_write_items_for(arr, 3, None, 0, None, 0, C.byref(count)) == code


BAD_OFFSETS = {"negative": (1, -4), "odd": (2, 6), "overlap": (1, None), "rounding_overlap": (2, None)}


def bad_offsets(name):
    files = hc.files_of([hc.CASES[3], hc.CASES[4], hc.CASES[12]])      # 45, 16368 and 4781 bytes
    offs = [0, 48, 48 + 16368]
    f, value = BAD_OFFSETS[name]
    if name == "overlap":
        offs[1] = 44                                                   # inside stream 0's last bytes
    elif name == "rounding_overlap":
        offs = [4784, 48 + 4784, 0]                                    # stream 2 owns its bytes up to 4784: fine
        assert layout_rc(files, offs) == 0
        offs[0] = 4780                                                 # inside the rounding of stream 2
    else:
        offs[f] = value
    return files, offs


def test_the_sets_own_refusals():
    dec, enc = hc.key_tables()
    files = hc.files_of(hc.CASES[:4])
    assert create_rc(files, None, 0) == ARG and re.match(r"file 1: key 2 outside -1 \.\. -1", last_error())
    assert create_rc(files, enc, 2) == ARG and last_error().startswith("file 1: key 2 outside")
    assert create_rc(files, None, 4) == ARG and "null" in last_error()
    assert create_rc(files, enc, -1) == ARG
    files[2].key = -2
    assert create_rc(files, enc, 4) == ARG and last_error().startswith("file 2: key -2")
    short = hc.files_of(hc.CASES[:2])
    short[1].hca.frame_size = 1
    assert create_rc(short, enc, 4) == ARG and last_error().startswith("file 1: keyed frames of 1 bytes")
    short[1].hca.frame_size = 0x10000
    short[1].hca.frame_count = 2
    assert create_rc(short, enc, 4) == ARG and last_error().startswith("file 1: keyed frames of 65536 bytes")
    for name in sorted(BAD_OFFSETS):
        files, offs = bad_offsets(name)
        assert layout_rc(files, offs) == ARG and re.match(r"file \d: ", last_error()), name
        assert ("overlaps" in last_error()) == ("overlap" in name)
    assert L().vga_hca_files_layout_for(None, 2, None, None, None, C.byref(_lib.HcaFilesTotalsC())) == ARG
    assert L().vga_hca_files_layout_for(None, -1, None, None, None, C.byref(_lib.HcaFilesTotalsC())) == ARG
    assert L().vga_hca_files_create(None, 0, None, None, 0, None) == ARG
    # totals past 2^62
    big = hc.files_of(hc.CASES[:2])
    assert layout_rc(big, [0, (1 << 62) + 4]) == RANGE and last_error().startswith("file 1: ")


def bad_infos():
    infos, _, _ = the_infos()
    out = {}
    for name, (field, value) in {"frame_size_7": ("frame_size", 7), "frame_size_65536": ("frame_size", 0x10000),
                                 "negative_frames": ("frame_count", -1)}.items():
        i = _lib.HcaFileInfoC.from_buffer_copy(infos[4])
        setattr(i.hca, field, value)
        out[name] = i
    i = _lib.HcaFileInfoC.from_buffer_copy(infos[4])
    i.frames_offset = -1
    out["negative_offset"] = i
    return out


def infos_rc(infos, offs=None, keys=None, tables=None, ntables=0, fo=None):
    ptrs = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) if i is not None else None for i in infos])
    keep = [np.ascontiguousarray(v, dtype=np.int64) if v is not None else None for v in (offs, fo)]
    kk = np.ascontiguousarray(keys, dtype=np.int32) if keys is not None else None
    h = C.c_void_p()
    rc = L().vga_hca_files_create_from_infos(ptrs, len(infos), keep[0].ctypes.data_as(i64p) if offs is not None else None,
                                             kk.ctypes.data_as(C.POINTER(C.c_int)) if keys is not None else None,
                                             tables.ctypes.data_as(_lib.u8p) if tables is not None else None, ntables,
                                             keep[1].ctypes.data_as(i64p) if fo is not None else None, C.byref(h))
    assert (rc == 0) == bool(h)
    if h:
        L().vga_hca_files_destroy(h)
    return rc


def test_a_reading_sets_refusals():
    infos, sizes, odd = the_infos()
    dec, _ = hc.key_tables()
    # what vga_hca_read_device refuses, with its words (that call needs no GPU to refuse)
    for name, bad in sorted(bad_infos().items()):
        assert L().vga_hca_read_device(C.byref(bad), None, 0, 1, None, 0, None, None) == ARG
        words = last_error()
        assert words == "info does not describe an HCA file"
        assert infos_rc([infos[1], bad]) == ARG and last_error() == "file 1: " + words, name
    assert infos_rc([infos[0], None]) == ARG and last_error() == "file 1: null info"
    assert infos_rc(infos[:2], offs=[3, -1]) == ARG and last_error().startswith("file 1: negative image offset")
    assert infos_rc(infos[:2], keys=[-1, 4], tables=dec, ntables=4) == ARG and last_error().startswith("file 1: key 4 outside")
    assert infos_rc(infos[:2], keys=[0, 0], tables=None, ntables=1) == ARG
    assert infos_rc(infos[:2], fo=[0, 2]) == ARG and "multiple of 4" in last_error()
    assert infos_rc(infos[:2], fo=[0, 8]) == ARG and "overlaps" in last_error()
    assert infos_rc(infos[:2], offs=[0, (1 << 62) + 1]) == RANGE
    assert infos_rc(None or [], offs=None) == 0
    assert L().vga_hca_files_create_from_infos(None, 1, None, None, None, 0, None, C.byref(C.c_void_p())) == ARG


# ---------------------------------------------------------------- the header alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as out:
        out.write(struct.pack("<i", len(cases)))
        for kind, items, fo, io, with_keys, ntables, tables_null in cases:
            out.write(struct.pack("<7i", kind, len(items), len(fo or []), len(io or []), with_keys, ntables, tables_null))
            for x in items:
                if kind == 0:
                    out.write(struct.pack("<4i", x.hca.frame_size, x.hca.frame_count, x.hca.header_size, x.key))
                else:
                    info, key = x
                    out.write(struct.pack("<5i", *((0, 0, 0, key, 1) if info is None else
                                                   (info.hca.frame_size, info.hca.frame_count, info.frames_offset, key, 0))))
            out.write(struct.pack("<%dq" % len(fo or []), *(fo or [])))
            out.write(struct.pack("<%dq" % len(io or []), *(io or [])))


def read_result(rd):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc:
        return rc, msg, None
    nf = rd.take("i")[0]
    r = {"frame_off": rd.take("%dq" % nf), "image_off": rd.take("%dq" % nf), "image_size": rd.take("%di" % nf),
         "totals": rd.take("3q"), "files": rd.take("3i"), "items": []}
    for _ in range(2):
        count = rd.take("i")[0]
        r["items"].append([tuple(rd.take("4i2q")) for _ in range(count)])
    return rc, msg, r


def as_tuples(items):
    return [(i.form, i.file, i.first_frame, i.frames, i.begin, i.end) for i in items]


DRIVER_REFUSALS = ("file_too_large", "negative_frames", "negative_frame_size", "header_size_7", "header_size_0x8000")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("hca_files_host")
    exe = str(tmp / "hca_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name, (files, offs) in sorted(the_sets().items()):
        cases.append((0, files, offs, None, 1, 4, 0))
        names.append(("set", name))
    cases.append((0, [], None, None, 1, 0, 0))
    names.append(("empty", ""))
    for name in DRIVER_REFUSALS:
        for position in ("first", "middle", "last"):
            cases.append((0, refused_set(name, position)[0], None, None, 0, 0, 0))
            names.append(("refused", name, position))
    for name in sorted(BAD_OFFSETS):
        files, offs = bad_offsets(name)
        cases.append((0, files, offs, None, 0, 0, 0))
        names.append(("offsets", name))
    files = hc.files_of(hc.CASES[:4])
    cases += [(0, files, None, None, 1, 2, 0), (0, files, None, None, 1, 4, 1), (0, files, None, None, 1, -1, 0)]
    names += [("keys", "outside"), ("keys", "null"), ("keys", "negative")]
    infos, sizes, odd = the_infos()
    keyed = [(i, c[8]) for i, c in zip(infos, hc.CASES)]
    fo = hc.explicit_frame_offsets(hc.files_of(hc.CASES))
    cases += [(1, keyed, None, None, 1, 4, 0), (1, keyed, fo, odd, 1, 4, 0), (1, [], None, None, 1, 0, 0), (1, [keyed[0], (None, -1)], None, None, 1, 4, 0)]
    names += [("infos", "packed"), ("infos", "odd"), ("infos", "empty"), ("infos", "null")]
    for name, bad in sorted(bad_infos().items()):
        cases.append((1, [keyed[1], (bad, -1)], None, None, 1, 4, 0))
        names.append(("infos", "refused", name))
    write_cases(tmp / "cases.bin", cases)
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(cases), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rd = Reader(open(tmp / "results.bin", "rb").read())
    out = {}
    for name, case in zip(names, cases):
        out[name] = (case, read_result(rd))
    assert rd.at == len(rd.d)
    return out


def test_host_layer_is_the_librarys_and_the_models(driver):
    for name, (files, offs) in the_sets().items():
        _, (rc, msg, r) = driver[("set", name)]
        assert rc == 0, (name, msg)
        m = hc.model(files, offs)
        assert r["frame_off"] == m["frame_off"] and r["image_off"] == m["image_off"] and r["image_size"] == m["image_size"]
        assert r["totals"] == [m["total_frames"], m["frame_bytes"], m["image_bytes"]]
        moving = [f for f in files if f.hca.frame_count]
        spans = sum(f.hca.frame_size <= hc.MAX_SPAN_FRAME for f in moving)
        assert r["files"] == [spans, len(moving) - spans, len(moving)]
        for general in (0, 1):
            assert r["items"][general] == as_tuples(HcaFileSet.write_items(files, offs, general)), (name, general)
    _, (rc, msg, r) = driver[("empty", "")]
    assert rc == 0 and r["totals"] == [0, 8, 256] and r["items"] == [[], []]
    infos, sizes, odd = the_infos()
    files = hc.files_of(hc.CASES)
    fo = hc.explicit_frame_offsets(files)
    for which, offs, frames_at in (("packed", None, None), ("odd", odd, fo)):
        _, (rc, msg, r) = driver[("infos", which)]
        assert rc == 0, msg
        want_off, at = [], 0
        for sz in sizes:
            want_off.append(at)
            at = hc.up(at + sz, 16)
        assert r["image_off"] == (offs or want_off) and r["image_size"] == sizes
        assert r["totals"][2] == max(hc.up(o + s, 16) for o, s in zip(r["image_off"], sizes)) + 256
        m = hc.model(files, frames_at)
        assert r["frame_off"] == m["frame_off"] and r["totals"][:2] == [m["total_frames"], m["frame_bytes"]]
        for general in (0, 1):
            assert r["items"][general] == as_tuples(HcaFileSet.read_items(infos, offs, frames_at, general)), (which, general)
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"] == [0, 8, 256]


def test_host_layer_refusals(driver):
    for name in DRIVER_REFUSALS:
        for position in ("first", "middle", "last"):
            (_, files, *_), (rc, msg, _) = driver[("refused", name, position)]
            assert layout_rc(files) == rc == refused_files()[name][1]
            assert msg == last_error() and msg.startswith("file %d: " % refused_set(name, position)[1]), (name, position, msg)
    for name in sorted(BAD_OFFSETS):
        (_, files, offs, *_), (rc, msg, _) = driver[("offsets", name)]
        assert rc == ARG == layout_rc(files, offs) and msg == last_error(), (name, msg)
    _, enc = hc.key_tables()
    for name, (tables, ntables) in {"outside": (enc, 2), "null": (None, 4), "negative": (enc, -1)}.items():
        (_, files, *_), (rc, msg, _) = driver[("keys", name)]
        assert rc == ARG == create_rc(files, tables, ntables) and msg == last_error(), (name, msg)
    for name in bad_infos():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == ARG and msg == "file 1: info does not describe an HCA file", (name, rc, msg)
    _, (rc, msg, _) = driver[("infos", "null")]
    assert rc == ARG and msg == "file 1: null info"
