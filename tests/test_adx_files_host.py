"""include/vgaudio_hip/adx_files.h without a GPU: the header's functions are exported and in the ctypes table with the header's
argument counts, vga_adx_files_layout_for (host code) against a model built from the per-file vga_adx_file_layout_for
(tests/adx_files_cases.py) for packed and explicit row offsets, the work items' tiling of every image and row, the form every
file takes, every refusal with its file and the per-file call's code and message, that the GPU file's table of cases names
every function the header declares, the per-file layout against the oracle's, and the HIP-free host layer
(vgaudio_amd/csrc/adx_files_host.hpp) on its own under AddressSanitizer and UBSan."""
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

import adx_files_cases as ac
from oracle import pyoracle as po
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.adx import AdxFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "adx_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_adx_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "adx_files_host_driver.cpp")

NAMES = ["vga_adx_files_layout_for", "vga_adx_files_create", "vga_adx_files_create_from_infos", "vga_adx_files_destroy",
         "vga_adx_files_totals_of", "vga_adx_files_offsets", "vga_adx_write_device_v", "vga_adx_read_device_v",
         "vga_adx_files_write_items_for", "vga_adx_files_read_items_for", "vga_adx_files_stats", "vga_adx_files_force_general_this_thread"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
HEADER_ITEM, SPAN, GENERAL, FOOTER = 0, 1, 2, 3
GOOD = ac.CASES[:3]


def L():
    return _lib.lib()


def last_error():
    L().vga_last_error.restype = C.c_char_p
    return L().vga_last_error().decode()


def the_sets():
    """name -> (files, audio offsets): packed rows, rows at multiples of 16 in another order, rows at multiples of 4 only"""
    files = ac.files_of(ac.CASES)
    return {"packed": (files, None), "explicit16": (files, ac.explicit_offsets(files, 0)), "explicit4": (files, ac.explicit_offsets(files, 4))}


def the_infos():
    """the parsed headers of the cases' images, and two frame sizes no case writes"""
    files = ac.files_of(ac.CASES)
    infos = [ac.info_of(f, ac.file_layout(f)[1]) for f in files]
    for fs, nch, frames, offset in ((16, 2, 300, 32), (64, 1, 77, 41), (18, 1, 5000, 36)):
        i = _lib.AdxFileInfoC()
        i.frame_size, i.channel_count, i.frame_count, i.audio_bytes, i.audio_offset, i.version = fs, nch, frames, frames * fs, offset, 3
        infos.append(i)
    sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
    return infos, sizes, ac.odd_image_offsets(sizes)


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


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    for name in ("vga_adx_write_device_v", "vga_adx_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the per-file layout: moved, and still the oracle's
def test_the_moved_per_file_layout_is_the_oracles():
    for case in ac.CASES:
        f = ac.adx_file(case)
        rc, lay = ac.file_layout(f)
        p = f.params
        orc, want = po.adxfile_layout(po.adxfile_params(p.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end, p.alignment_samples,
                                                        p.frame_size, p.version, p.type, p.highpass_frequency, p.encryption_type, p.trim_file), f.channels)
        assert rc == orc == 0, case
        assert all(getattr(lay, k) == getattr(want, k) for k, _ in lay._fields_), case


def test_the_cases_reach_what_they_are_for():
    lay = [ac.file_layout(f)[1] for f in ac.files_of(ac.CASES)]
    files = ac.files_of(ac.CASES)
    assert [ac.alignment_of(c) for c in ac.CASES[5:8]] == [59, 27, 0]
    assert (lay[3].file_size, lay[3].audio_offset) == (58, 40)
    assert (lay[5].frame_count, ac.row_bytes(files[5]) // 18) == (10, 9)                    # more frames asked than the rows hold
    assert (lay[8].frame_count, ac.row_bytes(files[8]) // 18) == (6, 8)                     # fewer: truncation
    assert lay[9].frame_count == 8
    assert lay[10].alignment_bytes > 0 and files[10].params.version == 3
    assert ac.model(files)["header_end"][12] == 1068 and lay[12].audio_offset == 40         # the 255-channel header overrun
    assert {f.params.frame_size for f in files} >= {18, 19, 36, 255}
    assert {l.audio_offset % 16 for l in lay} >= {8, 4, 0}                                  # 40, 36, behind a loop's 0x800 boundary


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("name", sorted(the_sets()))
def test_layout_is_the_per_file_calls_packed(name):
    files, offs = the_sets()[name]
    fc, ao, io, tot = AdxFileSet.layout(files, offs)
    m = ac.model(files, offs)
    assert (tot.files, tot.channels) == (len(files), m["channels"]) and len(ao) == m["channels"]
    assert list(fc) == m["first_channel"] and list(ao) == m["audio_off"] and list(io) == m["image_off"]
    assert (tot.audio_bytes, tot.image_bytes) == (m["audio_bytes"], m["image_bytes"])
    assert all(o % 16 == 0 for o in io) and tot.image_bytes == io[-1] + ac.up(m["image_size"][-1], 16) + 256
    if offs is None:                                                   # one ragged ADX object's output is the set's input as it lies
        from vgaudio_amd.criadx import CriAdxParameters, RaggedAdx
        same = [f for f in files if f.params.frame_size == 18 and f.params.alignment_samples == 0]
        _, want, rt = RaggedAdx.layout(CriAdxParameters(FrameSize=18), [f.params.sample_count for f in same for _ in range(f.channels)])
        _, got, _, st = AdxFileSet.layout(same)
        assert len(same) > 5 and list(got) == list(want) and st.audio_bytes == rt.adx_bytes
    # outputs one at a time
    arr, i64p = (_lib.AdxFileC * len(files))(*files), C.POINTER(C.c_int64)
    f = L().vga_adx_files_layout_for
    only, one = _lib.AdxFilesTotalsC(), np.zeros(m["channels"], np.int64)
    po_ = np.ascontiguousarray(offs, dtype=np.int64).ctypes.data_as(i64p) if offs is not None else None
    assert f(arr, len(files), po_, None, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), po_, None, one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, ao)
    assert f(arr, len(files), po_, None, None, None, None) == ARG


def test_an_empty_set_needs_no_gpu():
    fc, ao, io, tot = AdxFileSet.layout([])
    assert len(fc) == len(ao) == len(io) == 0 and (tot.files, tot.channels, tot.audio_bytes, tot.image_bytes) == (0, 0, 256, 256)
    s = AdxFileSet([])
    assert s.files == s.channels == 0 and s.stats() == (0, 0, 0, 0)
    assert L().vga_adx_write_device_v(s._h, None, None, None, None) == 0
    assert L().vga_adx_read_device_v(s._h, None, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == []
    s.close()
    r = AdxFileSet.from_infos([])
    assert r.files == 0 and L().vga_adx_read_device_v(r._h, None, None, None, None) == 0
    r.close()
    assert AdxFileSet.write_items([]) == [] and AdxFileSet.read_items([]) == []


# ---------------------------------------------------------------- the work items: tiling and forms
def check_write_items(files, offs, items, general, what):
    m = ac.model(files, offs)
    per = {}
    for it in items:
        per.setdefault(it.file, []).append(it)
    seen = set()
    for f, file in enumerate(files):
        lay, nch, fs = m["layouts"][f], file.channels, file.params.frame_size
        mine = per.pop(f)
        head = [i for i in mine if i.form == HEADER_ITEM]
        foot = [i for i in mine if i.form == FOOTER]
        audio = [i for i in mine if i.form in (SPAN, GENERAL)]
        assert len(head) == len(foot) == 1, (what, f)
        copy = m["copy_frames"][f]
        footer_pos = lay.audio_offset + copy * fs * nch
        assert (head[0].begin, head[0].end) == (0, m["header_end"][f]) and m["header_end"][f] <= lay.file_size
        assert (foot[0].begin, foot[0].end, foot[0].keep_end) == (footer_pos, lay.file_size, m["header_end"][f])
        assert footer_pos + 4 <= lay.file_size
        # the audio items tile [audio offset, footer) exactly; the header overlaps them only where its fields ran past the
        # audio offset, and the footer item only keeps such bytes behind its own four
        ranges = [(i.begin, i.end) for i in audio]
        if copy:
            check_tiling([(a - lay.audio_offset, b - lay.audio_offset) for a, b in ranges], copy * fs * nch, (what, f))
        else:
            assert not audio
        # header + audio + footer cover the image: what the header leaves behind the audio offset is the audio's or the footer's
        covered = np.zeros(lay.file_size, np.int32)
        covered[:lay.audio_offset] += 1
        for a, b in ranges:
            covered[a:b] += 1
        covered[footer_pos:footer_pos + 4] += 1
        covered[max(footer_pos + 4, m["header_end"][f]):] += 1
        covered[max(footer_pos + 4, lay.audio_offset):max(footer_pos + 4, m["header_end"][f])] += 1      # header fields kept
        assert (covered == 1).all(), (what, f)
        want_span = m["span"][f] and not general
        for i in audio:
            assert i.form == (SPAN if want_span else GENERAL), (what, f)
            if i.form == SPAN:
                span = ac.span_frames(nch)
                assert span % 8 == 0 and span * 18 * nch <= ac.SPAN_BYTES and i.x == f and i.y % span == 0
                assert i.begin == lay.audio_offset + i.y * 18 * nch and i.end == lay.audio_offset + min(i.y + span, copy) * 18 * nch
                assert all(o % 16 == 0 for o in m["audio_off"][m["first_channel"][f]:m["first_channel"][f] + nch])
            else:
                g = m["granule"][f]
                assert i.granule == g and i.x == f and (i.begin - lay.audio_offset) == i.y * ac.CHUNK_GRANULES * g
                assert (m["image_off"][f] + lay.audio_offset) % g == 0 and (nch == 1 or fs % g == 0)
                assert all(o % g == 0 for o in m["audio_off"][m["first_channel"][f]:m["first_channel"][f] + nch])
            seen.add((i.form, i.granule))
    assert not per
    return seen


@pytest.mark.parametrize("name", sorted(the_sets()))
def test_writer_work_items_tile_every_image(name):
    files, offs = the_sets()[name]
    own = check_write_items(files, offs, AdxFileSet.write_items(files, offs), False, name)
    forced = check_write_items(files, offs, AdxFileSet.write_items(files, offs, general=True), True, name)
    assert not any(form == SPAN for form, _ in forced)
    if name == "explicit4":
        assert not any(form == SPAN for form, _ in own), "rows off the 16-byte grid take the general form"
    else:
        assert any(form == SPAN for form, _ in own) and any(form == GENERAL for form, _ in own), "the cases reach both forms"
    # the launch order: headers, span items, general items, footers
    forms = [i.form for i in AdxFileSet.write_items(files, offs)]
    assert forms == sorted(forms)


def test_the_form_of_every_file_follows_the_rule():
    files, _ = the_sets()["packed"]
    form = {}
    for i in AdxFileSet.write_items(files):
        if i.form in (SPAN, GENERAL):
            form.setdefault(i.file, set()).add(i.form)
    for f, (case, file) in enumerate(zip(ac.CASES, files)):
        if f in form:
            assert form[f] == {SPAN if case[5] == 18 and case[0] <= 113 else GENERAL}, case
    by_case = {c: form.get(f) for f, c in enumerate(ac.CASES)}
    assert by_case[ac.CASES[-1]] == {GENERAL} and by_case[ac.CASES[-2]] == {SPAN}           # 114 and 113 channels
    spans = [i for i in AdxFileSet.write_items(files) if i.form == SPAN and i.file == len(files) - 3]
    assert [(i.y, (i.end - i.begin) // 36) for i in spans] == [(0, 448), (448, 1)]            # one span plus one frame
    assert ac.span_frames(113) == 8 and ac.span_frames(1) == 904


@pytest.mark.parametrize("which", ["packed", "odd"])
def test_reader_work_items_tile_every_row(which):
    infos, sizes, odd = the_infos()
    offs = odd if which == "odd" else None
    want_off, at = [], 0
    for sz in sizes:
        want_off.append(at)
        at = ac.up(at + sz, 16)
    image_off = offs or want_off
    seen = set()
    for general in (False, True):
        items = AdxFileSet.read_items(infos, offs, general)
        assert not [i for i in items if i.form in (HEADER_ITEM, FOOTER)]
        rows, row0 = {}, []
        n = 0
        for i in infos:
            row0.append(n)
            n += i.channel_count
        for it in items:
            f = it.file
            info = infos[f]
            want_span = info.frame_size == 18 and info.channel_count <= 113 and not general
            assert it.form == (SPAN if want_span else GENERAL)
            if it.form == SPAN:                                        # a span item serves every row of its file
                span = ac.span_frames(info.channel_count)
                assert it.x == f and it.y % span == 0 and (it.begin, it.end) == (it.y * 18, min(it.y + span, info.frame_count) * 18)
                for c in range(info.channel_count):
                    rows.setdefault(row0[f] + c, []).append((it.begin, it.end))
            else:
                g = ac.granule_of(image_off[f] + info.audio_offset, *([info.frame_size] if info.channel_count > 1 else []))
                assert it.granule == g and row0[f] <= it.x < row0[f] + info.channel_count and it.begin == it.y * ac.CHUNK_GRANULES * g
                rows.setdefault(it.x, []).append((it.begin, it.end))
            seen.add((it.form, it.granule))
        for f, info in enumerate(infos):
            for c in range(info.channel_count):
                if info.audio_bytes:
                    check_tiling(rows.pop(row0[f] + c), info.audio_bytes, (which, f, c))
        assert not rows
    if which == "odd":
        assert {g for form, g in seen if form == GENERAL} >= {1, 2}
    else:
        assert {g for form, g in seen if form == GENERAL} >= {2, 4, 16} and (SPAN, 0) in seen


def test_the_odd_image_offsets_reach_every_residue():
    """(create needs a device: the read side's layout is checked through the driver below and on the GPU)"""
    _, _, odd = the_infos()
    assert any(o % 2 for o in odd) and len({o % 16 for o in odd}) > 8


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code and message
def refused_set(name, position):
    bad = ac.adx_file(ac.REFUSED[name][0])
    good = ac.files_of(GOOD)
    at = {"first": 0, "middle": 2, "last": len(good)}[position]
    return good[:at] + [bad] + good[at:], at


def per_file_refusal(f):
    """what vga_adx_write_device says to this file alone (its checks come before any device work)"""
    rows = ac.row_bytes(f) if f.params.frame_size > 2 and f.params.sample_count >= 0 else 0
    rc = L().vga_adx_write_device(C.c_void_p(16), max(rows, 1), min(rows, 0x7FFFFFFF), C.c_void_p(16), f.channels, C.byref(f.params), C.c_void_p(16), None)
    return rc, last_error()


@pytest.mark.parametrize("position", ["first", "middle", "last"])
@pytest.mark.parametrize("name", sorted(ac.REFUSED))
def test_refusals_name_their_file_with_the_per_file_code_and_message(name, position):
    _, code, per_file_too = ac.REFUSED[name]
    files, at = refused_set(name, position)
    arr, tot, out = (_lib.AdxFileC * len(files))(*files), _lib.AdxFilesTotalsC(), C.c_void_p()
    assert L().vga_adx_files_layout_for(arr, len(files), None, None, None, None, C.byref(tot)) == code
    message = last_error()
    assert message.startswith("file %d: " % at)
    if per_file_too:
        rc, per_file = per_file_refusal(files[at])
        assert rc == code and per_file and message == "file %d: %s" % (at, per_file)
    else:
        assert "footer" in message and ac.file_layout(files[at])[0] == 0
    assert L().vga_adx_files_create(arr, len(files), None, C.byref(out)) == code and not out.value
    assert last_error() == message
    count = C.c_int64()
    assert L().vga_adx_files_write_items_for(arr, len(files), None, 0, None, 0, C.byref(count)) == code and last_error() == message
    with pytest.raises(_lib._EXC[code], match=r"file %d\b" % at):
        AdxFileSet.layout(files)


def test_the_oracle_refuses_the_refused_files_too():
    for name in ("header_does_not_fit", "frame_size_3"):
        f = ac.adx_file(ac.REFUSED[name][0])
        p = f.params
        rows = ac.row_bytes(f)
        rc, _ = po.adxfile_write([np.zeros(max(rows, 1), np.uint8)[:rows]] * f.channels, np.zeros(f.channels, np.int16),
                                 po.adxfile_params(p.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end, p.alignment_samples,
                                                   p.frame_size, p.version, p.type, p.highpass_frequency, p.encryption_type, p.trim_file))
        assert rc != 0, name


BAD_OFFSETS = {"negative": (0, -16), "off_4": (1, 18), "overlap": (3, 4), "overlap_inside": (2, 40)}


def bad_offsets(name):
    files = ac.files_of([(2, 64, 0, 0, 0) + ac.D, (2, 64, 0, 0, 0) + ac.D])            # four rows of 36 bytes
    offs = [0, 48, 96, 144]
    row, value = BAD_OFFSETS[name]
    offs[row] = value
    return files, offs


@pytest.mark.parametrize("name", sorted(BAD_OFFSETS))
def test_row_offsets_the_set_refuses(name):
    files, offs = bad_offsets(name)
    with pytest.raises(_lib.ArgumentError, match=r"file \d\b"):
        AdxFileSet.layout(files, offs)
    assert AdxFileSet.layout(files, [0, 48, 96, 144])[3].audio_bytes == 144 + 36 + 256
    assert AdxFileSet.layout(files, [144, 96, 48, 4])[3].audio_bytes == 144 + 36 + 256      # any order, multiples of 4


def bad_infos():
    out = {}
    for name, (field, value) in {"channels0": ("channel_count", 0), "channels256": ("channel_count", 256), "frame0": ("frame_size", 0),
                                 "frames": ("frame_count", -1), "bytes": ("audio_bytes", 17), "offset": ("audio_offset", -1)}.items():
        i = ac.info_of(ac.adx_file(ac.CASES[1]), ac.file_layout(ac.adx_file(ac.CASES[1]))[1])
        setattr(i, field, value)
        out[name] = i
    return out


def test_infos_the_per_file_reader_refuses_are_refused_with_their_file():
    good = ac.info_of(ac.adx_file(ac.CASES[1]), ac.file_layout(ac.adx_file(ac.CASES[1]))[1])
    for name, bad in bad_infos().items():
        if bad.audio_bytes:
            assert L().vga_adx_read_device(C.byref(bad), None, 0, 1, None, 0, None) == ARG, name
            per_file = last_error()
            with pytest.raises(_lib.ArgumentError, match=r"file 2: " + re.escape(per_file)):
                AdxFileSet.read_items([good, good, bad, good])
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        AdxFileSet.read_items([good, good], image_offsets=[0, -1])
    count = C.c_int64()
    ptrs = (C.c_void_p * 2)(C.addressof(good), None)
    assert L().vga_adx_files_read_items_for(ptrs, 2, None, 0, None, 0, C.byref(count)) == ARG and last_error().startswith("file 1: ")
    out = C.c_void_p()
    assert L().vga_adx_files_create_from_infos(None, 2, None, C.byref(out)) == ARG and not out.value


def test_null_arguments():
    tot = _lib.AdxFilesTotalsC()
    assert L().vga_adx_files_layout_for(None, 2, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_adx_files_layout_for(None, -1, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_adx_files_create(None, 0, None, None) == ARG
    assert L().vga_adx_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_adx_files_offsets(None, None, None, None) == ARG
    assert L().vga_adx_files_stats(None, None) == ARG
    L().vga_adx_files_destroy(None)
    assert L().vga_adx_write_device_v(None, None, None, None, None) == ARG
    assert L().vga_adx_read_device_v(None, None, None, None, None) == ARG
    files = (_lib.AdxFileC * 1)(ac.adx_file(ac.CASES[1]))
    items, count = (_lib.AdxFilesItemC * 1)(), C.c_int64()
    assert L().vga_adx_files_write_items_for(files, 1, None, 0, items, 1, C.byref(count)) == ARG and count.value == 3
    old = L().vga_adx_files_force_general_this_thread(1)
    assert old == 0 and L().vga_adx_files_force_general_this_thread(0) == 1


# ---------------------------------------------------------------- the headers alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, files, offsets in cases:
            offsets = list(offsets) if offsets is not None else []
            f.write(struct.pack("<3i", kind, len(files), len(offsets)))
            for x in files:
                if kind == 0:
                    f.write(struct.pack("<13i", x.channels, *[getattr(x.params, k) for k, _ in x.params._fields_]))
                elif x is None:
                    f.write(struct.pack("<7i", 0, 0, 0, 0, 0, 0, 1))
                else:
                    f.write(struct.pack("<7i", x.channel_count, x.frame_size, x.frame_count, x.audio_bytes, x.audio_offset, x.version, 0))
            f.write(struct.pack("<%dq" % len(offsets), *offsets))


def read_result(rd):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc:
        return rc, msg, None
    nfiles, nrows = rd.take("2i")
    r = {"first_channel": rd.take("%di" % nfiles), "image_off": rd.take("%dq" % nfiles), "image_size": rd.take("%di" % nfiles),
         "row_off": rd.take("%dq" % nrows), "row_bytes": rd.take("%di" % nrows), "totals": rd.take("2q"), "items": []}
    for _ in range(2):
        count = rd.take("i")[0]
        r["items"].append([tuple(rd.take("3iIi3q")) for _ in range(count)])
    return rc, msg, r


def as_tuples(items):
    return [(i.form, i.file, i.x, i.y, i.granule, i.begin, i.end, i.keep_end) for i in items]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("adx_files_host")
    exe = str(tmp / "adx_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name, (files, offs) in sorted(the_sets().items()):
        cases.append((0, files, offs))
        names.append(("set", name))
    cases.append((0, [], None))
    names.append(("empty", ""))
    for name in sorted(ac.REFUSED):
        for position in ("first", "middle", "last"):
            cases.append((0, refused_set(name, position)[0], None))
            names.append(("refused", name, position))
    for name in sorted(BAD_OFFSETS):
        cases.append((0,) + bad_offsets(name))
        names.append(("offsets", name))
    infos, sizes, odd = the_infos()
    cases += [(1, infos, None), (1, infos, odd), (1, [], None), (1, [infos[0], None], None)]
    names += [("infos", "packed"), ("infos", "odd"), ("infos", "empty"), ("infos", "null")]
    for name, bad in sorted(bad_infos().items()):
        cases.append((1, [infos[1], bad], None))
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
        m = ac.model(files, offs)
        assert r["first_channel"] == m["first_channel"] and r["row_off"] == m["audio_off"] and r["image_off"] == m["image_off"]
        assert r["image_size"] == m["image_size"] and r["totals"] == [m["audio_bytes"], m["image_bytes"]]
        assert r["row_bytes"] == [ac.row_bytes(f) for f in files for _ in range(f.channels)]
        for general in (0, 1):
            assert r["items"][general] == as_tuples(AdxFileSet.write_items(files, offs, general)), (name, general)
    _, (rc, msg, r) = driver[("empty", "")]
    assert rc == 0 and r["totals"] == [256, 256] and r["items"] == [[], []]
    infos, sizes, odd = the_infos()
    for which, offs in (("packed", None), ("odd", odd)):
        _, (rc, msg, r) = driver[("infos", which)]
        assert rc == 0, msg
        want_off, at = [], 0
        for sz in sizes:
            want_off.append(at)
            at = ac.up(at + sz, 16)
        assert r["image_off"] == (offs or want_off) and r["image_size"] == sizes
        assert r["totals"][1] == max(ac.up(o + s, 16) for o, s in zip(r["image_off"], sizes)) + 256
        rows, at = [], 0
        for i in infos:
            for _ in range(i.channel_count):
                rows.append(at)
                at += ac.up(i.audio_bytes, 16)
        assert r["row_off"] == rows and r["totals"][0] == at + 256
        assert r["row_bytes"] == [i.audio_bytes for i in infos for _ in range(i.channel_count)]
        for general in (0, 1):
            assert r["items"][general] == as_tuples(AdxFileSet.read_items(infos, offs, general)), (which, general)
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"] == [256, 256]


def test_host_layer_refusals(driver):
    for name in sorted(ac.REFUSED):
        for position in ("first", "middle", "last"):
            (_, files, _), (rc, msg, _) = driver[("refused", name, position)]
            at = refused_set(name, position)[1]
            arr, tot = (_lib.AdxFileC * len(files))(*files), _lib.AdxFilesTotalsC()
            assert L().vga_adx_files_layout_for(arr, len(files), None, None, None, None, C.byref(tot)) == rc == ac.REFUSED[name][1]
            assert msg == last_error() and msg.startswith("file %d: " % at), (name, position, msg)
    for name in sorted(BAD_OFFSETS):
        _, (rc, msg, _) = driver[("offsets", name)]
        assert rc == ARG and re.match(r"file \d: ", msg), (name, msg)
    for name in bad_infos():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == ARG and msg == "file 1: info does not describe an ADX file", (name, rc, msg)
    _, (rc, msg, _) = driver[("infos", "null")]
    assert rc == ARG and msg == "file 1: null info"
