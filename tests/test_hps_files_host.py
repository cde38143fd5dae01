"""include/vgaudio_hip_files/hps_files.h without a GPU: the header's functions are exported and in the ctypes table with the
header's argument counts, vga_hps_files_layout_for (host code) against a model built on tests/gc_containers_ref.py
(tests/hps_files_cases.py) and against vga_gc_aligned_layout_for fed with the files' layout.channel, that the case table
reaches every shape of the block map it is for, that every size and offset of an HPS image is a multiple of 0x20, the regions
the kernels write (every image byte once, every row byte once), every refusal with its file and the per-file call's code and
message, that the GPU file's table of cases names every function the header declares, the per-file layouts and block maps
against gc_containers_ref, and the HIP-free host layer (vgaudio_amd/csrc/hps_files_host.hpp) on its own under
AddressSanitizer and UBSan."""
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

import gc_containers_ref as gr
import hps_files_cases as hc
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.hps import HpsFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "hps_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_hps_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "hps_files_host_driver.cpp")

NAMES = ["vga_hps_files_layout_for", "vga_hps_files_create", "vga_hps_files_create_from_infos", "vga_hps_files_destroy",
         "vga_hps_files_totals_of", "vga_hps_files_offsets", "vga_hps_files_gc_files", "vga_hps_files_ragged",
         "vga_hps_write_device_v", "vga_hps_read_device_v", "vga_hps_files_write_regions_for", "vga_hps_files_read_regions_for",
         "vga_hps_files_stats"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
HEADER_KERNEL, BLOCK_HEADER_KERNEL, AUDIO_KERNEL = 0, 1, 2


def L():
    return _lib.lib()


def last_error():
    L().vga_last_error.restype = C.c_char_p
    return L().vga_last_error().decode()


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
    for name in ("vga_hps_write_device_v", "vga_hps_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout against the model
def test_layout_is_the_per_file_layouts_packed():
    files = hc.the_files()
    fc, io, fb, tot = HpsFileSet.layout(files)
    m = hc.model(files)
    assert (tot.files, tot.channels, tot.blocks) == (len(files), sum(f.channels for f in files), m["blocks"])
    assert list(fc) == m["first_channel"] and list(io) == m["image_off"] and list(fb) == m["first_block"]
    assert (tot.pcm_samples, tot.adpcm_bytes, tot.image_bytes) == (m["pcm_samples"], m["adpcm_bytes"], m["image_bytes"])
    assert tot.image_bytes == hc.up(io[-1] + m["image_size"][-1], 16) + 256
    # outputs one at a time
    arr = (_lib.HpsFileC * len(files))(*files)
    f = L().vga_hps_files_layout_for
    only, one = _lib.HpsFilesTotalsC(), np.zeros(len(files), np.int64)
    i64p = C.POINTER(C.c_int64)
    assert f(arr, len(files), None, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), None, one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, io)
    assert f(arr, len(files), None, None, one.ctypes.data_as(i64p), None) == 0 and np.array_equal(one, fb)
    assert f(arr, len(files), None, None, None, None) == ARG


def test_the_cases_reach_what_they_are_for():
    """from the block maps (the library's, which test_per_file_layouts_are_the_reference_restatements holds to the restatement)"""
    maps = {k: hc.block_map(hc.hps_file(*t)) for k, t in hc.FILES.items()}
    count = {k: len(b) for k, (_, b) in maps.items()}
    full = lambda lay: lay.channel_size * 2                                # nibbles of a full block
    assert {t[0] for t in hc.FILES.values()} >= {1, 2, 4, 5, 6, 8, 16, 253}
    assert count["short"] == 1 and hc.FILES["short"][1] < 14 and count["full"] == 1                 # one block only
    lay, b = maps["full"]
    assert b[0].end_nibble + 1 == full(lay)                               # exactly one full block
    lay, b = maps["full+1"]
    assert count["full+1"] == 2 and b[0].end_nibble + 1 == full(lay) and b[1].end_nibble + 1 == 3   # ... plus one sample
    assert (b[1].end_nibble + 1) % 2 == 1                                 # a last block with an odd nibble count
    assert b[1].end_nibble + 1 < 0x40                                     # min(left, multiple of 0x40) took `left`
    lay, b = maps["blocks"]
    assert count["blocks"] >= 3 and not lay.looping and [x.end_nibble + 1 for x in b[:-1]] == [full(lay)] * (len(b) - 1)
    lay, b = maps["loop0"]                                                # a loop in block 0: the even re-division throughout
    assert lay.loop_block == 0 and count["loop0"] >= 3 and all(x.end_nibble + 1 < full(lay) for x in b)
    assert all((x.end_nibble + 1) % 0x40 == 0 for x in b[:-1]) and b[-1].next_offset == b[0].offset
    lay, b = maps["later"]                                                # a loop in a later block that needs the re-encode
    assert lay.alignment_needed and lay.loop_block == 2 and lay.loop_start == 28672 and hc.FILES["later"][3] // lay.alignment == 1
    assert b[-1].next_offset == b[2].offset and lay.sample_count == 40672
    lay, b = maps["on"]                                                   # a loop start already on the multiple
    assert not lay.alignment_needed and lay.loop_block == 2 and lay.loop_start == hc.FILES["on"][3]
    assert maps["align2"][0].alignment_needed and maps["mono"][0].alignment_needed and count["mono"] >= 2
    assert count["wide"] >= 3
    assert all(t[1] < 250_000 for t in hc.FILES.values() if t[0] == 1) and maps["mono"][0].sample_count < 250_000
    # several work items in one block, and blocks of one
    assert any(x.written_size > hc.CHUNK_BYTES for _, b in maps.values() for x in b)


def test_every_size_and_offset_of_an_image_is_a_multiple_of_0x20():
    files = hc.the_files()
    _, io, _, _ = HpsFileSet.layout(files)
    for f, at in zip(files, io):
        lay, blocks = hc.block_map(f)
        assert at % 16 == 0
        assert lay.file_size % 0x20 == 0 and lay.header_size % 0x20 == 0 and lay.block_header_size % 0x20 == 0
        for b in blocks:
            assert b.offset % 0x20 == 0 and b.byte_in_index % 0x20 == 0 and b.written_size % (0x20 * f.channels) == 0
            assert b.total_size == lay.block_header_size + b.written_size
        assert blocks[-1].byte_in_index + blocks[-1].channel_size == lay.channel_adpcm_bytes


def test_the_sets_inputs_are_the_aligned_sets_outputs():
    files = hc.the_files()
    m = hc.model(files)
    lays = [hc.file_layout(f)[1] for f in files]
    gc = [_lib.GcFileC(f.channels, f.sample_rate, lay.channel) for f, lay in zip(files, lays)]
    for f, lay in zip(files, lays):
        assert lay.channel.loop_alignment_multiple == gr.byte_count_to_sample_count(hc.up(0x10000 // f.channels, 0x20))
    assert len({lay.channel.loop_alignment_multiple for lay in lays}) >= 7          # it differs with the channel count
    fc, _, tot = AlignedFileSet.layout(gc)
    _, _, _, htot = HpsFileSet.layout(files)
    assert list(fc) == m["first_channel"]
    assert (tot.out_adpcm_bytes, tot.out_pcm_samples) == (htot.adpcm_bytes, htot.pcm_samples)
    import gc_aligned_cases as ga
    am = ga.model(gc)
    assert am["out_adpcm_off"] == m["adpcm_off"]                          # gc_aligned_cases' model: the output batch's rows


def test_an_empty_set_needs_no_gpu():
    fc, io, fb, tot = HpsFileSet.layout([])
    assert len(fc) == len(io) == len(fb) == 0
    assert (tot.files, tot.channels, tot.pcm_samples, tot.adpcm_bytes, tot.image_bytes, tot.blocks) == (0, 0, 128, 256, 256, 0)
    s = HpsFileSet([])
    assert s.files == s.channels == 0 and s.gc_files() == []
    assert L().vga_hps_write_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert L().vga_hps_read_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == [] and s.stats() == (0, 0, 0, 0)
    s.close()
    r = HpsFileSet.from_infos([])
    assert r.files == 0 and L().vga_hps_read_device_v(r._h, None, None, None, None, None, None, None) == 0
    assert L().vga_hps_write_device_v(r._h, None, None, None, None, None, None, None) == 0
    r.close()
    n = C.c_int64(-1)
    assert L().vga_hps_files_write_regions_for(None, 0, None, 0, C.byref(n)) == 0 and n.value == 0
    assert L().vga_hps_files_read_regions_for(None, None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0


# ---------------------------------------------------------------- the regions the kernels write (the library's hook)
def write_regions(files):
    arr, n = (_lib.HpsFileC * max(len(files), 1))(*files), C.c_int64()
    _lib.check(L().vga_hps_files_write_regions_for(arr, len(files), None, 0, C.byref(n)))
    out = (_lib.HpsFilesRegionC * max(n.value, 1))()
    assert n.value == 0 or L().vga_hps_files_write_regions_for(arr, len(files), out, n.value - 1, C.byref(n)) == ARG
    _lib.check(L().vga_hps_files_write_regions_for(arr, len(files), out, n.value, C.byref(n)))
    return [(r.kernel, r.index, r.granule, r.begin, r.end) for r in out[:n.value]]


def pointers(parsed):
    infos = (C.c_void_p * max(len(parsed), 1))(*[C.addressof(i) for i, _ in parsed])
    tables = (C.c_void_p * max(len(parsed), 1))(*[C.addressof(b) for _, b in parsed])
    return infos, tables


def read_regions(parsed, offsets):
    (infos, tables), n = pointers(parsed), C.c_int64()
    offs = np.ascontiguousarray(offsets, dtype=np.int64) if offsets is not None else None
    o = offs.ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None
    _lib.check(L().vga_hps_files_read_regions_for(infos, tables, len(parsed), o, None, 0, C.byref(n)))
    out = (_lib.HpsFilesRegionC * max(n.value, 1))()
    _lib.check(L().vga_hps_files_read_regions_for(infos, tables, len(parsed), o, out, n.value, C.byref(n)))
    return [(r.kernel, r.index, r.granule, r.begin, r.end) for r in out[:n.value]]


def test_writer_regions_cover_every_image_byte_once():
    files = hc.the_files()
    m = hc.model(files)
    regions = write_regions(files)
    kernels = [r[0] for r in regions]
    assert kernels == sorted(kernels)                                     # launch order: headers, block headers, bodies
    assert [r[1] for r in regions if r[0] == HEADER_KERNEL] == list(range(len(files)))
    assert sum(1 for k in kernels if k == BLOCK_HEADER_KERNEL) == m["blocks"]
    per_file = {}
    for kernel, f, gran, begin, end in regions:
        per_file.setdefault(f, []).append((kernel, gran, begin, end))
    several = 0
    for f, lay in enumerate(m["layouts"]):
        items = per_file.pop(f)
        assert items[0] == (HEADER_KERNEL, 0, 0, lay["header_size"])
        heads = [(b, e) for k, _, b, e in items if k == BLOCK_HEADER_KERNEL]
        assert heads == [(B["offset"], B["offset"] + lay["block_header_size"]) for B in lay["blocks"]]
        for kernel, gran, begin, end in items:
            assert 0 <= begin < end <= lay["file_size"], (f, "an item outside its image")
            if kernel == AUDIO_KERNEL:
                assert gran == 16 and begin % 16 == 0 and end % 16 == 0 and end - begin <= hc.CHUNK_BYTES
                inside = [B for B in lay["blocks"] if B["offset"] + lay["block_header_size"] <= begin
                          and end <= B["offset"] + lay["block_header_size"] + B["written_size"]]
                assert len(inside) == 1, (f, "an item that straddles two blocks")
        several += sum(1 for k, *_ in items if k == AUDIO_KERNEL) > len(lay["blocks"])
        check_tiling([(b, e) for _, _, b, e in items], lay["file_size"], f)
    assert not per_file and several


def the_parsed():
    """what the writer makes (the reference images of the case table), and foreign geometry: block sizes, strides and offsets on
    no multiple of 16"""
    images = list(hc.inputs()["given"])
    images.append(hc.foreign_image(2, [0x40 * 5, 0x40 * 3 + 7])[0])       # the last block ragged
    images.append(hc.foreign_image(3, [0x45, 0x40 * 200, 30], stride_pad=4)[0])   # odd bytes: out_offset 35, strides off 16
    images.append(hc.foreign_image(1, [0x40 * 40 + 4, 0x40], stride_pad=1)[0])
    parsed = [hc.parse(i) for i in images]
    # an image for reading reaches to the end of its last block, as a written file does
    sizes = [max(max(b[k].audio_offset + b[k].size, b[k].audio_offset + b[k].size // i.channel_count * (i.channel_count - 1) + b[k].audio_bytes) for k in range(i.block_count))
             for i, b in parsed]
    assert all(0 < n <= len(image) for image, n in zip(images, sizes))
    odd, at = [], 3
    for sz in sizes:                                                      # any byte offsets
        odd.append(at)
        at = at + sz + 5
    return images, parsed, sizes, odd


def check_read_regions(regions, parsed, image_off, what):
    per_row, seen, c = {}, set(), 0
    for kernel, row, gran, begin, end in regions:
        assert kernel == AUDIO_KERNEL
        per_row.setdefault(row, []).append((gran, begin, end))
    for f, (i, blocks) in enumerate(parsed):
        nch = i.channel_count
        want = {}
        for b in blocks[:i.block_count]:
            geometry = (image_off[f] + b.audio_offset) | (b.size // nch) | b.out_offset
            want[b.out_offset] = (16 if geometry % 16 == 0 else 1, b.out_offset + b.audio_bytes)
        for _ in range(nch):
            items = per_row.pop(c, [])
            for gran, begin, end in items:
                start = max(o for o in want if o <= begin)
                assert gran == want[start][0] and end <= want[start][1], (what, f, "an item that straddles two blocks")
                assert (begin - start) % (hc.CHUNK_BYTES if gran == 16 else hc.CHUNK_BYTES1) == 0
                assert end - begin <= (hc.CHUNK_BYTES if gran == 16 else hc.CHUNK_BYTES1) and end <= i.adpcm_bytes
                seen.add(gran)
            check_tiling([(b, e) for _, b, e in items], i.adpcm_bytes, (what, f, c))
            c += 1
    assert not per_row
    return seen


def test_reader_regions_cover_every_row_byte_once():
    images, parsed, sizes, odd = the_parsed()
    want_off, at = [], 0
    for sz in sizes:
        want_off.append(at)
        at = hc.up(at + sz, 16)
    assert check_read_regions(read_regions(parsed, None), parsed, want_off, "packed") == {16, 1}
    assert 1 in check_read_regions(read_regions(parsed, odd), parsed, odd, "odd")
    far = [(1 << 32) - 0x40 + o for o in want_off]
    assert 16 in check_read_regions(read_regions(parsed, far), parsed, far, "far")


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code and message
REFUSED = {                                                            # name -> (the file, the code)
    "channels0": ((0, 50, 0, 0, 0), ARG),
    "channels256": ((256, 50, 0, 0, 0), OP),
    "channels3": ((3, 50, 0, 0, 0), OP),                               # nch % 4 == 3
    "channels255": ((255, 50, 0, 0, 0), OP),
    "no_block": ((2, 0, 0, 0, 0), RANGE),
    "negative": ((1, -1, 0, 0, 0), RANGE),
    "inverted": ((2, 50, 1, 30, 20), RANGE),
    "loop_past_end": ((2, 50, 1, 10, 51), RANGE),
    "negative_rate": ((2, 50, 0, 0, 0, -1), RANGE),
    "too_large": ((8, 500_000_000, 0, 0, 0), RANGE),                   # a file past 2 GiB
}
GOOD = [(1, 1, 0, 0, 0), (2, 28, 0, 0, 0), (2, 100, 1, 14, 57)]


def refused_set(name, position):
    bad = hc.hps_file(*REFUSED[name][0])
    good = hc.files_of(GOOD)
    at = {"first": 0, "middle": 2, "last": len(good)}[position]
    return good[:at] + [bad] + good[at:], at


@pytest.mark.parametrize("position", ["first", "middle", "last"])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file_with_the_per_file_code_and_message(name, position):
    code = REFUSED[name][1]
    files, at = refused_set(name, position)
    rc, _ = hc.file_layout(files[at])
    per_file = last_error()
    assert rc == code and per_file
    arr, tot, out, n = (_lib.HpsFileC * len(files))(*files), _lib.HpsFilesTotalsC(), C.c_void_p(), C.c_int64()
    assert L().vga_hps_files_layout_for(arr, len(files), None, None, None, C.byref(tot)) == code
    assert last_error() == "file %d: %s" % (at, per_file)
    assert L().vga_hps_files_create(arr, len(files), C.byref(out)) == code and not out.value
    assert last_error() == "file %d: %s" % (at, per_file)
    assert L().vga_hps_files_write_regions_for(arr, len(files), None, 0, C.byref(n)) == code
    with pytest.raises(_lib._EXC[code], match=r"file %d\b" % at):
        HpsFileSet.layout(files)


def test_the_hist_check_is_the_per_file_calls_and_rows_of_the_aligned_length_pass_it():
    """a block whose hist index lies at or past the PCM row: vga_hps_write_device's refusal (VGA_ERR_OUT_OF_RANGE) is the
    check a set's create runs with pcm_len = the row's aligned sample count -- which every block of every case passes, as the
    last block starts inside the stream; one sample less and the per-file call refuses the last block of a file of several"""
    f = hc.hps_file(*hc.FILES["full+1"])
    lay, blocks = hc.block_map(f)
    p = hc.params_of(f)
    one = np.zeros(16, np.uint8).ctypes.data_as(C.c_void_p)              # never read: the call refuses before it launches
    short = blocks[-1].start_sample - 1
    rc = L().vga_hps_write_device(C.byref(p), f.channels, 1, one, lay.channel_adpcm_bytes, lay.channel_adpcm_bytes, one, None, None,
                                  one, short, short, one, lay.file_size, None)
    assert rc == RANGE and "hist1" in last_error()
    for g in hc.the_files():
        lay, blocks = hc.block_map(g)
        assert all(b.start_sample - 1 < lay.sample_count for b in blocks)


def good_parsed():
    return hc.parse(hc.inputs()["given"][hc.ORDER.index("four")])


def bad_parsed():
    """name -> ((info, blocks), code, the per-file reader refuses it too)"""
    out = {}
    for name, (field, value, per_file) in {"channels0": ("channel_count", 0, True), "channels256": ("channel_count", 256, True),
                                           "no_block": ("block_count", 0, True), "bytes": ("adpcm_bytes", 5, True),
                                           "samples": ("sample_count", 1, False)}.items():
        i, b = good_parsed()
        setattr(i, field, value)
        out[name] = ((i, b), ARG, per_file)
    for name, (field, value, per_file) in {"block_bytes": ("audio_bytes", -1, True), "block_out": ("out_offset", 1 << 20, True),
                                           "block_at": ("audio_offset", -32, False)}.items():
        i, b = good_parsed()
        setattr(b[0], field, value)
        out[name] = ((i, b), ARG, per_file)
    return out


def test_infos_the_per_file_reader_refuses_are_refused_with_their_file_and_its_message():
    one = np.zeros(16, np.uint8).ctypes.data_as(C.c_void_p)              # never read: the calls refuse before they launch
    for name, ((i, b), code, per_file) in bad_parsed().items():
        message = None
        if per_file:
            assert L().vga_hps_read_device(C.byref(i), b, one, 1 << 20, 1, one, 1 << 20, None) == ARG, name
            message = last_error()
        with pytest.raises(_lib._EXC[code], match=r"file 2\b"):
            HpsFileSet.from_infos([good_parsed(), good_parsed(), (i, b), good_parsed()])
        if per_file and name != "bytes":                                 # ("bytes": the reader says block 0 does not fit, the set
            assert last_error() == "file 2: " + message, name           #  meets the row length first)
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        HpsFileSet.from_infos([good_parsed(), good_parsed()], image_offsets=[0, -8])
    out = C.c_void_p()
    assert L().vga_hps_files_create_from_infos(None, None, 2, None, C.byref(out)) == ARG and not out.value
    assert L().vga_hps_files_create_from_infos(None, None, 0, None, None) == ARG


def test_null_arguments():
    tot, n = _lib.HpsFilesTotalsC(), C.c_int64()
    assert L().vga_hps_files_layout_for(None, 2, None, None, None, C.byref(tot)) == ARG
    assert L().vga_hps_files_layout_for(None, -1, None, None, None, C.byref(tot)) == ARG
    assert L().vga_hps_files_create(None, 0, None) == ARG
    assert L().vga_hps_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_hps_files_offsets(None, None, None, None) == ARG
    assert L().vga_hps_files_gc_files(None, None) == ARG
    assert L().vga_hps_files_stats(None, None) == ARG
    assert not L().vga_hps_files_ragged(None)
    L().vga_hps_files_destroy(None)
    assert L().vga_hps_write_device_v(None, None, None, None, None, None, None, None) == ARG
    assert L().vga_hps_read_device_v(None, None, None, None, None, None, None, None) == ARG
    assert L().vga_hps_files_write_regions_for(None, 0, None, 0, None) == ARG


# ---------------------------------------------------------------- the per-file layouts: what the restatement says
MORE = [                                                               # (channels, samples, looping, loop start, loop end)
    (1, 1, 0, 0, 0), (1, 114688, 0, 0, 0), (1, 114689, 0, 0, 0), (2, 200000, 1, 100, 150000), (2, 200000, 1, 57344, 200000),
    (8, 50000, 0, 0, 0), (8, 50000, 1, 14336, 50000), (8, 50000, 1, 20000, 49999), (4, 100, 1, 10, 90), (5, 30000, 0, 0, 0),
    (6, 30001, 1, 1, 30001), (16, 20000, 1, 9000, 19999), (253, 2000, 1, 600, 1999), (253, 504, 0, 0, 0), (253, 521, 0, 0, 0),
]
REFUSED_MORE = [(7, 100, 0, 0, 0)]


def hps_grid():
    """params x channel counts for hps_layout: the case table, further shapes, and the refused ones"""
    return ([hc.FILES[k] for k in hc.ORDER] + MORE + REFUSED_MORE
            + [t[:5] for t, _ in (REFUSED[k] for k in sorted(REFUSED)) if len(t) == 5])


def test_per_file_layouts_are_the_reference_restatements():
    """vga_hps_layout_for and vga_hps_block_map (gc_stream_host.hpp) say what tests/gc_containers_ref.py says on the case table"""
    for k in hc.ORDER + MORE:
        f = hc.hps_file(*(hc.FILES[k] if k in hc.FILES else k))
        lay, blocks = hc.block_map(f)
        want = hc.ref_layout(f)
        assert (lay.header_size, lay.file_size, lay.block_count, lay.loop_block) == (want["header_size"], want["file_size"],
                                                                                    len(want["blocks"]), want["loop_block"]), k
        assert (lay.loop_start, lay.loop_end, lay.sample_count, lay.alignment) == (want["loop_start"], want["loop_end"],
                                                                                   want["sample_count"], want["alignment"]), k
        assert lay.channel_adpcm_bytes == gr.bytes_of(want["channel_sample_count"]) and lay.block_header_size == want["block_header_size"]
        for b, w in zip(blocks, want["blocks"]):
            for name in ("offset", "next_offset", "start_sample", "byte_in_index", "channel_size", "written_size", "total_size", "end_nibble"):
                assert getattr(b, name) == w[name], (k, name)


# ---------------------------------------------------------------- the headers alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, files, extra in cases:
            if kind == 0:
                f.write(struct.pack("<2i", 0, len(files)))
                for x in files:
                    f.write(struct.pack("<6i", x.channels, x.sample_rate, x.sample_count, x.looping, x.loop_start, x.loop_end))
            elif kind == 1:
                f.write(struct.pack("<3i", 1, len(files), int(extra is not None)))
                for i, b in files:
                    f.write(struct.pack("<5i", i.channel_count, i.sample_count, i.adpcm_bytes, i.sample_rate, i.block_count))
                    f.write(bytes(b)[:max(i.block_count, 0) * C.sizeof(_lib.HpsBlockInfoC)])
                if extra is not None:
                    f.write(struct.pack("<%dq" % len(files), *extra))
            else:
                f.write(struct.pack("<2i", 3, extra) + bytes(files))


def read_result(rd, kind):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc:
        return rc, msg, None
    if kind == 3:
        size = C.sizeof(_lib.HpsLayoutC)
        raw = rd.d[rd.at:rd.at + size]
        rd.at += size
        more = _lib.HpsLayoutC.from_buffer_copy(raw).block_count * C.sizeof(_lib.HpsBlockC)
        raw += rd.d[rd.at:rd.at + more]
        rd.at += more
        return rc, msg, raw
    nfiles, nch, nblocks = rd.take("3i")
    r = {"first_channel": rd.take("%di" % nfiles), "image_off": rd.take("%dq" % nfiles), "first_block": rd.take("%dq" % nfiles),
         "image_size": rd.take("%di" % nfiles), "counts": rd.take("%di" % nch), "adpcm_off": rd.take("%dq" % nch),
         "pcm_off": rd.take("%dq" % nch), "totals": rd.take("4q")}
    r["blocks"] = [rd.take("8i") for _ in range(nblocks)]
    r["regions"] = [tuple(rd.take("3i2q")) for _ in range(rd.take("i")[0])]
    return rc, msg, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("hps_files_host")
    exe = str(tmp / "hps_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [(0, hc.the_files(), None), (0, [], None)], [("set",), ("empty",)]
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            cases.append((0, refused_set(name, position)[0], None))
            names.append(("refused", name, position))
    images, parsed, sizes, odd = the_parsed()
    cases += [(1, parsed, None), (1, parsed, odd), (1, [], None)]
    names += [("infos", "packed"), ("infos", "odd"), ("infos", "empty")]
    for name, (bad, _, _) in sorted(bad_parsed().items()):
        cases.append((1, [good_parsed(), bad], None))
        names.append(("infos", "refused", name))
    for k, t in enumerate(hps_grid()):
        cases.append((3, _lib.HpsParamsC(hc.RATE, t[1], t[2], t[3], t[4]), t[0]))
        names.append(("hps_layout", k))
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


def test_layouts_and_block_maps_are_the_librarys_struct_for_struct(driver):
    refused = 0
    for k, t in enumerate(hps_grid()):
        _, (rc, msg, raw) = driver[("hps_layout", k)]
        lay, p = _lib.HpsLayoutC(), _lib.HpsParamsC(hc.RATE, t[1], t[2], t[3], t[4])
        want = L().vga_hps_layout_for(C.byref(p), t[0], C.byref(lay))
        assert rc == want, (t, rc, want, msg)
        if rc:
            assert msg == last_error() and msg, t
            refused += 1
        else:
            blocks = (_lib.HpsBlockC * lay.block_count)()
            assert L().vga_hps_block_map(C.byref(p), t[0], blocks, lay.block_count) == 0
            assert raw == bytes(lay) + bytes(blocks), t
    assert refused == len(REFUSED) - 1 + len(REFUSED_MORE)                # (the negative rate is not a tuple of five)


def test_host_layer_layout_tables_and_regions_are_the_librarys(driver):
    (_, files, _), (rc, msg, r) = driver[("set",)]
    assert rc == 0, msg
    m = hc.model(files)
    for k in ("first_channel", "counts", "adpcm_off", "pcm_off", "image_off", "image_size", "first_block"):
        assert r[k] == m[k], k
    assert r["totals"] == [m["pcm_samples"], m["adpcm_bytes"], m["image_bytes"], m["blocks"]]
    want = [[f, B["offset"], B["next_offset"], B["written_size"], B["end_nibble"], B["start_sample"], B["byte_in_index"], B["channel_size"]]
            for f, lay in enumerate(m["layouts"]) for B in lay["blocks"]]
    assert r["blocks"] == want                                            # the block table: 32 bytes an entry
    assert r["regions"] == write_regions(files)
    _, (rc, msg, r) = driver[("empty",)]
    assert rc == 0 and r["totals"] == [128, 256, 256, 0] and not r["regions"]
    images, parsed, sizes, odd = the_parsed()
    for which, offs in (("packed", None), ("odd", odd)):
        _, (rc, msg, r) = driver[("infos", which)]
        assert rc == 0, msg
        assert r["image_size"] == sizes and r["regions"] == read_regions(parsed, offs)
        assert r["totals"][2] == max(hc.up(o + s, 16) for o, s in zip(r["image_off"], sizes)) + 256
        assert r["counts"] == [i.sample_count for i, _ in parsed for _ in range(i.channel_count)]
        assert r["totals"][3] == sum(i.block_count for i, _ in parsed)
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"][2] == 256 and not r["regions"]


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            (_, files, _), (rc, msg, _) = driver[("refused", name, position)]
            at = refused_set(name, position)[1]
            assert hc.file_layout(files[at])[0] == rc == REFUSED[name][1]
            assert msg == "file %d: %s" % (at, last_error()), (name, position, msg)
    for name, (_, code, _) in bad_parsed().items():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == code and re.search(r"file 1\b", msg), (name, rc, msg)
