"""include/vgaudio_hip_files/idsp_files.h without a GPU: the header's functions are exported and in the ctypes table with the
header's argument counts, vga_idsp_files_layout_for (host code) against a model built on tests/gc_containers_ref.py
(tests/idsp_files_cases.py) and against vga_gc_aligned_layout_for fed with the files' layout.channel, the regions the kernels
write (every image byte once, every row byte once), every refusal with its file and the per-file call's code and message,
that the GPU file's table of cases names every function the header declares, the moved hps_layout / idsp_layout
(vgaudio_amd/csrc/gc_stream_host.hpp; its HPS half: tests/test_hps_files_host.py) against gc_containers_ref and struct for struct against the library, and the HIP-free
host layer (vgaudio_amd/csrc/idsp_files_host.hpp) on its own under AddressSanitizer and UBSan."""
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
import idsp_files_cases as ic
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.idsp import IdspFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "idsp_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_idsp_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "idsp_files_host_driver.cpp")

NAMES = ["vga_idsp_files_layout_for", "vga_idsp_files_create", "vga_idsp_files_create_from_infos", "vga_idsp_files_destroy",
         "vga_idsp_files_totals_of", "vga_idsp_files_offsets", "vga_idsp_files_gc_files", "vga_idsp_files_ragged",
         "vga_idsp_write_device_v", "vga_idsp_read_device_v", "vga_idsp_files_write_regions_for", "vga_idsp_files_read_regions_for",
         "vga_idsp_files_stats"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
HEADER_KERNEL, AUDIO_KERNEL = 0, 1


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
    for name in ("vga_idsp_write_device_v", "vga_idsp_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("name", sorted(ic.CONFIGS))
def test_layout_is_the_per_file_layouts_packed(name):
    cfg, files = ic.config_of(name), ic.files_of(ic.CONFIGS[name][2])
    fc, io, tot = IdspFileSet.layout(files, configuration=cfg)
    m = ic.model(files, cfg)
    nch = sum(f.channels for f in files)
    assert (tot.files, tot.channels) == (len(files), nch)
    assert list(fc) == m["first_channel"] and list(io) == m["image_off"]
    assert (tot.pcm_samples, tot.adpcm_bytes, tot.image_bytes) == (m["pcm_samples"], m["adpcm_bytes"], m["image_bytes"])
    # an IDSP header is a multiple of 0x20 and the audio one of 8: the rounding of the offsets to 16 is at work
    assert all(s % 8 == 0 for s in m["image_size"]) and all(o % 16 == 0 for o in io)
    assert tot.image_bytes == ic.up(io[-1] + m["image_size"][-1], 16) + 256
    # outputs one at a time
    arr = (_lib.IdspFileC * len(files))(*files)
    f = L().vga_idsp_files_layout_for
    only, one = _lib.IdspFilesTotalsC(), np.zeros(len(files), np.int64)
    assert f(arr, len(files), C.byref(cfg), None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), C.byref(cfg), None, one.ctypes.data_as(C.POINTER(C.c_int64)), None) == 0 and np.array_equal(one, io)
    assert f(arr, len(files), C.byref(cfg), None, None, None) == ARG
    assert f(arr, len(files), None, None, None, C.byref(only)) == ARG


def test_the_cases_reach_what_they_are_for():
    lay = {n: ic.model(ic.files_of(t), ic.config(b, trim))["layouts"] for n, (b, trim, t) in ic.CONFIGS.items()}
    assert {b for b, _, _ in ic.CONFIGS.values()} == {0, 8, 0x10, 0x4000} and {t for _, t, _ in ic.CONFIGS.values()} == {0, 1}
    assert {t[0] for t in ic.FILES} >= {1, 2, 4, 5, 6, 8, 16, 255}
    b16 = lay["b16"]
    assert (b16[1]["channel_sample_count"], b16[1]["loop_start"]) == (57 + 13, 28)          # 15 -> 28: the re-encode
    assert (b16[2]["channel_sample_count"], b16[2]["loop_start"], b16[2]["sample_count"]) == (100, 28, 57)   # on the multiple; trimmed
    assert lay["b16-keep"][2]["sample_count"] == 100 and lay["b0"][1]["channel_sample_count"] == 100        # block size 0: no alignment
    assert gr.bytes_of(b16[6]["channel_sample_count"]) % 16 not in (0,) and gr.bytes_of(lay["b8"][6]["channel_sample_count"]) % 8   # a short last block
    rows = [gr.bytes_of(x["channel_sample_count"]) for x in lay["b4000"]]
    assert any(0 < n < 0x4000 for n in rows) and any(n > 0x4000 and n % 0x4000 for n in rows)   # rows shorter than a block; a short last block
    assert lay["b4000"][1]["loop_start"] == 28672
    assert b16[0]["channel_sample_count"] == 1 and b16[10]["audio_data_size"] == 0 and b16[10]["file_size"] == 0x40 + 0x60 * 2
    assert any(x["audio_data_size"] % 16 for x in lay["b0"]) and any(x["audio_data_size"] % 16 == 0 for x in lay["b0"])


@pytest.mark.parametrize("name", sorted(ic.CONFIGS))
def test_the_sets_inputs_are_the_aligned_sets_outputs(name):
    cfg, files = ic.config_of(name), ic.files_of(ic.CONFIGS[name][2])
    m = ic.model(files, cfg)
    lays = [ic.file_layout(f, cfg)[1] for f in files]
    gc = [_lib.GcFileC(f.channels, f.sample_rate, lay.channel) for f, lay in zip(files, lays)]
    for lay in lays:
        assert lay.channel.loop_alignment_multiple == (gr.byte_count_to_sample_count(cfg.block_size) if cfg.block_size else 0)
    fc, _, tot = AlignedFileSet.layout(gc)
    _, _, itot = IdspFileSet.layout(files, configuration=cfg)
    assert list(fc) == m["first_channel"]
    assert (tot.out_adpcm_bytes, tot.out_pcm_samples) == (itot.adpcm_bytes, itot.pcm_samples)
    import gc_aligned_cases as ga
    tuples = [(f.channels, c.sample_count, c.looping, c.loop_start, c.loop_end, c.samples_per_seek_table_entry, c.loop_alignment_multiple)
              for f, c in ((f, lay.channel) for f, lay in zip(files, lays))]
    assert ga.model(gc)["out_adpcm_off"] == m["adpcm_off"], tuples     # gc_aligned_cases' model: the output batch's rows


def test_an_empty_set_needs_no_gpu():
    fc, io, tot = IdspFileSet.layout([], configuration=ic.config(0x10))
    assert len(fc) == len(io) == 0
    assert (tot.files, tot.channels, tot.pcm_samples, tot.adpcm_bytes, tot.image_bytes) == (0, 0, 128, 256, 256)
    s = IdspFileSet([], configuration=ic.config(8))
    assert s.files == s.channels == 0 and s.gc_files() == []
    assert L().vga_idsp_write_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert L().vga_idsp_read_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == [] and s.stats() == (0, 0, 0, 0)
    s.close()
    r = IdspFileSet.from_infos([])
    assert r.files == 0 and L().vga_idsp_read_device_v(r._h, None, None, None, None, None, None, None) == 0
    assert L().vga_idsp_write_device_v(r._h, None, None, None, None, None, None, None) == 0
    r.close()
    n = C.c_int64(-1)
    assert L().vga_idsp_files_write_regions_for(None, 0, C.byref(ic.config(8)), None, 0, C.byref(n)) == 0 and n.value == 0
    assert L().vga_idsp_files_read_regions_for(None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0


# ---------------------------------------------------------------- the regions the kernels write (the library's hook)
def write_regions(files, cfg):
    arr, n = (_lib.IdspFileC * max(len(files), 1))(*files), C.c_int64()
    _lib.check(L().vga_idsp_files_write_regions_for(arr, len(files), C.byref(cfg), None, 0, C.byref(n)))
    out = (_lib.IdspFilesRegionC * max(n.value, 1))()
    assert n.value == 0 or L().vga_idsp_files_write_regions_for(arr, len(files), C.byref(cfg), out, n.value - 1, C.byref(n)) == ARG
    _lib.check(L().vga_idsp_files_write_regions_for(arr, len(files), C.byref(cfg), out, n.value, C.byref(n)))
    return [(r.kernel, r.index, r.granule, r.begin, r.end) for r in out[:n.value]]


def read_regions(infos, offsets):
    ptrs, n = (C.c_void_p * max(len(infos), 1))(*[C.addressof(i) for i in infos]), C.c_int64()
    offs = np.ascontiguousarray(offsets, dtype=np.int64) if offsets is not None else None
    o = offs.ctypes.data_as(C.POINTER(C.c_int64)) if offs is not None else None
    _lib.check(L().vga_idsp_files_read_regions_for(ptrs, len(infos), o, None, 0, C.byref(n)))
    out = (_lib.IdspFilesRegionC * max(n.value, 1))()
    _lib.check(L().vga_idsp_files_read_regions_for(ptrs, len(infos), o, out, n.value, C.byref(n)))
    return [(r.kernel, r.index, r.granule, r.begin, r.end) for r in out[:n.value]]


def check_write_regions(regions, files, m, what):
    """the header kernel's region and the audio items tile every image; no item lies outside an image; the granules are the
    header's rule"""
    per_file, seen = {}, set()
    for kernel, f, gran, begin, end in regions:
        per_file.setdefault(f, []).append((kernel, gran, begin, end))
    for f, lay in enumerate(m["layouts"]):
        ranges, items = [], per_file.pop(f)
        assert items[0] == (HEADER_KERNEL, 0, 0, lay["header_size"]) and lay["header_size"] % 0x20 == 0
        il, out = lay["interleave"], lay["audio_data_size"]
        blocks = -(-out // il)
        last_out = out - (blocks - 1) * il
        for kernel, gran, begin, end in items:
            ranges.append((begin, end))
            if kernel == HEADER_KERNEL:
                continue
            assert 0 <= begin < end <= lay["file_size"], (what, f, "an item outside its image")
            assert end - begin <= ic.CHUNK * gran and begin % gran == 0 and (end - lay["header_size"]) % gran == 0
            in_last = begin - lay["header_size"] >= (blocks - 1) * il * files[f].channels
            allowed = il % 16 == 0 and (not in_last or last_out % 16 == 0)
            assert gran == (16 if allowed else 8), (what, f, begin, gran)
            assert m["image_off"][f] % 16 == 0
            seen.add(gran)
        check_tiling(ranges, lay["file_size"], (what, f))
        assert (len(items) > 1) == (out > 0)
    assert not per_file
    return seen


def test_writer_regions_cover_every_image_byte_once():
    seen, several = set(), 0
    for name, (block, trim, tuples) in ic.CONFIGS.items():
        cfg, files = ic.config(block, trim), ic.files_of(tuples)
        regions = write_regions(files, cfg)
        seen |= check_write_regions(regions, files, ic.model(files, cfg), name)
        several += sum(1 for r in regions if r[0] == AUDIO_KERNEL and r[1] == 9) > 1
        assert [r[1] for r in regions if r[0] == HEADER_KERNEL] == list(range(len(files)))       # launch order: headers first
    assert seen == {8, 16} and several, "the cases do not reach every granule choice and a file of several items"


def info_of(nch, samples, il, length, audio_offset=None):
    i = _lib.IdspInfoC()
    i.channel_count, i.sample_count, i.interleave_size, i.interleave, i.audio_data_length = nch, samples, il, il or length, length
    i.audio_data_offset = 0x40 + 0x60 * nch if audio_offset is None else audio_offset
    i.header_size, i.channel_info_size, i.sample_rate, i.adpcm_bytes = 0x40, 0x60, ic.RATE, gr.bytes_of(samples)
    return i


def the_infos():
    """what the writers make, and foreign geometry: interleaves, lengths and offsets on no multiple of 16, of 8, of anything"""
    infos = [info_of(1, 1, 0x10, 0x10), info_of(2, 100, 8, 64), info_of(2, 100, 0x10, 64), info_of(5, 40000, 0x10, 22864),
             info_of(1, 40000, 0, 22864), info_of(2, 0, 0x10, 0), info_of(255, 15, 8, 16), info_of(3, 5000, 0x4000, 0x4000),
             info_of(2, 1000, 12, 580), info_of(2, 1000, 7, 575), info_of(3, 4000, 0x10, 2288, 0x40 + 0x60 * 3 + 5),
             info_of(2, 100, 0x10, 32)]                                # the last: the rows are longer than the audio (zero fill)
    sizes = [i.audio_data_offset + i.channel_count * i.audio_data_length for i in infos]
    odd, at = [], 3
    for sz in sizes:                                                   # any byte offsets
        odd.append(at)
        at = at + sz + 5
    return infos, sizes, odd


def granule_of(info, image_off):
    geometry = (image_off + info.audio_data_offset) | info.interleave | info.audio_data_length
    return 16 if geometry % 16 == 0 else 8 if geometry % 8 == 0 else 1


def check_read_regions(regions, infos, image_off, what):
    per_row, seen, c = {}, set(), 0
    for kernel, row, gran, begin, end in regions:
        assert kernel == AUDIO_KERNEL
        per_row.setdefault(row, []).append((gran, begin, end))
    for f, i in enumerate(infos):
        want = granule_of(i, image_off[f])
        for _ in range(i.channel_count):
            items = per_row.pop(c, [])
            for gran, begin, end in items:
                assert gran == want and begin % max(gran, 8) == 0 and begin < end <= i.adpcm_bytes and end - begin <= ic.CHUNK * gran
            if i.adpcm_bytes:
                check_tiling([(b, e) for _, b, e in items], i.adpcm_bytes, (what, f, c))
            else:
                assert not items
            seen.add(want)
            c += 1
    assert not per_row
    return seen


def test_reader_regions_cover_every_row_byte_once():
    infos, sizes, odd = the_infos()
    want_off, at = [], 0
    for sz in sizes:
        want_off.append(at)
        at = ic.up(at + sz, 16)
    assert check_read_regions(read_regions(infos, None), infos, want_off, "packed") == {16, 8, 1}
    assert 1 in check_read_regions(read_regions(infos, odd), infos, odd, "odd")
    on8 = [o + 8 for o in want_off]
    assert check_read_regions(read_regions(infos, on8), infos, on8, "8 mod 16") == {8, 1}


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code and message
REFUSED = {                                                            # name -> (the file, the configuration, the code)
    "channels0": ((0, 50, 0, 0, 0), ic.config(0x10), ARG),
    "channels256": ((256, 50, 0, 0, 0), ic.config(0x10), OP),
    "negative": ((1, -1, 0, 0, 0), ic.config(8), RANGE),
    "inverted": ((2, 50, 1, 30, 20), ic.config(0), RANGE),
    "loop_past_end": ((2, 50, 1, 10, 51), ic.config(0x10), RANGE),
    "negative_rate": ((2, 50, 0, 0, 0, -1), ic.config(0x10), RANGE),
    "block_negative": ((2, 50, 0, 0, 0), ic.config(-8), RANGE),
    "block12": ((2, 50, 0, 0, 0), ic.config(12), RANGE),
    "block0_no_audio": ((2, 0, 0, 0, 0), ic.config(0), OP),
    "too_large": ((255, 20_000_000, 0, 0, 0), ic.config(0x10), RANGE),
    "aligned_overflow": ((1, 0x7FFFFFF0, 1, 1, 0x7FFFFFF0), ic.config(0x10), RANGE),
}
OF_THE_SET = {"block_negative", "block12"}                             # the configuration is the set's: the first file meets it
GOOD = [(1, 1, 0, 0, 0), (2, 28, 0, 0, 0), (2, 100, 1, 14, 57)]


def refused_set(name, position):
    bad = ic.idsp_file(*REFUSED[name][0])
    good = ic.files_of(GOOD)
    at = {"first": 0, "middle": 2, "last": len(good)}[position]
    return good[:at] + [bad] + good[at:], 0 if name in OF_THE_SET else at


@pytest.mark.parametrize("position", ["first", "middle", "last"])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file_with_the_per_file_code_and_message(name, position):
    _, cfg, code = REFUSED[name]
    files, at = refused_set(name, position)
    rc, _ = ic.file_layout(files[at], cfg)
    per_file = last_error()
    assert rc == code and per_file
    arr, tot, out, n = (_lib.IdspFileC * len(files))(*files), _lib.IdspFilesTotalsC(), C.c_void_p(), C.c_int64()
    assert L().vga_idsp_files_layout_for(arr, len(files), C.byref(cfg), None, None, C.byref(tot)) == code
    assert last_error() == "file %d: %s" % (at, per_file)
    assert L().vga_idsp_files_create(arr, len(files), C.byref(cfg), C.byref(out)) == code and not out.value
    assert last_error() == "file %d: %s" % (at, per_file)
    assert L().vga_idsp_files_write_regions_for(arr, len(files), C.byref(cfg), None, 0, C.byref(n)) == code
    with pytest.raises(_lib._EXC[code], match=r"file %d\b" % at):
        IdspFileSet.layout(files, configuration=cfg)


def bad_infos():
    out = {}
    for name, (field, value, code) in {"interleave0": ("interleave", 0, ARG), "channels0": ("channel_count", 0, ARG),
                                       "channels256": ("channel_count", 256, ARG), "length": ("audio_data_length", -1, ARG),
                                       "bytes": ("adpcm_bytes", 5, ARG), "offset": ("audio_data_offset", -1, ARG),
                                       "too_large": ("audio_data_length", 0x7FFFFFF0, RANGE)}.items():
        i = info_of(2, 100, 0x10, 64)
        setattr(i, field, value)
        out[name] = (i, code)
    return out


def test_infos_the_per_file_reader_refuses_are_refused_with_their_file():
    good = lambda: info_of(2, 100, 0x10, 64)
    for name, (bad, code) in bad_infos().items():
        if name in ("interleave0", "channels0", "channels256", "length"):
            assert L().vga_idsp_read_device(C.byref(bad), None, 0, 1, None, 0, None) == ARG, name
            per_file = last_error()
        with pytest.raises(_lib._EXC[code], match=r"file 2\b"):
            IdspFileSet.from_infos([good(), info_of(1, 5, 8, 8), bad, good()])
        if name in ("interleave0", "channels0", "channels256", "length"):   # the per-file call's own message
            assert last_error() == "file 2: " + per_file, name
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        IdspFileSet.from_infos([good(), good()], image_offsets=[0, -8])
    out = C.c_void_p()
    assert L().vga_idsp_files_create_from_infos(None, 2, None, C.byref(out)) == ARG and not out.value
    assert L().vga_idsp_files_create_from_infos(None, 0, None, None) == ARG


def test_null_arguments():
    tot, cfg, n = _lib.IdspFilesTotalsC(), ic.config(0x10), C.c_int64()
    assert L().vga_idsp_files_layout_for(None, 2, C.byref(cfg), None, None, C.byref(tot)) == ARG
    assert L().vga_idsp_files_layout_for(None, -1, C.byref(cfg), None, None, C.byref(tot)) == ARG
    assert L().vga_idsp_files_create(None, 0, C.byref(cfg), None) == ARG
    assert L().vga_idsp_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_idsp_files_offsets(None, None, None) == ARG
    assert L().vga_idsp_files_gc_files(None, None) == ARG
    assert L().vga_idsp_files_stats(None, None) == ARG
    assert not L().vga_idsp_files_ragged(None)
    L().vga_idsp_files_destroy(None)
    assert L().vga_idsp_write_device_v(None, None, None, None, None, None, None, None) == ARG
    assert L().vga_idsp_read_device_v(None, None, None, None, None, None, None, None) == ARG
    assert L().vga_idsp_files_write_regions_for(None, 0, C.byref(cfg), None, 0, None) == ARG
    assert L().vga_idsp_files_write_regions_for(None, 0, None, None, 0, C.byref(n)) == ARG


# ---------------------------------------------------------------- the moved per-file layouts: unchanged
def idsp_grid():
    """params x channel counts for the moved idsp_layout: the case tables, and the refused ones"""
    grid = []
    for block, trim, tuples in ic.CONFIGS.values():
        for f in ic.files_of(tuples):
            grid.append((ic.params_of(f, ic.config(block, trim)), f.channels))
    for name in sorted(REFUSED):
        t, cfg, _ = REFUSED[name]
        grid.append((ic.params_of(ic.idsp_file(*t), cfg), t[0]))
    return grid


def test_per_file_layouts_are_the_reference_restatements():
    """vga_idsp_layout_for, whose code moved into gc_stream_host.hpp, still says what tests/gc_containers_ref.py says (the HPS
    half of that header is held by tests/test_hps_files_host.py)"""
    for block, trim, tuples in ic.CONFIGS.values():
        cfg = ic.config(block, trim)
        for f in ic.files_of(tuples):
            rc, lay = ic.file_layout(f, cfg)
            want = ic.ref_layout(f, cfg)
            assert rc == 0
            for k in ("loop_start", "loop_end", "sample_count", "channel_sample_count", "audio_data_size", "header_size", "file_size",
                      "start_addr", "end_addr"):
                assert getattr(lay, k) == want[k], (block, trim, f.channels, f.sample_count, k)
            assert lay.interleave_size == want["interleave"] and lay.channel_adpcm_bytes == gr.bytes_of(want["channel_sample_count"])


# ---------------------------------------------------------------- the headers alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, files, extra in cases:
            if kind == 0:
                f.write(struct.pack("<4i", 0, len(files), extra.block_size, extra.trim_file))
                for x in files:
                    f.write(struct.pack("<6i", x.channels, x.sample_rate, x.sample_count, x.looping, x.loop_start, x.loop_end))
            elif kind == 1:
                f.write(struct.pack("<3i", 1, len(files), int(extra is not None)))
                for i in files:
                    f.write(struct.pack("<7i", i.channel_count, i.sample_count, i.adpcm_bytes, i.interleave, i.audio_data_offset,
                                        i.audio_data_length, i.sample_rate))
                if extra is not None:
                    f.write(struct.pack("<%dq" % len(files), *extra))
            else:
                f.write(struct.pack("<2i", kind, extra) + bytes(files))


def read_result(rd, kind):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc:
        return rc, msg, None
    if kind == 2:
        size = C.sizeof(_lib.IdspLayoutC)
        raw = rd.d[rd.at:rd.at + size]
        rd.at += size
        return rc, msg, raw
    nfiles, nch = rd.take("2i")
    r = {"first_channel": rd.take("%di" % nfiles), "image_off": rd.take("%dq" % nfiles), "image_size": rd.take("%di" % nfiles),
         "counts": rd.take("%di" % nch), "adpcm_off": rd.take("%dq" % nch), "file": rd.take("%di" % nch), "totals": rd.take("3q")}
    r["tab"] = [rd.take("4I3i") for _ in range(nfiles)]
    r["regions"] = [tuple(rd.take("3i2q")) for _ in range(rd.take("i")[0])]
    return rc, msg, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("idsp_files_host")
    exe = str(tmp / "idsp_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name, (block, trim, tuples) in sorted(ic.CONFIGS.items()):
        cases.append((0, ic.files_of(tuples), ic.config(block, trim)))
        names.append(("set", name))
    cases.append((0, [], ic.config(0x10)))
    names.append(("empty", ""))
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            cases.append((0, refused_set(name, position)[0], REFUSED[name][1]))
            names.append(("refused", name, position))
    infos, sizes, odd = the_infos()
    cases += [(1, infos, None), (1, infos, odd), (1, [], None)]
    names += [("infos", "packed"), ("infos", "odd"), ("infos", "empty")]
    for name, (bad, _) in sorted(bad_infos().items()):
        cases.append((1, [info_of(2, 100, 0x10, 64), bad], None))
        names.append(("infos", "refused", name))
    for k, (p, nch) in enumerate(idsp_grid()):
        cases.append((2, p, nch))
        names.append(("idsp_layout", k))
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


def test_moved_layouts_are_the_librarys_struct_for_struct(driver):
    refused = 0
    for k, (p, nch) in enumerate(idsp_grid()):
        _, (rc, msg, raw) = driver[("idsp_layout", k)]
        lay = _lib.IdspLayoutC()
        want = L().vga_idsp_layout_for(C.byref(p), nch, C.byref(lay))
        assert rc == want, (k, rc, want, msg)
        if rc:
            assert msg == last_error() and msg, k
            refused += 1
        else:
            assert raw == bytes(lay), k
    assert refused == len(REFUSED)


def test_host_layer_layout_and_regions_are_the_librarys(driver):
    for name, (block, trim, tuples) in ic.CONFIGS.items():
        (_, files, cfg), (rc, msg, r) = driver[("set", name)]
        assert rc == 0, (name, msg)
        m = ic.model(files, cfg)
        for k in ("first_channel", "counts", "adpcm_off", "image_off", "image_size"):
            assert r[k] == m[k], (name, k)
        assert r["file"] == [i for i, f in enumerate(files) for _ in range(f.channels)]
        assert r["totals"] == [m["pcm_samples"], m["adpcm_bytes"], m["image_bytes"]]
        for t, lay, f in zip(r["tab"], m["layouts"], files):
            assert t[:3] == [gr.bytes_of(lay["channel_sample_count"]), lay["interleave"], lay["audio_data_size"]]
            assert t[4:] == [lay["header_size"], lay["header_size"], f.channels]
        assert r["regions"] == write_regions(files, cfg), name
    _, (rc, msg, r) = driver[("empty", "")]
    assert rc == 0 and r["totals"] == [128, 256, 256] and not r["regions"]
    infos, sizes, odd = the_infos()
    for which, offs in (("packed", None), ("odd", odd)):
        _, (rc, msg, r) = driver[("infos", which)]
        assert rc == 0, msg
        assert r["image_size"] == sizes and r["regions"] == read_regions(infos, offs)
        assert r["totals"][2] == max(ic.up(o + s, 16) for o, s in zip(r["image_off"], sizes)) + 256
        assert r["counts"] == [i.sample_count for i in infos for _ in range(i.channel_count)]
        for t, i, o in zip(r["tab"], infos, r["image_off"]):
            assert t[:3] == [i.audio_data_length, i.interleave, i.adpcm_bytes] and t[4] == i.audio_data_offset
            assert t[3] == {16: 1, 8: 0, 1: 4}[granule_of(i, o)]
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"][2] == 256 and not r["regions"]


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            (_, files, cfg), (rc, msg, _) = driver[("refused", name, position)]
            at = refused_set(name, position)[1]
            assert ic.file_layout(files[at], cfg)[0] == rc == REFUSED[name][2]
            assert msg == "file %d: %s" % (at, last_error()), (name, position, msg)
    for name, (_, code) in bad_infos().items():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == code and re.search(r"file 1\b", msg), (name, rc, msg)
