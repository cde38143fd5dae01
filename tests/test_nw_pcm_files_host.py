"""include/vgaudio_hip_files/nw_pcm_files.h without a GPU: the header's functions are exported and in the ctypes table with the
header's argument counts and are declared in no other header, vga_nw_pcm_files_layout_for (host code) against a model built
from vga_nwstm_pcm_layout_for per file and the header's rounding rules (tests/nw_pcm_files_cases.py), the packed rows against
vga_wave_files_layout_for, the work items' tiling of every image and row in both forms, that the cases reach every conversion
in every form, every refusal with its file and the per-file call's code and message, that the GPU file's table of cases names
every function the header declares, tests/nwstm_pcm_ref.py's layout against every per-file layout of the cases, and the
HIP-free host layer (vgaudio_amd/csrc/nw_pcm_files_host.hpp) on its own under AddressSanitizer and UBSan."""
import ast
import ctypes as C
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

import nw_pcm_files_cases as nc
import nwstm_pcm_ref as ref
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib, nwstm
from vgaudio_amd.nwstm import NwPcmFileSet
from vgaudio_amd.wave import WaveFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "nw_pcm_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_nw_pcm_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "nw_pcm_files_host_driver.cpp")

NAMES = ["vga_nw_pcm_files_layout_for", "vga_nw_pcm_files_create", "vga_nw_pcm_files_create_from_infos", "vga_nw_pcm_files_destroy",
         "vga_nw_pcm_files_totals_of", "vga_nw_pcm_files_offsets", "vga_nwstm_pcm_write_device_v", "vga_nwstm_pcm_read_device_v",
         "vga_nw_pcm_files_write_items_for", "vga_nw_pcm_files_read_items_for", "vga_nw_pcm_files_stats",
         "vga_nw_pcm_files_force_general_this_thread"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
HEADER_ITEM, VECTOR, GENERAL = nc.HEADER_ITEM, nc.VECTOR, nc.GENERAL
CONFIG_NAMES = sorted(nc.CONFIGS)
i64p = C.POINTER(C.c_int64)


def L():
    return _lib.lib()


def last_error():
    L().vga_last_error.restype = C.c_char_p
    return L().vga_last_error().decode()


def per_file_layout(file, cfg, codec):
    return NwPcmFileSet.file_layout(file, cfg, codec)


def the_set(name, layout="packed"):
    """(files, config, codec, pcm offsets, image offsets, image sizes) of a named configuration"""
    cfg, codec = nc.config_c(name)
    cases = nc.CONFIGS[name][5]
    files = nc.files_of(cases)
    sizes = [per_file_layout(f, cfg, codec).file_size for f in files]
    if layout == "packed":
        return files, cfg, codec, None, None, sizes
    return files, cfg, codec, nc.explicit_pcm_offsets(nc.counts_of(cases)), [o + 48 for o in nc.image_offsets_at(sizes, 0, gap=21)], sizes


def c_files(files):
    return (_lib.NwFileC * max(len(files), 1))(*files)


def offsets_arg(values):
    return (C.c_int64 * len(values))(*values) if values is not None else None


def write_items(name, layout="packed", general=False):
    files, cfg, codec, po_, io_, _ = the_set(name, layout)
    count = C.c_int64()
    call = L().vga_nw_pcm_files_write_items_for
    args = (c_files(files), len(files), C.byref(cfg), codec, offsets_arg(po_), offsets_arg(io_), int(general))
    _lib.check(call(*args, None, 0, C.byref(count)))
    items = (_lib.NwPcmFilesItemC * max(count.value, 1))()
    _lib.check(call(*args, items, count.value, C.byref(count)))
    return list(items[:count.value])


_infos = {}


def the_infos(name):
    """(infos, image sizes) of the reference images of a named configuration, or of the mixed reading set"""
    if name not in _infos:
        images = nc.mixed_read_side()[0] if name == "mixed" else nc.reference(name)[2]
        _infos[name] = ([nc.parse(i) for i in images], [len(i) for i in images])
    return _infos[name]


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
    for name in ("vga_nwstm_pcm_write_device_v", "vga_nwstm_pcm_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once",
                "test_offsets_past_4_gib", "test_refused_calls_launch_nothing"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source and "FarBuffer" in source


# ---------------------------------------------------------------- the cases
def test_the_cases_reach_what_they_are_for():
    """every conversion in every form by at least two files, a truncating looping file, a file of no samples and a file of
    several work items in sets of both forms: from the items hooks, so that a regrouping of the cases cannot pass silently"""
    assert {(c[0], c[1]) for c in nc.SMALL} >= {(1, 1), (2, 28), (3, 15), (2, 100), (2, 57), (1, 100), (255, 15), (2, 0)}
    at = nc.SMALL.index((2, 57, 0, 0, 0))
    assert nc.SMALL[at - 1] == (2, 100, 1, 15, 57) and nc.SMALL[at + 1] == (1, 100, 1, 50, 100)
    assert (2, 2 * 4096 + 5, 0, 0, 0) in nc.big(nc.PCM16) and (2, 2 * 8192 + 3, 0, 0, 0) in nc.big(nc.PCM8)
    kinds = {(t, codec, nc.big_endian(n)) for n, (t, codec, _, _, _, _) in nc.CONFIGS.items()}
    assert kinds >= {(t, c, True) for t in (nc.RSTM, nc.CSTM, nc.FSTM) for c in (nc.PCM8, nc.PCM16)}
    assert kinds >= {(t, c, False) for t in (nc.CSTM, nc.FSTM) for c in (nc.PCM8, nc.PCM16)}
    assert {(codec, spi) for _, codec, _, _, spi, _ in nc.CONFIGS.values()} >= {(nc.PCM16, 8), (nc.PCM16, 16), (nc.PCM16, 5), (nc.PCM16, 0),
                                                                                 (nc.PCM8, 16), (nc.PCM8, 32), (nc.PCM8, 1001), (nc.PCM8, 0)}
    for side in ("write", "read"):
        reached, truncating, empty, several = {}, set(), set(), set()
        for name in CONFIG_NAMES:
            cases = nc.CONFIGS[name][5]
            if side == "write":
                items = [i for i in write_items(name) if i.form != HEADER_ITEM]
            else:
                items = NwPcmFileSet.read_items(the_infos(name)[0])
            assert {i.conv for i in items} == {nc.conv_of(name)}
            per = {}
            for i in items:
                reached.setdefault((i.conv, i.form), set()).add((name, i.file))
                per.setdefault((i.file, i.x), []).append(i)
            forms = {i.form for i in items}
            assert len(forms) == 1 or name == "cstm8_be_i1001", (name, forms)
            for f, case in enumerate(cases):
                mine = {i.form for i in items if i.file == f}
                if case[2] and case[4] < case[1]:
                    truncating |= mine
                if case[1] == 0:
                    assert not mine
                    empty |= forms
            several |= {v[0].form for v in per.values() if len(v) > 1}
        for conv in (nc.COPY, nc.SWAP16, nc.PCM8_CONV):
            for form in (VECTOR, GENERAL):
                assert len(reached.get((conv, form), ())) >= 2, (side, conv, form)
        assert truncating == empty == several == {VECTOR, GENERAL}, (side, truncating, empty, several)


def test_the_restatements_layout_is_every_per_file_layout():
    for name in CONFIG_NAMES:
        target, codec, endian, version, spi, cases = nc.CONFIGS[name]
        cfg, _ = nc.config_c(name)
        for file, (nch, n, looping, ls, le) in zip(nc.files_of(cases), cases):
            got = per_file_layout(file, cfg, codec)
            want = ref.layout(target, codec, nch, n, bool(looping), ls, le, spi or None, version=version or None)
            for key, value in want.items():
                if hasattr(got, key):
                    assert getattr(got, key) == value, (name, (nch, n), key)
            assert got.endianness == int(nc.big_endian(name)) and got.channel_sample_count == n


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("layout", ["packed", "explicit"])
@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_layout_is_the_model(name, layout):
    files, cfg, codec, po_, io_, sizes = the_set(name, layout)
    cases = nc.CONFIGS[name][5]
    arr, n = c_files(files), len(files)
    nch = sum(f.channels for f in files)
    fc, po2, io2, tot = np.zeros(n, np.int32), np.zeros(nch, np.int64), np.zeros(n, np.int64), _lib.NwPcmFilesTotalsC()
    f = L().vga_nw_pcm_files_layout_for
    _lib.check(f(arr, n, C.byref(cfg), codec, offsets_arg(po_), offsets_arg(io_), fc.ctypes.data_as(C.POINTER(C.c_int)),
                 po2.ctypes.data_as(i64p), io2.ctypes.data_as(i64p), C.byref(tot)))
    m = nc.model(nc.counts_of(cases), sizes, po_, io_)
    assert (tot.files, tot.channels) == (n, m["channels"]) == (n, nch)
    assert list(fc) == m["first_channel"] and list(po2) == m["pcm_off"] and list(io2) == m["image_off"]
    assert (tot.pcm_samples, tot.image_bytes) == (m["pcm_samples"], m["image_bytes"])
    assert all(o % 16 == 0 for o in io2)
    # the rows are vga_wave_files_layout_for's for the same counts
    wav = [_lib.WaveFileC(c[0], 16, _lib.WaveParamsC(nc.RATE, c[1], 0, 0, 0)) for c in cases]
    _, wave_rows, _, wave_tot = WaveFileSet.layout(wav, po_)
    assert list(wave_rows) == list(po2) and wave_tot.pcm_samples == tot.pcm_samples
    # the Python mirror, and the outputs one at a time
    fc3, po3, io3, tot3 = NwPcmFileSet.layout(files, cfg.target, configuration_of(name), po_, io_)
    assert list(fc3) == list(fc) and list(po3) == list(po2) and list(io3) == list(io2) and tot3.image_bytes == tot.image_bytes
    only = _lib.NwPcmFilesTotalsC()
    assert f(arr, n, C.byref(cfg), codec, offsets_arg(po_), offsets_arg(io_), None, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, n, C.byref(cfg), codec, offsets_arg(po_), offsets_arg(io_), None, None, None, None) == ARG


def configuration_of(name):
    target, codec, endian, version, spi, _ = nc.CONFIGS[name]
    c = nwstm.BxstmConfiguration(Codec=nwstm.NwCodec(codec))
    if spi:
        c.SamplesPerInterleave = spi
    if endian is not None:
        c.Endianness = nwstm.Endianness(endian)
    if version:
        c.Version = nwstm.NwVersion.FromPacked(version)
    return c


def test_an_empty_set_needs_no_gpu():
    cfg, codec = nc.config_c("rstm16_default")
    fc, po_, io_, tot = NwPcmFileSet.layout([], nc.RSTM, configuration_of("rstm16_default"))
    assert len(fc) == len(po_) == len(io_) == 0 and (tot.files, tot.channels, tot.pcm_samples, tot.image_bytes) == (0, 0, 128, 256)
    s = NwPcmFileSet([], nc.RSTM, configuration_of("rstm16_default"))
    assert s.files == s.channels == 0 and s.stats() == (0, 0, 0, 0)
    assert L().vga_nwstm_pcm_write_device_v(s._h, None, None, None) == 0
    assert L().vga_nwstm_pcm_read_device_v(s._h, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == []
    s.close()
    r = NwPcmFileSet.from_infos([])
    assert r.files == 0 and L().vga_nwstm_pcm_read_device_v(r._h, None, None, None) == 0
    r.close()
    assert NwPcmFileSet.write_items([], nc.RSTM, configuration_of("rstm16_default")) == [] and NwPcmFileSet.read_items([]) == []


# ---------------------------------------------------------------- the work items: tiling and forms
def check_write_items(name, layout, general):
    files, cfg, codec, po_, io_, sizes = the_set(name, layout)
    items = write_items(name, layout, general)
    forms = [i.form for i in items]
    assert forms == sorted(forms)                                      # the launch order: headers, vector items, general items
    per = {}
    for it in items:
        per.setdefault(it.file, []).append(it)
    seen = set()
    for f, file in enumerate(files):
        N = per_file_layout(file, cfg, codec)
        mine = per.pop(f)
        head = [i for i in mine if i.form == HEADER_ITEM]
        data = [i for i in mine if i.form != HEADER_ITEM]
        assert len(head) == 1 and (head[0].begin, head[0].end) == (0, N.audio_data_offset), (name, f)
        total = N.audio_data_size * file.channels
        assert N.audio_data_offset + total == N.file_size == sizes[f]
        if total:
            check_tiling([(i.begin - N.audio_data_offset, i.end - N.audio_data_offset) for i in data], total, (name, f))
        else:
            assert not data
        assert len({i.form for i in data}) <= 1 and all(i.x == f and i.begin == N.audio_data_offset + i.y * nc.CHUNK_BYTES for i in data)
        assert not general or all(i.form == GENERAL for i in data)
        seen |= {i.form for i in data}
    assert not per
    return seen


@pytest.mark.parametrize("name", CONFIG_NAMES)
def test_writer_work_items_tile_every_image(name):
    own = check_write_items(name, "packed", False)
    assert check_write_items(name, "packed", True) == {GENERAL}
    explicit = check_write_items(name, "explicit", False)
    assert GENERAL in explicit                                         # rows off 8 samples
    spi, codec = nc.CONFIGS[name][4], nc.CONFIGS[name][1]
    vector = (spi or 4096) * (2 if codec == nc.PCM16 else 1) % 16 == 0
    assert (VECTOR in own) == vector or name == "cstm8_be_i1001", (name, own)


@pytest.mark.parametrize("which", ["packed", "odd", "rows"])
@pytest.mark.parametrize("name", CONFIG_NAMES + ["mixed"])
def test_reader_work_items_tile_every_row(name, which):
    infos, sizes = the_infos(name)
    io_ = nc.image_offsets_at(sizes, 1) if which == "odd" else None
    po_ = nc.explicit_pcm_offsets([[i.sample_count] * i.channel_count for i in infos]) if which == "rows" else None
    row0, n = [], 0
    for i in infos:
        row0.append(n)
        n += i.channel_count
    for general in (False, True):
        items = NwPcmFileSet.read_items(infos, po_, io_, general)
        assert not [i for i in items if i.form == HEADER_ITEM]
        forms = [i.form for i in items]
        assert forms == sorted(forms)
        if general or which == "odd":
            assert set(forms) <= {GENERAL}
        rows = {}
        for it in items:
            info = infos[it.file]
            assert row0[it.file] <= it.x < row0[it.file] + info.channel_count
            assert it.begin == it.y * nc.CHUNK_BYTES * (2 if info.codec == nc.PCM8 else 1)
            rows.setdefault(it.x, []).append((it.begin, it.end))
        for f, info in enumerate(infos):
            for c in range(info.channel_count):
                if info.sample_count:
                    check_tiling(rows.pop(row0[f] + c), info.sample_count * 2, (name, which, f, c))
        assert not rows


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code and message
GOOD = [(2, 100, 0, 0, 0), (1, 33, 1, 1, 30), (3, 9, 0, 0, 0)]
REFUSED = {                                                  # name -> (configuration, codec, case, code)
    "channels_0": ("rstm16_i8", None, (0, 100, 0, 0, 0), ARG),
    "channels_256": ("rstm16_i8", None, (256, 1, 0, 0, 0), ARG),
    "negative_samples": ("cstm8_le_i32", None, (2, -1, 0, 0, 0), RANGE),
    "loop_past_the_end": ("fstm16_be_default", None, (2, 100, 1, 5, 101), RANGE),
    "loop_backwards": ("rstm8_default", None, (2, 100, 1, 50, 20), RANGE),
    "too_large": ("rstm16_default", None, (255, 0x7FFFFFF, 0, 0, 0), RANGE),
    "cstm_2_3": ("cstm_2_3", nc.PCM16, (2, 100, 0, 0, 0), OP),
    "fstm_0_4": ("fstm_0_4", nc.PCM8, (2, 100, 0, 0, 0), OP),
}


def refused_config(name):
    config, codec = REFUSED[name][:2]
    if config in nc.REFUSED_VERSIONS:
        target, version = nc.REFUSED_VERSIONS[config]
        return _lib.NwFileConfigC(target, 0, 0, 0, 0, 0, version, -1), codec
    return nc.config_c(config)


def refused_set(name, position):
    bad = nc.files_of([REFUSED[name][2]])[0]
    good = nc.files_of(GOOD)
    if REFUSED[name][0] in nc.REFUSED_VERSIONS:                        # the configuration refuses every file: the first is named
        return good + [bad], 0
    at = {"first": 0, "middle": 2, "last": len(good)}[position]
    return good[:at] + [bad] + good[at:], at


def per_file_refusal(file, cfg, codec):
    """what vga_nwstm_pcm_write_device says to this file alone (its checks come before any device work)"""
    p = NwPcmFileSet.file_params(file, cfg)
    rc = L().vga_nwstm_pcm_write_device(C.byref(p), codec, file.channels, 1, None, C.c_void_p(16), 0, 1 << 40, C.c_void_p(16), 1 << 40, None)
    return rc, last_error()


@pytest.mark.parametrize("position", ["first", "middle", "last"])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file_with_the_per_file_code_and_message(name, position):
    code = REFUSED[name][3]
    cfg, codec = refused_config(name)
    files, at = refused_set(name, position)
    arr, tot, out, count = c_files(files), _lib.NwPcmFilesTotalsC(), C.c_void_p(), C.c_int64()
    assert L().vga_nw_pcm_files_layout_for(arr, len(files), C.byref(cfg), codec, None, None, None, None, None, C.byref(tot)) == code
    message = last_error()
    rc, per_file = per_file_refusal(files[at], cfg, codec)
    assert rc == code and per_file and message == "file %d: %s" % (at, per_file)
    assert L().vga_nw_pcm_files_create(arr, len(files), C.byref(cfg), codec, None, None, C.byref(out)) == code and not out.value
    assert last_error() == message
    assert L().vga_nw_pcm_files_write_items_for(arr, len(files), C.byref(cfg), codec, None, None, 0, None, 0, C.byref(count)) == code
    assert last_error() == message


def test_refusals_of_the_set_itself():
    cfg, codec = nc.config_c("rstm16_i8")
    files = nc.files_of([(2, 100, 0, 0, 0), (2, 100, 0, 0, 0)])        # four rows of 100 samples; two images of the same size
    size = per_file_layout(files[0], cfg, codec).file_size
    arr, tot = c_files(files), _lib.NwPcmFilesTotalsC()
    f = L().vga_nw_pcm_files_layout_for

    def call(po_=None, io_=None, config=cfg, the_codec=codec):
        return f(arr, 2, C.byref(config) if config is not None else None, the_codec, offsets_arg(po_), offsets_arg(io_), None, None, None, C.byref(tot))

    assert call([0, 100, 201, 301], [0, nc.up(size, 16)]) == 0
    assert (tot.pcm_samples, tot.image_bytes) == (401 + 128, 2 * nc.up(size, 16) + 256)
    assert call([301, 201, 100, 0], [nc.up(size, 16) + 32, 16]) == 0                       # any order, any sample boundary
    for po_, io_, file, word in (([-1, 100, 201, 301], None, 0, "negative"), ([0, 100, 201, 250], None, 1, "overlaps"),
                                 (None, [0, -16], 1, "negative"), (None, [0, size - 16], 1, "overlaps"), (None, [0, size + 8], 1, "multiple of 16"),
                                 (None, [8, 2 * size], 0, "multiple of 16")):
        assert call(po_, io_) == ARG and last_error().startswith("file %d: " % file) and word in last_error(), (po_, io_, last_error())
    for po_, io_, file in (([0, (1 << 61) + 1, 201, 301], None, 0), (None, [0, (1 << 62) + 16], 1)):
        assert call(po_, io_) == RANGE and last_error().startswith("file %d: " % file) and "2^62" in last_error()
    assert call(the_codec=2) == ARG and "codec 2" in last_error()
    assert call(the_codec=7) == ARG and call(the_codec=-1) == ARG
    assert call(config=None) == ARG and "configuration" in last_error()
    # more than 2^31 rows: refused before a row is placed
    one = nc.files_of([(255, 0, 0, 0, 0)])[0]
    n = 0x7FFFFFFF // 255 + 1
    many = (_lib.NwFileC * n)(*([one] * n))
    assert f(many, n, C.byref(cfg), codec, None, None, None, None, None, C.byref(tot)) == ARG
    assert last_error() == "file %d: more than 2^31 rows" % (n - 1)


def bad_infos():
    """name -> (info, code, vga_nwstm_pcm_read_device refuses it with that code too)"""
    infos, _ = the_infos("rstm16_i8")
    base16 = next(i for i in infos if i.channel_count == 2 and i.sample_count > 20)
    infos8, _ = the_infos("cstm8_le_i32")
    base8 = next(i for i in infos8 if i.channel_count == 2 and i.sample_count > 20)
    out = {}
    for name, (base, field, value, code, per_file) in {
            "gc_adpcm": (base16, "codec", 2, ARG, True), "codec_9": (base8, "codec", 9, ARG, True),
            "no_channels": (base16, "channel_count", 0, ARG, True), "interleave_0": (base8, "interleave_size", 0, ARG, True),
            "length_negative": (base16, "audio_data_length", -4, ARG, True), "length_not_divisible": (base8, "audio_data_length", base8.audio_data_length + 1, ARG, True),
            "bytes_not_the_samples": (base16, "adpcm_bytes", base16.adpcm_bytes - 2, ARG, True),
            "offset_negative": (base16, "audio_data_offset", -32, ARG, False), "channels_256": (base8, "channel_count", 256, ARG, False),
            "interleave_odd_pcm16": (base16, "interleave_size", 15, OP, False),
            "image_past_2_gib": (base8, "audio_data_offset", 0x7FFFFFF0, RANGE, False)}.items():
        i = _lib.NwInfoC.from_buffer_copy(base)
        setattr(i, field, value)
        if name == "channels_256":
            i.audio_data_length = 256 * 64
        out[name] = (i, code, per_file)
    return out


def test_infos_the_per_file_reader_refuses_are_refused_with_their_file():
    infos, _ = the_infos("rstm16_i8")
    good = infos[1]
    for position, at in (("first", 0), ("middle", 2), ("last", 3)):
        for name, (bad, code, per_file) in bad_infos().items():
            group = [good, good, good]
            group.insert(at, bad)
            with pytest.raises(_lib._EXC[code], match=r"file %d: " % at) as e:
                NwPcmFileSet.read_items(group)
            if per_file:                                               # the per-file call refuses before it looks at a pointer
                rc = L().vga_nwstm_pcm_read_device(C.byref(bad), C.c_void_p(16), 1 << 40, 1, C.c_void_p(16), 0, 1 << 40, None)
                assert rc == code and str(e.value) == "file %d: %s" % (at, last_error()), name
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        NwPcmFileSet.read_items([good, good], image_offsets=[0, -1])
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b.*overlaps"):
        NwPcmFileSet.read_items([good, good], pcm_offsets=[0, 28, 27, 400])
    assert NwPcmFileSet.read_items([good, good], image_offsets=[3, 1])  # read images may overlap and start at any byte
    count, out = C.c_int64(), C.c_void_p()
    ptrs = (C.c_void_p * 2)(C.addressof(good), None)
    assert L().vga_nw_pcm_files_read_items_for(ptrs, 2, None, None, 0, None, 0, C.byref(count)) == ARG and last_error() == "file 1: null info"
    assert L().vga_nw_pcm_files_create_from_infos(None, 2, None, None, C.byref(out)) == ARG and not out.value


def test_the_per_file_reader_keeps_its_codes_and_order():
    """vga_nwstm_pcm_read_device after its info checks moved into nw_host.hpp"""
    infos, _ = the_infos("rstm16_i8")
    info = _lib.NwInfoC.from_buffer_copy(infos[1])
    call = lambda i, nfiles=1, kind=0, rows=C.c_void_p(16): L().vga_nwstm_pcm_read_device(C.byref(i), C.c_void_p(16), 1 << 40, nfiles, rows, kind, 1 << 40, None)
    assert L().vga_nwstm_pcm_read_device(None, None, 0, 1, None, 0, 0, None) == ARG and last_error() == "null / negative argument"
    assert call(info, nfiles=-1) == ARG and last_error() == "null / negative argument"
    assert call(info, kind=7) == ARG and last_error() == "unknown sample kind 7"
    assert call(info, kind=1) == ARG and last_error() == "a PCM16 stream is read to VGA_SAMPLES_S16 rows"
    info.codec = 2
    assert call(info, kind=7) == ARG and last_error() == "info is not a PCM8 / PCM16 stream (vga_nwstm_pcm_parse)"      # the codec first
    info.codec, info.channel_count = 1, 0
    assert call(info) == ARG and last_error() == "info does not describe a stream"
    assert call(info, nfiles=0) == 0                                   # no files: the geometry is not looked at
    info.adpcm_bytes = 0
    assert call(info) == 0                                             # no samples: nothing to do
    info = _lib.NwInfoC.from_buffer_copy(infos[1])
    assert call(info, rows=None) == ARG and "null pointer" in last_error()                   # the pointers come after the info


def test_null_arguments():
    tot = _lib.NwPcmFilesTotalsC()
    cfg, codec = nc.config_c("rstm16_i8")
    assert L().vga_nw_pcm_files_layout_for(None, 2, C.byref(cfg), codec, None, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_nw_pcm_files_layout_for(None, -1, C.byref(cfg), codec, None, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_nw_pcm_files_create(None, 0, C.byref(cfg), codec, None, None, None) == ARG
    assert L().vga_nw_pcm_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_nw_pcm_files_offsets(None, None, None, None) == ARG
    assert L().vga_nw_pcm_files_stats(None, None) == ARG
    L().vga_nw_pcm_files_destroy(None)
    assert L().vga_nwstm_pcm_write_device_v(None, None, None, None) == ARG
    assert L().vga_nwstm_pcm_read_device_v(None, None, None, None) == ARG
    files = c_files(nc.files_of([(2, 100, 0, 0, 0)]))
    items, count = (_lib.NwPcmFilesItemC * 1)(), C.c_int64()
    assert L().vga_nw_pcm_files_write_items_for(files, 1, C.byref(cfg), codec, None, None, 0, items, 1, C.byref(count)) == ARG and count.value == 2
    old = L().vga_nw_pcm_files_force_general_this_thread(1)
    assert old == 0 and L().vga_nw_pcm_files_force_general_this_thread(0) == 1
    with pytest.raises(_lib.ArgumentError, match="Pcm16Bit or Pcm8Bit"):
        NwPcmFileSet.layout([(2, 100, 0)], nc.RSTM, nwstm.BxstmConfiguration())
    with pytest.raises(_lib.ArgumentError, match="GC-ADPCM"):           # NwFileSet keeps its refusal of a PCM configuration
        nwstm.NwFileSet.layout([(2, 100, 0)], nc.RSTM, nwstm.BxstmConfiguration(Codec=nwstm.NwCodec.Pcm16Bit))


# ---------------------------------------------------------------- the header alone under the sanitizers
INFO_FIELDS = ("target", "endianness", "codec", "channel_count", "sample_count", "interleave_size", "audio_data_offset", "audio_data_length",
               "adpcm_bytes", "looping")
CHECKS = [(kind, moves) for kind in (0, 1, 7) for moves in (1, 0)]


def pack_info(i):
    if i is None:
        return struct.pack("<11i", *([0] * 10 + [1]))
    return struct.pack("<11i", *[getattr(i, k) for k in INFO_FIELDS], 0)


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, first, po_, io_ in cases:
            po_, io_ = list(po_) if po_ is not None else [], list(io_) if io_ is not None else []
            if kind == 0:
                files, cfg, codec = first
                f.write(struct.pack("<6i", 0, len(files), len(po_), len(io_), codec, int(cfg is not None)))
                f.write(struct.pack("<6iIi", *[getattr(cfg, k) for k, _ in cfg._fields_]) if cfg is not None else bytes(32))
                for x in files:
                    f.write(struct.pack("<6i", *[getattr(x, k) for k, _ in x._fields_]))
            elif kind == 1:
                f.write(struct.pack("<6i", 1, len(first), len(po_), len(io_), 0, 0))
                for x in first:
                    f.write(pack_info(x))
            else:
                info, sample_kind, moves = first
                f.write(struct.pack("<6i", 2, 1, 0, 0, 0, 0) + pack_info(info) + struct.pack("<2i", sample_kind, moves))
            f.write(struct.pack("<%dq" % len(po_), *po_))
            f.write(struct.pack("<%dq" % len(io_), *io_))


def read_result(rd, kind):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc or kind == 2:
        return rc, msg, None
    nfiles, nrows = rd.take("2i")
    r = {"first_channel": rd.take("%di" % nfiles), "image_off": rd.take("%dq" % nfiles), "image_size": rd.take("%di" % nfiles),
         "row_off": rd.take("%dq" % nrows), "row_samples": rd.take("%di" % nrows), "totals": rd.take("2q"),
         "tab": [tuple(rd.take("2i3Iq")) for _ in range(nfiles)], "files": rd.take("3i"), "items": []}
    for _ in range(2):
        count = rd.take("i")[0]
        r["items"].append([tuple(rd.take("3iIi2q")) for _ in range(count)])
    return rc, msg, r


def as_tuples(items):
    return [(i.form, i.file, i.x, i.y, i.conv, i.begin, i.end) for i in items]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("nw_pcm_files_host")
    exe = str(tmp / "nw_pcm_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name in CONFIG_NAMES:
        for layout in ("packed", "explicit"):
            files, cfg, codec, po_, io_, _ = the_set(name, layout)
            cases.append((0, (files, cfg, codec), po_, io_))
            names.append(("set", name, layout))
    cfg, codec = nc.config_c("rstm16_i8")
    cases += [(0, ([], cfg, codec), None, None), (0, (nc.files_of(GOOD), None, codec), None, None), (0, (nc.files_of(GOOD), cfg, 2), None, None)]
    names += [("empty", ""), ("null_config", ""), ("codec_2", "")]
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            rcfg, rcodec = refused_config(name)
            cases.append((0, (refused_set(name, position)[0], rcfg, rcodec), None, None))
            names.append(("refused", name, position))
    two = nc.files_of([(2, 100, 0, 0, 0), (2, 100, 0, 0, 0)])
    for k, (po_, io_) in enumerate((([0, 100, 201, 250], None), (None, [0, 24]), (None, [0, 16]), ([0, (1 << 61) + 1, 201, 301], None))):
        cases.append((0, (two, cfg, codec), po_, io_))
        names.append(("offsets", k))
    for name in CONFIG_NAMES + ["mixed"]:
        infos, sizes = the_infos(name)
        rows = nc.explicit_pcm_offsets([[i.sample_count] * i.channel_count for i in infos])
        cases += [(1, infos, None, None), (1, infos, rows, nc.image_offsets_at(sizes, 1))]
        names += [("infos", name, "packed"), ("infos", name, "odd")]
    good = the_infos("rstm16_i8")[0][1]
    cases += [(1, [], None, None), (1, [good, None], None, None)]
    names += [("infos", "empty"), ("infos", "null")]
    for name, (bad, _, _) in sorted(bad_infos().items()):
        cases.append((1, [good, bad], None, None))
        names.append(("infos", "refused", name))
        for sample_kind, moves in CHECKS:
            cases.append((2, (bad, sample_kind, moves), None, None))
            names.append(("check", name, sample_kind, moves))
    for sample_kind, moves in CHECKS:
        cases.append((2, (good, sample_kind, moves), None, None))
        names.append(("check", "good", sample_kind, moves))
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
    for name in CONFIG_NAMES:
        for layout in ("packed", "explicit"):
            files, cfg, codec, po_, io_, sizes = the_set(name, layout)
            cases = nc.CONFIGS[name][5]
            _, (rc, msg, r) = driver[("set", name, layout)]
            assert rc == 0, (name, msg)
            m = nc.model(nc.counts_of(cases), sizes, po_, io_)
            assert r["first_channel"] == m["first_channel"] and r["row_off"] == m["pcm_off"] and r["image_off"] == m["image_off"]
            assert r["image_size"] == sizes and r["totals"] == [m["pcm_samples"], m["image_bytes"]]
            assert r["row_samples"] == [n for per in nc.counts_of(cases) for n in per]
            for general in (0, 1):
                assert r["items"][general] == as_tuples(write_items(name, layout, general)), (name, layout, general)
            for f, (file, tab) in enumerate(zip(files, r["tab"])):     # the table the kernels read, against the per-file layout
                N = per_file_layout(file, cfg, codec)
                conv, vector, input_size, interleave, output_size, audio_at = tab
                assert conv == nc.conv_of(name) and input_size == N.channel_adpcm_bytes and output_size == N.audio_data_size
                assert interleave == min(N.interleave_size, max(N.audio_data_size, 1)) and audio_at == r["image_off"][f] + N.audio_data_offset
                mine = {i[0] for i in r["items"][0] if i[1] == f and i[0] != HEADER_ITEM}
                assert mine <= {VECTOR if vector else GENERAL}
    _, (rc, msg, r) = driver[("empty", "")]
    assert rc == 0 and r["totals"] == [128, 256] and r["items"] == [[], []]
    for name in CONFIG_NAMES + ["mixed"]:
        infos, sizes = the_infos(name)
        for which in ("packed", "odd"):
            (_, _, po_, io_), (rc, msg, r) = driver[("infos", name, which)]
            assert rc == 0, msg
            m = nc.model([[i.sample_count] * i.channel_count for i in infos], sizes, po_, io_)
            assert r["image_off"] == m["image_off"] and r["image_size"] == sizes and r["row_off"] == m["pcm_off"]
            assert r["totals"] == [m["pcm_samples"], m["image_bytes"]]
            for general in (0, 1):
                assert r["items"][general] == as_tuples(NwPcmFileSet.read_items(infos, po_, io_, general)), (name, which, general)
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"] == [128, 256]


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            (_, (files, cfg, codec), _, _), (rc, msg, _) = driver[("refused", name, position)]
            at = refused_set(name, position)[1]
            tot = _lib.NwPcmFilesTotalsC()
            assert L().vga_nw_pcm_files_layout_for(c_files(files), len(files), C.byref(cfg), codec, None, None, None, None, None, C.byref(tot)) == rc
            assert rc == REFUSED[name][3] and msg == last_error() and msg.startswith("file %d: " % at), (name, position, msg)
    for k, (code, word) in enumerate(((ARG, "overlaps"), (ARG, "multiple of 16"), (ARG, "overlaps"), (RANGE, "2^62"))):
        _, (rc, msg, _) = driver[("offsets", k)]
        assert rc == code and msg.startswith("file ") and word in msg, (k, rc, msg)
    _, (rc, msg, _) = driver[("null_config", "")]
    assert rc == ARG and "configuration" in msg
    _, (rc, msg, _) = driver[("codec_2", "")]
    assert rc == ARG and "codec 2" in msg
    for name, (_, code, _) in bad_infos().items():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == code and msg.startswith("file 1: "), (name, rc, msg)
    _, (rc, msg, _) = driver[("infos", "null")]
    assert rc == ARG and msg == "file 1: null info"


def test_the_moved_read_info_check_is_the_per_file_calls(driver):
    """nw::pcm_read_info_check on its own gives, for every info and every (sample kind, files or none), the code and the message
    of vga_nwstm_pcm_read_device up to its first look at a pointer"""
    good = the_infos("rstm16_i8")[0][1]
    seen = set()
    for name, info in [("good", good)] + [(k, v[0]) for k, v in bad_infos().items()]:
        for sample_kind, moves in CHECKS:
            _, (rc, msg, _) = driver[("check", name, sample_kind, moves)]
            got = L().vga_nwstm_pcm_read_device(C.byref(info), None, 1 << 40, 1 if moves else 0, None, sample_kind, 1 << 40, None)
            if rc:
                assert got == rc and last_error() == msg, (name, sample_kind, moves, msg)
                seen.add(msg)
            elif moves and info.adpcm_bytes:                           # past the info: the call goes on to its pointers
                assert got == ARG and "null pointer" in last_error(), (name, sample_kind, moves)
            else:
                assert got == 0
    assert len(seen) == 4, seen
