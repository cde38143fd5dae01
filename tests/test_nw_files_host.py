"""include/vgaudio_hip/nw_files.h without a GPU: the header's functions are exported and in the ctypes table with the header's
argument counts, vga_nw_files_layout_for (host code) against a model built from the per-file vga_nwstm_layout_for
(tests/nw_files_cases.py) and against vga_gc_aligned_layout_for fed with vga_nw_files_gc_files' files, the work tables, every
refusal with its file and the per-file call's code and message, that the GPU file's table of cases names every function the
header declares, the moved nw_layout (vgaudio_amd/csrc/nw_host.hpp) struct for struct against the library, and the HIP-free
host layer (vgaudio_amd/csrc/nw_files_host.hpp) on its own under AddressSanitizer and UBSan."""
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

import nw_files_cases as nf
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.nwstm import NwFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "nw_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_nw_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "nw_files_host_driver.cpp")

NAMES = ["vga_nw_files_layout_for", "vga_nw_files_create", "vga_nw_files_create_from_infos", "vga_nw_files_destroy",
         "vga_nw_files_totals_of", "vga_nw_files_offsets", "vga_nw_files_gc_files", "vga_nw_files_ragged", "vga_nwstm_write_device_v",
         "vga_nwstm_read_device_v"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4


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
    for name in ("vga_nwstm_write_device_v", "vga_nwstm_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("name", sorted(nf.CONFIGS))
def test_layout_is_the_per_file_calls_packed(name):
    cfg, tuples = nf.CONFIGS[name]
    files = nf.files_of(tuples)
    fc, so, io, tot = NwFileSet.layout(files, configuration=cfg)
    m = nf.model(files, cfg)
    nch = sum(f.channels for f in files)
    assert (tot.files, tot.channels) == (len(files), nch) and len(so) == nch
    assert list(fc) == m["first_channel"] and list(so) == m["seek_off"] and list(io) == m["image_off"]
    assert (tot.pcm_samples, tot.adpcm_bytes, tot.seek_shorts, tot.image_bytes) == (m["pcm_samples"], m["adpcm_bytes"], m["seek_shorts"], m["image_bytes"])
    # every NW image size is a multiple of 0x20: the rounding of the offsets to 16 is a no-op today
    assert all(s % 0x20 == 0 for s in m["image_size"]) and all(o % 16 == 0 for o in io)
    assert tot.image_bytes == io[-1] + m["image_size"][-1] + 256
    # outputs one at a time
    arr, i64p = (_lib.NwFileC * len(files))(*files), C.POINTER(C.c_int64)
    f = L().vga_nw_files_layout_for
    only, one = _lib.NwFilesTotalsC(), np.zeros(nch, np.int64)
    assert f(arr, len(files), C.byref(cfg), None, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), C.byref(cfg), None, one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, so)
    assert f(arr, len(files), C.byref(cfg), None, None, None, None) == ARG
    assert f(arr, len(files), None, None, None, None, C.byref(only)) == ARG


def test_the_cases_reach_what_they_are_for():
    lay = {n: nf.model(nf.files_of(t), c)["layouts"] for n, (c, t) in nf.CONFIGS.items()}
    a = lay["rstm"]                                                   # alignment 14
    assert (a[3].alignment_needed, a[3].channel_sample_count) == (1, 70)
    assert (a[5].alignment_needed, a[5].channel_sample_count, a[5].sample_count) == (0, 100, 57)
    assert a[5].channel_adpcm_bytes > nf.byte_count(a[5].sample_count) and a[5].channel_seek_entries != a[5].seek_table_entry_count
    assert lay["rstm-short"][7].channel_sample_count == 114           # alignment 64
    assert any(x.seek_table_entry_count > x.channel_seek_entries for x in lay["rstm-short"])          # zero fill past the source entries
    assert a[6].track_count == 128 and a[8].audio_data_size == 0
    assert {x.interleave_size for x in a} == {8} and {x.interleave_size for x in lay["rstm-short"]} == {16}
    d = lay["rstm-default"]
    assert (d[0].interleave_count, d[0].interleave_size, d[0].last_block_size_without_padding, d[0].last_block_size) == (3, 0x2000, 4, 0x20)
    assert d[1].alignment_needed and d[1].channel_sample_count == 30000 + 14335
    flags = {(x[0].include_track_info, x[0].include_region_info, x[0].include_unaligned_loop) for n, x in lay.items() if n[0] in "cf"}
    assert flags == {(1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 1, 1)}                # every combination the writers produce


@pytest.mark.parametrize("name", sorted(nf.CONFIGS))
def test_the_sets_inputs_are_the_aligned_sets_outputs(name):
    cfg, tuples = nf.CONFIGS[name]
    files = nf.files_of(tuples)
    m = nf.model(files, cfg)
    gc = [_lib.GcFileC(f.channels, f.sample_rate, lay.channel) for f, lay in zip(files, m["layouts"])]
    fc, so, tot = AlignedFileSet.layout(gc)
    _, nso, _, ntot = NwFileSet.layout(files, configuration=cfg)
    assert list(fc) == m["first_channel"] and list(so) == list(nso)
    assert (tot.out_adpcm_bytes, tot.out_pcm_samples, tot.seek_shorts) == (ntot.adpcm_bytes, ntot.pcm_samples, ntot.seek_shorts)
    gm = nf.ga.model(gc)                                               # gc_aligned_cases' model: the output batch's rows
    assert gm["out_adpcm_off"] == m["adpcm_off"] and gm["seek_off"] == m["seek_off"]


def test_an_empty_set_needs_no_gpu():
    fc, so, io, tot = NwFileSet.layout([], configuration=nf.config(nf.RSTM))
    assert len(fc) == len(so) == len(io) == 0
    assert (tot.files, tot.channels, tot.pcm_samples, tot.adpcm_bytes, tot.seek_shorts, tot.image_bytes) == (0, 0, 128, 256, 0, 256)
    s = NwFileSet([], configuration=nf.config(nf.FSTM))
    assert s.files == s.channels == 0 and s.gc_files() == []
    assert L().vga_nwstm_write_device_v(s._h, None, None, None, None, None, None, None, None) == 0
    assert L().vga_nwstm_read_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert s.images(np.zeros(256, np.uint8)) == []
    s.close()
    r = NwFileSet.from_infos([])
    assert r.files == 0 and L().vga_nwstm_read_device_v(r._h, None, None, None, None, None, None, None) == 0
    assert L().vga_nwstm_write_device_v(r._h, None, None, None, None, None, None, None, None) == 0
    r.close()


def test_a_file_of_no_samples_is_a_good_file():
    """vga_nwstm_write_device writes one (headers, an empty table, an empty DATA block), so the set takes it"""
    rc, lay = nf.file_layout(nf.nw_file(2, 0), nf.config(nf.RSTM))
    assert rc == 0 and lay.audio_data_size == 0 and lay.file_size % 0x20 == 0


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code and message
REFUSED = {                                                            # name -> (the file, the configuration, the code)
    "channels0": ((0, 50, 0, 0, 0), nf.config(nf.RSTM), ARG),
    "channels256": ((256, 50, 0, 0, 0), nf.config(nf.RSTM), ARG),
    "negative": ((1, -1, 0, 0, 0), nf.config(nf.CSTM), RANGE),
    "inverted": ((2, 50, 1, 30, 20), nf.config(nf.FSTM), RANGE),
    "loop_past_end": ((2, 50, 1, 10, 51), nf.config(nf.RSTM), RANGE),
    "interleave15": ((2, 50, 0, 0, 0), nf.config(nf.RSTM, 15), RANGE),
    "seek_entry1": ((2, 50, 0, 0, 0), nf.config(nf.RSTM, 14, 1), RANGE),
    "alignment_negative": ((2, 50, 0, 0, 0), nf.config(nf.CSTM, 14, 14, -1), RANGE),
    "target3": ((2, 50, 0, 0, 0), nf.config(3), ARG),
    "track_type": ((2, 50, 0, 0, 0), nf.config(nf.RSTM, track=2), ARG),
    "seek_type": ((2, 50, 0, 0, 0), nf.config(nf.RSTM, seek=2), ARG),
    "version": ((2, 50, 0, 0, 0), nf.config(nf.CSTM, version=nf.V(2, 4)), RANGE),
    "too_large": ((255, 20_000_000, 0, 0, 0), nf.config(nf.RSTM), RANGE),
    "aligned_overflow": ((1, 0x7FFFFFF0, 1, 1, 0x7FFFFFF0), nf.config(nf.RSTM), RANGE),
}
# the configuration is the set's: the first file meets what it refuses
OF_THE_SET = {"interleave15", "seek_entry1", "alignment_negative", "target3", "track_type", "seek_type", "version"}
GOOD = [(1, 1, 0, 0, 0), (2, 28, 0, 0, 0), (2, 100, 1, 14, 57)]


def refused_set(name, position):
    bad = nf.nw_file(*REFUSED[name][0])
    good = nf.files_of(GOOD)
    at = {"first": 0, "middle": 2, "last": len(good)}[position]
    return good[:at] + [bad] + good[at:], 0 if name in OF_THE_SET else at


@pytest.mark.parametrize("position", ["first", "middle", "last"])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file_with_the_per_file_code_and_message(name, position):
    _, cfg, code = REFUSED[name]
    files, at = refused_set(name, position)
    rc, _ = nf.file_layout(files[at], cfg)
    per_file = last_error()
    assert rc == code and per_file
    arr, tot, out = (_lib.NwFileC * len(files))(*files), _lib.NwFilesTotalsC(), C.c_void_p()
    assert L().vga_nw_files_layout_for(arr, len(files), C.byref(cfg), None, None, None, C.byref(tot)) == code
    assert last_error() == "file %d: %s" % (at, per_file)
    assert L().vga_nw_files_create(arr, len(files), C.byref(cfg), C.byref(out)) == code and not out.value
    assert last_error() == "file %d: %s" % (at, per_file)
    with pytest.raises(_lib._EXC[code], match=r"file %d\b" % at):
        NwFileSet.layout(files, configuration=cfg)


def good_info(nch=2, samples=100, il=8, audio_offset=0x100):
    i = _lib.NwInfoC()
    i.channel_count, i.sample_count, i.interleave_size, i.audio_data_offset = nch, samples, il, audio_offset
    i.adpcm_bytes = nf.byte_count(samples)
    i.audio_data_length = nf.up(i.adpcm_bytes, 0x20) * nch
    i.sample_rate = nf.RATE
    return i


def bad_infos():
    out = {}
    for name, (field, value, code) in {"interleave0": ("interleave_size", 0, ARG), "channels0": ("channel_count", 0, ARG),
                                       "length": ("audio_data_length", 0x41, ARG), "bytes": ("adpcm_bytes", 5, ARG),
                                       "odd_offset": ("audio_data_offset", 0x101, OP), "odd_interleave": ("interleave_size", 12, OP)}.items():
        i = good_info()
        setattr(i, field, value)
        out[name] = (i, code)
    return out


def test_infos_the_per_file_reader_refuses_are_refused_with_their_file():
    for name, (bad, code) in bad_infos().items():
        if name in ("interleave0", "channels0", "length"):
            assert L().vga_nwstm_read_device(C.byref(bad), None, 0, 1, None, 0, None) == ARG, name
        with pytest.raises(_lib._EXC[code], match=r"file 2\b"):
            NwFileSet.from_infos([good_info(), good_info(1, 5), bad, good_info()])
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        NwFileSet.from_infos([good_info(), good_info()], image_offsets=[0, 1004])      # not a multiple of 8
    out = C.c_void_p()
    assert L().vga_nw_files_create_from_infos(None, 2, None, C.byref(out)) == ARG and not out.value
    assert L().vga_nw_files_create_from_infos(None, 0, None, None) == ARG


def test_null_arguments():
    tot, cfg = _lib.NwFilesTotalsC(), nf.config(nf.RSTM)
    assert L().vga_nw_files_layout_for(None, 2, C.byref(cfg), None, None, None, C.byref(tot)) == ARG
    assert L().vga_nw_files_layout_for(None, -1, C.byref(cfg), None, None, None, C.byref(tot)) == ARG
    assert L().vga_nw_files_create(None, 0, C.byref(cfg), None) == ARG
    assert L().vga_nw_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_nw_files_offsets(None, None, None, None) == ARG
    assert L().vga_nw_files_gc_files(None, None) == ARG
    assert not L().vga_nw_files_ragged(None)
    L().vga_nw_files_destroy(None)
    assert L().vga_nwstm_write_device_v(None, None, None, None, None, None, None, None, None) == ARG
    assert L().vga_nwstm_read_device_v(None, None, None, None, None, None, None, None) == ARG


# ---------------------------------------------------------------- the headers alone under the sanitizers
def layout_grid():
    """params x channel counts for the moved nw_layout: targets x versions x channel counts x loops, and the refused ones"""
    loops = [(100, 0, 0, 0), (100, 1, 15, 57), (100, 1, 14, 57), (100, 1, 50, 100), (0, 0, 0, 0), (30000, 1, 1, 30000)]
    versions = {nf.RSTM: [0], nf.CSTM: [0, nf.V(2, 0), nf.V(2, 1), nf.V(2, 2), nf.V(2, 3)], nf.FSTM: [0, nf.V(0, 2), nf.V(0, 3), nf.V(0, 4), nf.V(0, 5)]}
    grid = []
    for target, vs in versions.items():
        for v in vs:
            for nch in (1, 2, 3, 255):
                for k, (n, looping, ls, le) in enumerate(loops):
                    for spi, spe, align, short in ((14, 14, 14, 0), (28, 5, 64, 1), (0, 0, 0, 0)):
                        cfg = nf.config(target, spi, spe, align, short, short, v, -1 if k % 2 else k // 2 % 2)
                        grid.append((nf.params_of(nf.nw_file(nch, n, looping, ls, le), cfg), nch))
    for name in sorted(REFUSED):
        t, cfg, _ = REFUSED[name]
        grid.append((nf.params_of(nf.nw_file(*t), cfg), t[0]))
    keep = nf.params_of(nf.nw_file(2, 50), nf.config(nf.RSTM))
    keep.keep_seek_table = 1
    tracks = nf.params_of(nf.nw_file(2, 50), nf.config(nf.RSTM))
    tracks.track_count = 256
    return grid + [(keep, 2), (tracks, 2)]


def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, files, extra in cases:
            if kind == 0:
                c = extra
                f.write(struct.pack("<2i6iIi", 0, len(files), c.target, c.samples_per_interleave, c.samples_per_seek_table_entry,
                                    c.loop_point_alignment, c.track_type, c.seek_table_type, c.version, c.endianness))
                for x in files:
                    f.write(struct.pack("<6i", x.channels, x.sample_rate, x.sample_count, x.looping, x.loop_start, x.loop_end))
            elif kind == 1:
                f.write(struct.pack("<3i", 1, len(files), int(extra is not None)))
                for i in files:
                    f.write(struct.pack("<8i", i.channel_count, i.sample_count, i.adpcm_bytes, i.interleave_size, i.audio_data_offset,
                                        i.audio_data_length, i.sample_rate, i.looping))
                if extra is not None:
                    f.write(struct.pack("<%dq" % len(files), *extra))
            else:
                f.write(struct.pack("<2i", 2, extra) + bytes(files))


def read_result(rd, kind):
    rc, n = rd.take("2i")
    msg = rd.d[rd.at:rd.at + n].decode()
    rd.at += n
    if rc:
        return rc, msg, None
    if kind == 2:
        size = C.sizeof(_lib.NwLayoutC)
        raw = rd.d[rd.at:rd.at + size]
        rd.at += size
        return rc, msg, raw
    nfiles, nch = rd.take("2i")
    r = {"first_channel": rd.take("%di" % nfiles), "image_off": rd.take("%dq" % nfiles), "image_size": rd.take("%di" % nfiles),
         "counts": rd.take("%di" % nch), "adpcm_off": rd.take("%dq" % nch), "seek_off": rd.take("%dq" % nch),
         "entries": rd.take("%di" % nch), "file": rd.take("%di" % nch), "totals": rd.take("4q")}
    r["tab"] = [rd.take("4I8i") for _ in range(nfiles)]
    na = rd.take("i")[0]
    r["audio"] = [tuple(rd.take("iI")) for _ in range(na)]
    ns = rd.take("i")[0]
    r["seek"] = [tuple(rd.take("iI")) for _ in range(ns)]
    return rc, msg, r


def the_infos():
    infos = [good_info(1, 1), good_info(2, 100, 8), good_info(2, 100, 16, 0x120), good_info(3, 5000, 0x2000), good_info(1, 30000 + 14335, 0x2000),
             good_info(2, 0, 8), good_info(255, 15, 8, 0x3000), good_info(2, 2 * 14336 + 5, 0x2000)]
    sizes = [i.audio_data_offset + i.audio_data_length for i in infos]
    odd, at = [], 8
    for sz in sizes:                                                   # bases 8 mod 16
        odd.append(at)
        at = nf.up(at + sz, 16) + 8
    return infos, sizes, odd


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("nw_files_host")
    exe = str(tmp / "nw_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name, (cfg, tuples) in sorted(nf.CONFIGS.items()):
        cases.append((0, nf.files_of(tuples), cfg))
        names.append(("set", name))
    cases.append((0, [], nf.config(nf.RSTM)))
    names.append(("empty", ""))
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            cases.append((0, refused_set(name, position)[0], REFUSED[name][1]))
            names.append(("refused", name, position))
    infos, sizes, odd = the_infos()
    cases += [(1, infos, None), (1, infos, odd), (1, [], None)]
    names += [("infos", "packed"), ("infos", "odd"), ("infos", "empty")]
    for name, (bad, _) in sorted(bad_infos().items()):
        cases.append((1, [good_info(), bad], None))
        names.append(("infos", "refused", name))
    for k, (p, nch) in enumerate(layout_grid()):
        cases.append((2, p, nch))
        names.append(("layout", k))
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


def test_moved_nw_layout_is_the_librarys_struct_for_struct(driver):
    refused = 0
    for k, (p, nch) in enumerate(layout_grid()):
        _, (rc, msg, raw) = driver[("layout", k)]
        lay = _lib.NwLayoutC()
        want = L().vga_nwstm_layout_for(C.byref(p), nch, C.byref(lay))
        assert rc == want, (k, rc, want, msg)
        if rc:
            assert msg == last_error() and msg, k
            refused += 1
        else:
            assert raw == bytes(lay), k
    assert refused >= len(REFUSED) + 2


def test_host_layer_layout_is_the_model(driver):
    for name, (cfg, tuples) in nf.CONFIGS.items():
        (_, files, _), (rc, msg, r) = driver[("set", name)]
        assert rc == 0, (name, msg)
        m = nf.model(files, cfg)
        for k in ("first_channel", "counts", "adpcm_off", "seek_off", "entries", "image_off", "image_size"):
            assert r[k] == m[k], (name, k)
        assert r["file"] == [i for i, f in enumerate(files) for _ in range(f.channels)]
        assert r["totals"] == [m["pcm_samples"], m["adpcm_bytes"], m["seek_shorts"], m["image_bytes"]]
        for t, lay, f in zip(r["tab"], m["layouts"], files):
            assert t[:3] == [lay.channel_adpcm_bytes, lay.interleave_size, lay.audio_data_size]
            assert t[4:] == [lay.audio_data_offset, lay.channel_seek_entries, lay.seek_table_entry_count, (lay.seek_block_size - 8) // 2,
                             int(cfg.target == nf.RSTM), lay.seek_block_offset, lay.file_size, f.channels]
    _, (rc, msg, r) = driver[("empty", "")]
    assert rc == 0 and r["totals"] == [128, 256, 0, 256] and not r["audio"] and not r["seek"]


def test_writer_work_tables_cover_every_image_byte_once(driver):
    """the header kernel's region, the seek items and the audio items tile every image; no item lies outside an image"""
    seen16 = seen8 = several = 0
    for name, (cfg, tuples) in nf.CONFIGS.items():
        (_, files, _), (rc, msg, r) = driver[("set", name)]
        m = nf.model(files, cfg)
        audio, seek = {}, {}
        for x, y in r["audio"]:
            audio.setdefault(x, []).append(y)
        for x, y in r["seek"]:
            seek.setdefault(x, []).append(y)
        for f, lay in enumerate(m["layouts"]):
            t = r["tab"][f]
            geom = (t[0], t[1], t[2], files[f].channels)
            # the header kernel: everything in front of the seek body, and the DATA block's header up to the audio
            ranges = [(0, lay.seek_block_offset + 8), (lay.data_block_offset, lay.audio_data_offset)]
            body = lay.seek_block_offset + 8
            for y in seek.pop(f, []):
                assert y % nf.CHUNK == 0 and y < t[7], "a seek item outside its block"
                ranges.append((body + 2 * y, body + 2 * min(y + nf.CHUNK, t[7])))
            assert body + 2 * t[7] == lay.data_block_offset
            total = lay.audio_data_size * files[f].channels
            full = 16 if t[1] % 16 == 0 else 8
            for y in audio.pop(f, []):
                start, end, gran = nf.audio_item_range(geom, y)
                assert start < total and end <= total, "an item outside its image"
                assert gran == full and start % gran == 0 and end % gran == 0 and t[1] % gran == 0
                assert (lay.audio_data_offset + start) % gran == 0 and m["image_off"][f] % 16 == 0
                ranges.append((lay.audio_data_offset + start, lay.audio_data_offset + end))
                seen16 += gran == 16
                seen8 += gran == 8
            several += sum(1 for a, b in ranges if a >= lay.audio_data_offset) > 1
            check_tiling(ranges, lay.file_size, (name, f))
            assert lay.audio_data_offset + total == lay.file_size
        assert not audio and not seek
    assert seen16 and seen8 and several, "the cases do not reach every granule choice and a file of several items"


def test_reader_work_table_covers_every_row_byte_once(driver):
    infos, sizes, odd = the_infos()
    for which in ("packed", "odd"):
        (_, _, offs), (rc, msg, r) = driver[("infos", which)]
        assert rc == 0, msg
        want_off, at = [], 0
        for sz in sizes:
            want_off.append(at)
            at = nf.up(at + sz, 16)
        assert r["image_off"] == (want_off if offs is None else offs) and r["image_size"] == sizes
        assert r["totals"][3] == max(nf.up(o + s, 16) for o, s in zip(r["image_off"], sizes)) + 256 and r["totals"][2] == 0
        assert r["counts"] == [i.sample_count for i in infos for _ in range(i.channel_count)]
        per_channel = {}
        for x, y in r["audio"]:
            per_channel.setdefault(x, []).append(y)
        for f, i in enumerate(infos):
            inp = i.audio_data_length // i.channel_count
            assert r["tab"][f][:3] == [inp, i.interleave_size, i.adpcm_bytes] and r["tab"][f][4] == i.audio_data_offset
            allowed = (r["image_off"][f] + i.audio_data_offset) % 16 == 0 and i.interleave_size % 16 == 0 and inp % 16 == 0
            assert r["tab"][f][3] == int(allowed), (which, f)
            for c in range(r["first_channel"][f], r["first_channel"][f] + i.channel_count):
                ranges = []
                for y in per_channel.pop(c, []):
                    start, stop, gran = nf.reader_item_range(i.adpcm_bytes, y)
                    assert gran == (16 if allowed else 8) and start < i.adpcm_bytes and start % gran == 0
                    ranges.append((start, stop))
                if i.adpcm_bytes:
                    check_tiling(ranges, i.adpcm_bytes, (which, f, c))
                else:
                    assert not ranges
        assert not per_channel
    assert not any(t[3] for t in driver[("infos", "odd")][1][2]["tab"])
    assert any(t[3] for t in driver[("infos", "packed")][1][2]["tab"]) and not all(t[3] for t in driver[("infos", "packed")][1][2]["tab"])
    _, (rc, msg, r) = driver[("infos", "empty")]
    assert rc == 0 and r["totals"][3] == 256 and not r["audio"]


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        for position in ("first", "middle", "last"):
            (_, files, cfg), (rc, msg, _) = driver[("refused", name, position)]
            at = refused_set(name, position)[1]
            assert nf.file_layout(files[at], cfg)[0] == rc == REFUSED[name][2]
            assert msg == "file %d: %s" % (at, last_error()), (name, position, msg)
    for name, (_, code) in bad_infos().items():
        _, (rc, msg, _) = driver[("infos", "refused", name)]
        assert rc == code and re.search(r"file 1\b", msg), (name, rc, msg)
