"""include/vgaudio_hip/gc_files.h without a GPU: the header's functions are exported and in the ctypes table with the header's
argument counts (the header lies outside the directory listing tests/test_abi_exports.py reads), vga_gc_files_layout_for
(host code) against a model built from the per-file size calls (tests/gc_files_cases.py), the audio work tables, every
refusal with its file and its code, that the GPU file's table of cases names every function the header declares, and the
HIP-free host layer (vgaudio_amd/csrc/gc_files_host.hpp) on its own under AddressSanitizer and UBSan."""
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

import gc_files_cases as gf
from vgaudio_amd import _lib
from vgaudio_amd.dsp import DspFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "gc_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_gc_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "gc_files_host_driver.cpp")

NAMES = ["vga_gc_files_layout_for", "vga_gc_files_create", "vga_gc_files_create_from_dsp", "vga_gc_files_destroy",
         "vga_gc_files_totals_of", "vga_gc_files_offsets", "vga_gc_files_ragged", "vga_gcadpcm_build_channels_device_v",
         "vga_dsp_write_device_v", "vga_dsp_read_device_v"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4


def _strip(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//.*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    return re.sub(r"\btypedef\b[^;{]*;", "", text)


def _declared(path):
    """{function: argument count} (the regexes of tests/test_abi_exports.py)"""
    out = {}
    for name, args in re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{()]*)\)\s*;", _strip(open(path).read())):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def L():
    return _lib.lib()


def the_files():
    return [gf.gc_file(*f) for f in gf.FILES]


def all_configs():
    return [(name, trim, gf.config(spi, align, trim)) for name, (spi, align) in sorted(gf.CONFIGS.items()) for trim in (1, 0)]


BIG = [(2, 5_000_000, 1, 28, 4_000_000, 14), (1, 3_000_001, 0, 0, 0, 0x3800), (3, 70_001, 1, 14, 70_000, 1), (2, 14 * 4096, 0, 0, 0, 0)]


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
    for f in sorted(os.listdir(inc)):
        if f.endswith(".h"):
            assert not [n for n in NAMES if n in _declared(os.path.join(inc, f))], f


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    for name in ("vga_gcadpcm_build_channels_device_v", "vga_dsp_write_device_v", "vga_dsp_read_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_chain_on_a_busy_stream"} <= set(cases[name])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("which", ["none"] + ["%s-%d" % (n, t) for n, t, _ in all_configs()])
def test_layout_is_the_per_file_calls_packed(which):
    cfg = None if which == "none" else next(c for n, t, c in all_configs() if "%s-%d" % (n, t) == which)
    files = the_files()
    fc, so, io, tot = DspFileSet.layout(files, cfg)
    m = gf.model(files, cfg)
    nch = sum(f.channels for f in files)
    assert (tot.files, tot.channels) == (len(files), nch) and len(so) == nch
    assert list(fc) == m["first_channel"] and list(so) == m["seek_off"]
    assert (tot.pcm_samples, tot.adpcm_bytes, tot.seek_shorts, tot.image_bytes, tot.build_workspace_bytes) == \
        (m["pcm_samples"], m["adpcm_bytes"], m["seek_shorts"], m["image_bytes"], m["workspace"])
    assert all(o % 8 == 0 for o in so)
    for c in range(nch - 1):                                           # a channel without entries takes no room
        if m["entries"][c] == 0:
            assert so[c] == so[c + 1]
    assert any(e == 0 for e in m["entries"]) and any(n == 0 for n in m["counts"])
    if cfg is not None:
        assert list(io) == m["image_off"] and all(o % 16 == 0 for o in io)
        assert m["image_size"][0] == 98                                 # a mono image of 1 sample: images are not naturally aligned
        assert any(s % 16 for s in m["image_size"]), "no image that ends off a 16-byte boundary"
        assert tot.image_bytes == gf.up(io[-1] + m["image_size"][-1], 16) + 256
    # outputs one at a time
    arr, i64p = (_lib.GcFileC * len(files))(*files), C.POINTER(C.c_int64)
    f = L().vga_gc_files_layout_for
    pc = C.byref(cfg) if cfg is not None else None
    only, one = _lib.GcFilesTotalsC(), np.zeros(nch, np.int64)
    assert f(arr, len(files), pc, None, None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), pc, None, one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, so)
    assert f(arr, len(files), pc, None, None, None, None) == ARG


def test_alignment_shifts_header_numbers_only():
    files = the_files()
    a, b = gf.model(files, gf.config(0x3800, 1, 0)), gf.model(files, gf.config(0x3800, 4, 0))
    assert a["pcm_off"] == b["pcm_off"] and a["adpcm_off"] == b["adpcm_off"] and a["seek_off"] == b["seek_off"]
    assert any(x["layout"].loop_start != y["layout"].loop_start for x, y in zip(a["geom"], b["geom"]))


def test_an_empty_set_needs_no_gpu():
    fc, so, io, tot = DspFileSet.layout([], gf.config(14, 1, 1))
    assert len(fc) == len(so) == len(io) == 0
    assert (tot.files, tot.channels, tot.pcm_samples, tot.adpcm_bytes, tot.seek_shorts, tot.image_bytes, tot.build_workspace_bytes) == \
        (0, 0, 128, 256, 0, 256, 0)
    assert DspFileSet.layout([], None)[3].image_bytes == 0
    s = DspFileSet([], gf.config(14, 1, 1))
    assert s.files == s.channels == 0
    assert L().vga_gcadpcm_build_channels_device_v(s._h, None, None, None, None, None, None, None, 0, None) == 0
    assert L().vga_dsp_write_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert L().vga_dsp_read_device_v(s._h, None, None, None, None, None, None, None) == 0
    assert s.split_images(np.zeros(256, np.uint8)) == []
    s.close()
    r = DspFileSet.from_infos([])
    assert r.files == 0 and L().vga_dsp_read_device_v(r._h, None, None, None, None, None, None, None) == 0
    r.close()


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code
def per_file_codes():
    """what the per-file calls answer to the same mistakes"""
    lay, d = _lib.GcChannelLayoutC(), _lib.DspLayoutC()
    neg, inv = _lib.GcChannelParamsC(-1, 0, 0, 0, 0, 14), _lib.GcChannelParamsC(50, 1, 30, 20, 0, 14)
    p15 = _lib.DspParamsC(gf.RATE, 50, 0, 0, 0, 15, 1, 1)
    p0 = _lib.DspParamsC(gf.RATE, 50, 0, 0, 0, 14, 1, 1)
    info = _lib.DspInfoC()
    info.channel_count, info.sample_count, info.adpcm_bytes, info.interleave_size, info.data_length = 2, 28, 16, 0, 32
    return {"negative": L().vga_gcadpcm_channel_layout_for(C.byref(neg), C.byref(lay)),
            "inverted": L().vga_gcadpcm_channel_layout_for(C.byref(inv), C.byref(lay)),
            "interleave15": L().vga_dsp_layout_for(C.byref(p15), 2, C.byref(d)),
            "channels0": L().vga_dsp_layout_for(C.byref(p0), 0, C.byref(d)),
            "info": L().vga_dsp_read_device(C.byref(info), None, 0, 1, None, 0, None)}


NAMED = {"interleave15": 0}                                            # the configuration is the set's: the first file meets it
REFUSED = {                                                            # name -> (the file (put at index 3), the configuration, the code)
    "alignment": ((2, 100, 1, 15, 57, 14, 4), (14, 1, 1), OP),
    "channels0": ((0, 50, 0, 0, 0, 14), (14, 1, 1), ARG),
    "channels256": ((256, 50, 0, 0, 0, 14), (14, 1, 1), OP),
    "negative": ((1, -1, 0, 0, 0, 14), (14, 1, 1), RANGE),
    "inverted": ((2, 50, 1, 30, 20, 14), (14, 1, 1), RANGE),
    "interleave15": ((2, 50, 0, 0, 0, 14), (15, 1, 1), RANGE),
    "mono_past_row": ((1, 10, 1, 0, 20, 14), (14, 1, 1), ARG),
}


def test_per_file_codes_are_the_ones_the_table_states():
    codes = per_file_codes()
    assert codes == {"negative": RANGE, "inverted": RANGE, "interleave15": RANGE, "channels0": ARG, "info": ARG}
    assert all(REFUSED[k][2] == codes[k] for k in codes if k in REFUSED)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file(name):
    bad, (spi, align, trim), code = REFUSED[name]
    files = the_files()[:3] + [gf.gc_file(*bad)] + the_files()[3:5]
    cfg = gf.config(spi, align, trim)
    for call in ("layout", "create"):
        with pytest.raises(_lib._EXC[code], match=r"file %d\b" % NAMED.get(name, 3)):
            DspFileSet.layout(files, cfg) if call == "layout" else DspFileSet(files, cfg)
    arr, tot, out = (_lib.GcFileC * len(files))(*files), _lib.GcFilesTotalsC(), C.c_void_p()
    assert L().vga_gc_files_layout_for(arr, len(files), C.byref(cfg), None, None, None, C.byref(tot)) == code
    assert L().vga_gc_files_create(arr, len(files), C.byref(cfg), C.byref(out)) == code and not out.value
    if name in ("interleave15", "mono_past_row"):                      # without a configuration the same files are a good set
        assert L().vga_gc_files_layout_for(arr, len(files), None, None, None, None, C.byref(tot)) == 0


def good_info(nch=2, samples=100, fpi=1):
    i = _lib.DspInfoC()
    i.channel_count, i.sample_count, i.frames_per_interleave = nch, samples, fpi
    i.nibble_count = L().vga_gcadpcm_sample_count_to_nibble_count(samples)
    i.audio_offset, i.adpcm_bytes = 0x60 * nch, gf.byte_count(samples)
    i.interleave_size = 0 if nch == 1 else fpi * 8
    i.data_length = i.adpcm_bytes if nch == 1 else gf.up(i.adpcm_bytes, 8) * nch
    return i


def test_infos_the_per_file_reader_refuses_are_refused_with_their_file():
    bad = good_info()
    bad.interleave_size = 0
    assert L().vga_dsp_read_device(C.byref(bad), None, 0, 1, None, 0, None) == ARG
    with pytest.raises(_lib.ArgumentError, match=r"file 2\b"):
        DspFileSet.from_infos([good_info(), good_info(1, 5), bad, good_info()])
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        DspFileSet.from_infos([good_info(), good_info()], image_offsets=[0, 1004])      # not a multiple of 8
    out = C.c_void_p()
    assert L().vga_gc_files_create_from_dsp(None, 2, None, C.byref(out)) == ARG and not out.value
    assert L().vga_gc_files_create_from_dsp(None, 0, None, None) == ARG


def test_null_arguments():
    tot = _lib.GcFilesTotalsC()
    assert L().vga_gc_files_layout_for(None, 2, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_gc_files_layout_for(None, -1, None, None, None, None, C.byref(tot)) == ARG
    assert L().vga_gc_files_create(None, 0, None, None) == ARG
    assert L().vga_gc_files_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_gc_files_offsets(None, None, None, None) == ARG
    assert not L().vga_gc_files_ragged(None)
    L().vga_gc_files_destroy(None)
    assert L().vga_gcadpcm_build_channels_device_v(None, None, None, None, None, None, None, None, 0, None) == ARG
    assert L().vga_dsp_write_device_v(None, None, None, None, None, None, None, None) == ARG
    assert L().vga_dsp_read_device_v(None, None, None, None, None, None, None, None) == ARG


# ---------------------------------------------------------------- the header alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for kind, files, extra in cases:
            if kind == 0:
                cfg = extra
                f.write(struct.pack("<6i", 0, len(files), int(cfg is not None), *((cfg.samples_per_interleave, cfg.loop_point_alignment,
                                                                                   cfg.trim_file) if cfg is not None else (0, 0, 0))))
                for x in files:
                    ch = x.channel
                    f.write(struct.pack("<8i", x.channels, x.sample_rate, ch.sample_count, ch.looping, ch.loop_start, ch.loop_end,
                                        ch.loop_alignment_multiple, ch.samples_per_seek_table_entry))
            else:
                f.write(struct.pack("<3i", 1, len(files), int(extra is not None)))
                for i in files:
                    f.write(struct.pack("<10i", i.channel_count, i.sample_count, i.nibble_count, i.frames_per_interleave, i.audio_offset,
                                        i.adpcm_bytes, i.interleave_size, i.data_length, i.looping, i.sample_rate))
                if extra is not None:
                    f.write(struct.pack("<%dq" % len(files), *extra))


class Reader:
    def __init__(self, data):
        self.d, self.at = data, 0

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.d, self.at)
        self.at += struct.calcsize("<" + fmt)
        return list(v)

    def layout(self):
        rc, n = self.take("2i")
        msg = self.d[self.at:self.at + n].decode()
        self.at += n
        if rc:
            return rc, msg, None
        nf, nch = self.take("2i")
        r = {"first_channel": self.take("%di" % nf), "image_off": self.take("%dq" % nf), "counts": self.take("%di" % nch)}
        for k in ("pcm_off", "adpcm_off", "seek_off"):
            r[k] = self.take("%dq" % nch)
        for k in ("entries", "loop_start", "spacing", "file"):
            r[k] = self.take("%di" % nch)
        r["totals"] = self.take("5q")
        ng = self.take("i")[0]
        r["geom"] = [self.take("4I") for _ in range(ng)]
        na = self.take("i")[0]
        r["audio"] = [tuple(self.take("iI")) for _ in range(na)]
        nm = self.take("i")[0]
        r["meta"] = [tuple(self.take("2i")) for _ in range(nm)]
        return rc, msg, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("gc_files_host")
    exe = str(tmp / "gc_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, names = [], []
    for name, trim, cfg in [("none", 0, None)] + all_configs():
        cases.append((0, the_files(), cfg))
        names.append(("set", name, trim))
        cases.append((0, the_files() + [gf.gc_file(*b) for b in BIG], cfg))
        names.append(("big", name, trim))
    cases.append((0, [], gf.config(14, 1, 1)))
    names.append(("empty", "", 0))
    for name in sorted(REFUSED):
        bad, c, _ = REFUSED[name]
        cases.append((0, the_files()[:3] + [gf.gc_file(*bad)], gf.config(*c)))
        names.append(("refused", name, 0))
    infos = [good_info(1, 1), good_info(2, 100, 1), good_info(2, 100, 2), good_info(3, 5000, 7), good_info(1, 3_000_001), good_info(2, 0, 1),
             good_info(2, 3_000_001, 0x400), good_info(255, 15, 2)]
    sizes = [i.audio_offset + i.data_length for i in infos]
    odd, at = [], 8
    for sz in sizes:                                                   # bases 8 mod 16
        odd.append(at)
        at = gf.up(at + sz, 16) + 8
    cases += [(1, infos, None), (1, infos, odd), (1, [], None)]
    names += [("infos", "packed", 0), ("infos", "odd", 0), ("infos", "empty", 0)]
    bad = good_info()
    bad.interleave_size = 0
    cases.append((1, [good_info(), bad], None))
    names.append(("infos", "refused", 0))
    write_cases(tmp / "cases.bin", cases)
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(cases), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rd = Reader(open(tmp / "results.bin", "rb").read())
    out = {}
    for name, case in zip(names, cases):
        out[name] = (case, rd.layout())
    assert rd.at == len(rd.d)
    out["infos_sizes"], out["infos_odd"] = sizes, odd
    return out


def check_tiling(ranges, total, what):
    """the [start, end) ranges cover [0, total) exactly once"""
    at = 0
    for start, end in sorted(ranges):
        assert start == at and end > start, (what, start, end, at)
        at = end
    assert at == total, (what, at, total)


def test_host_layer_layout_is_the_model(driver):
    for key, value in driver.items():
        if not isinstance(key, tuple) or key[0] not in ("set", "big", "empty"):
            continue
        (kind, files, cfg), (rc, msg, r) = value
        assert rc == 0, (key, msg)
        m = gf.model(files, cfg)
        for k in ("first_channel", "counts", "pcm_off", "adpcm_off", "seek_off", "entries"):
            assert r[k] == m[k], (key, k)
        # the ragged batch's counts are the files' counts, repeated per channel
        assert r["counts"] == [f.channel.sample_count for f in files for _ in range(f.channels)]
        assert r["file"] == [i for i, f in enumerate(files) for _ in range(f.channels)]
        assert r["loop_start"] == [f.channel.loop_start for f in files for _ in range(f.channels)]
        assert r["totals"] == [m["pcm_samples"], m["adpcm_bytes"], m["seek_shorts"], m["image_bytes"], m["workspace"]]
        for c in range(len(r["counts"]) - 1):                          # empty rows take no room
            if r["counts"][c] == 0:
                assert r["pcm_off"][c] == r["pcm_off"][c + 1] and r["adpcm_off"][c] == r["adpcm_off"][c + 1]
        if cfg is not None:
            assert r["image_off"] == m["image_off"]
            assert [g[:3] for g in r["geom"]] == [[g["input"], g["interleave"], g["output"]] for g in m["geom"]]
        # metadata items: chunk 0 of every channel first, then every further 1024 entries
        nch = len(r["counts"])
        assert r["meta"][:nch] == [(c, 0) for c in range(nch)]
        assert sorted(r["meta"][nch:]) == [(c, e) for c in range(nch) for e in range(gf.CHUNK_ENTRIES, r["entries"][c], gf.CHUNK_ENTRIES)]


def test_writer_work_table_covers_every_audio_byte_once(driver):
    seen16 = seen8 = mixed = 0
    for key, value in driver.items():
        if not isinstance(key, tuple) or key[0] not in ("set", "big") or value[0][2] is None:
            continue
        (kind, files, cfg), (rc, msg, r) = value
        m = gf.model(files, cfg)
        per_file = {}
        for x, y in r["audio"]:
            per_file.setdefault(x, []).append(y)
        for f, g in enumerate(m["geom"]):
            total = g["output"] * g["channels"]
            assert m["image_size"][f] == 0x60 * g["channels"] + total
            ys = per_file.pop(f, [])
            if total == 0:
                assert not ys
                continue
            full, last = gf.writer_granules(g)
            assert r["geom"][f][3] == (full == 16) + 2 * (last == 16), (key, f)
            out_blocks = -(-g["output"] // g["interleave"])
            boundary = (out_blocks - 1) * g["interleave"] * g["channels"]
            ranges = []
            for y in ys:
                start, end, gran = gf.item_range(g, y)
                assert start < total, "an item wholly outside its image"
                assert gran == (full if start < boundary else last), (key, f, start)
                assert start % gran == 0 and (end % gran == 0 or g["channels"] == 1)
                ranges.append((start, end))
            check_tiling(ranges, total, (key, f))
            seen16 += full == 16 and g["channels"] > 1
            seen8 += full == 8
            mixed += full != last
        assert not per_file
    assert seen16 and seen8 and mixed, "the cases do not reach every granule choice"


def test_reader_work_table_covers_every_row_byte_once(driver):
    for which in ("packed", "odd"):
        (kind, infos, offs), (rc, msg, r) = driver[("infos", which, 0)]
        assert rc == 0, msg
        sizes = driver["infos_sizes"]
        want_off, at = [], 0
        for sz in sizes:
            want_off.append(at)
            at = gf.up(at + sz, 16)
        assert r["image_off"] == (want_off if offs is None else offs)
        end = max(gf.up(o + s, 16) for o, s in zip(r["image_off"], sizes))
        assert r["totals"][3] == end + 256
        assert r["counts"] == [i.sample_count for i in infos for _ in range(i.channel_count)]
        per_channel = {}
        for x, y in r["audio"]:
            per_channel.setdefault(x, []).append(y)
        for f, i in enumerate(infos):
            mono = i.channel_count == 1
            g = {"output": i.adpcm_bytes, "channels": i.channel_count}
            inp = i.adpcm_bytes if mono else i.data_length // i.channel_count
            il = gf.up(max(i.adpcm_bytes, 1), 16) if mono else i.interleave_size
            assert r["geom"][f][:3] == [inp, il, i.adpcm_bytes]
            allowed = r["image_off"][f] % 16 == 0 and (mono or (il % 16 == 0 and inp % 16 == 0))
            assert r["geom"][f][3] == int(allowed), (which, f)
            for c in range(r["first_channel"][f], r["first_channel"][f] + i.channel_count):
                ranges = []
                for y in per_channel.pop(c, []):
                    start, stop, gran = gf.item_range(g, y, reader=True)
                    assert gran == (16 if allowed else 8) and start < i.adpcm_bytes
                    ranges.append((start, stop))
                if i.adpcm_bytes:
                    check_tiling(ranges, i.adpcm_bytes, (which, f, c))
                else:
                    assert not ranges
        assert not per_channel
    assert not any(g[3] for g in driver[("infos", "odd", 0)][1][2]["geom"])
    assert any(g[3] for g in driver[("infos", "packed", 0)][1][2]["geom"])


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        _, (rc, msg, _) = driver[("refused", name, 0)]
        assert rc == REFUSED[name][2] and re.search(r"file %d\b" % NAMED.get(name, 3), msg), (name, rc, msg)
    _, (rc, msg, _) = driver[("infos", "refused", 0)]
    assert rc == ARG and re.search(r"file 1\b", msg)
    _, (rc, msg, r) = driver[("empty", "", 0)]
    assert rc == 0 and r["totals"] == [128, 256, 0, 256, 0] and not r["audio"] and not r["meta"]
    _, (rc, msg, r) = driver[("infos", "empty", 0)]
    assert rc == 0 and r["totals"][3] == 256 and not r["audio"]
