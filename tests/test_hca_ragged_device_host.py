"""include/vgaudio_hip/hca_ragged.h without a GPU: the header's functions are exported and in the ctypes table with the header's
argument counts (the header lies outside the directory listing tests/test_abi_exports.py reads, so the same regexes are pointed
at it here), the packed layout (vga_hca_ragged_layout_for is host code), what it refuses, and that the GPU file's table of cases
names every function the header declares."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

from vgaudio_amd import _lib
from vgaudio_amd.crihca import RaggedHca, RaggedTotalsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "hca_ragged.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_hca_ragged_device.py")


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


NAMES = ["vga_hca_ragged_layout_for", "vga_hca_ragged_create", "vga_hca_ragged_destroy", "vga_hca_ragged_streams",
         "vga_hca_ragged_totals_of", "vga_hca_ragged_offsets", "vga_hca_decode_device_v", "vga_hca_encode_device_v"]


def L():
    return _lib.lib()


def info(nch, n, quality=2, loop=None, rate=48000):
    p = _lib.HcaParamsC(quality, 0, 0, nch, rate, n, 0, 0, 0)
    if loop:
        p.looping, p.loop_start, p.loop_end = 1, loop[0], loop[1]
    h = _lib.HcaInfoC()
    _lib.check(L().vga_hca_encoder_initialize(C.byref(p), C.byref(h)))
    return h


# ---------------------------------------------------------------- the header against the library and the ctypes table
def test_header_functions_are_exported_with_the_headers_argument_counts():
    declared = _declared(HEADER)
    assert sorted(declared) == sorted(NAMES)
    lib = C.CDLL(_lib.SO_PATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert not [n for n in declared if n not in _lib.SIGNATURES]
    wrong = {n: (len(_lib.SIGNATURES[n][1]), c) for n, c in declared.items() if len(_lib.SIGNATURES[n][1]) != c}
    assert not wrong, f"(ctypes, header) argument counts differ: {wrong}"
    hook = _declared(os.path.join(ROOT, "include", "vgaudio_hip_testing.h"))
    assert hook["vga_testing_hca_ragged_stats"] == len(_lib.SIGNATURES["vga_testing_hca_ragged_stats"][1]) == 3
    assert hasattr(lib, "vga_testing_hca_ragged_stats")


def test_the_new_names_are_declared_in_the_new_header_only():
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        if f.endswith(".h"):
            names = _declared(os.path.join(inc, f))
            assert not [n for n in NAMES if n in names], f
            assert "vga_hca_ragged" not in _strip(open(os.path.join(inc, f)).read()), f
    assert not [n for n in _declared(HEADER) if n.startswith("vga_testing_")]
    assert "vga_testing_" not in _strip(open(HEADER).read())


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    source = open(GPU_FILE).read()
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    # the two calls that launch are exercised under every discipline the older files apply to the top-level headers
    for name in ("vga_hca_decode_device_v", "vga_hca_encode_device_v"):
        assert {"test_bytes_do_not_depend_on_poison_or_run_length", "test_round_trip_on_a_busy_stream_and_two_streams_at_once",
                "test_refused_layouts_launch_nothing"} <= set(cases[name])
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout
def _seeded_infos(nch, seed, count=30):
    rng = np.random.default_rng(seed)
    ns = [0, 1, 896, 897, 1024 * 3 - 128] + [int(rng.integers(1, 40000)) for _ in range(count)]
    infos = [info(nch, n) for n in ns]
    infos.insert(3, info(nch, 30000, loop=(1000, 20000)))
    infos.insert(9, info(nch, 5000, loop=(0, 5000)))
    zero_frames = info(nch, 4000)
    zero_frames.frame_count = 0                                       # a header without frames
    infos.insert(12, zero_frames)
    return infos


@pytest.mark.parametrize("nch", [1, 2, 6])
def test_layout_offsets_alignments_and_totals(nch):
    infos = _seeded_infos(nch, 100 + nch)
    assert {0, 1} <= {h.frame_count for h in infos} and any(h.looping for h in infos) and any(h.sample_count == 0 for h in infos)
    fo, ro, tot = RaggedHca.layout(infos)
    assert len(fo) == len(infos) and len(ro) == tot.rows == nch * len(infos)
    assert tot.total_frames == sum(h.frame_count for h in infos)
    end = 0
    for h, at in zip(infos, fo):                                      # ascending, back to back rounded up to 4, no overlap
        assert at == end and at % 4 == 0
        end = at + (h.frame_count * h.frame_size + 3) // 4 * 4
    assert tot.frame_bytes == end + 8
    end, i = 0, 0
    for h in infos:                                                   # stream-major rows, rounded up to 8 samples
        for _ in range(nch):
            assert ro[i] == end and ro[i] % 8 == 0
            end += (h.sample_count + 7) // 8 * 8
            i += 1
    assert tot.pcm_samples == end
    assert tot.decode_workspace_bytes == tot.total_frames * L().vga_hca_decode_workspace_bytes(C.byref(info(nch, 800)), 1)
    # a stream without frames / samples takes no room: its offset is the next stream's
    for s, h in enumerate(infos[:-1]):
        if h.frame_count == 0:
            assert fo[s] == fo[s + 1]
        if h.sample_count == 0:
            assert ro[s * nch] == ro[(s + 1) * nch]
    # outputs one at a time
    only = RaggedTotalsC()
    assert L().vga_hca_ragged_layout_for((_lib.HcaInfoC * len(infos))(*infos), len(infos), None, None, C.byref(only)) == 0
    assert all(getattr(only, f) == getattr(tot, f) for f, _ in only._fields_)


def test_layout_of_an_empty_batch():
    fo, ro, tot = RaggedHca.layout([])
    assert len(fo) == len(ro) == 0 and (tot.frame_bytes, tot.pcm_samples, tot.rows, tot.total_frames, tot.decode_workspace_bytes) == (8, 0, 0, 0, 0)


# ---------------------------------------------------------------- refusals
def test_a_second_shape_class_is_refused_and_named():
    for others in ([info(1, 5000), info(1, 900), info(2, 5000)], [info(2, 5000, quality=2), info(2, 700, quality=2), info(2, 5000, quality=4)]):
        with pytest.raises(_lib.ArgumentError, match="stream 2"):
            RaggedHca.layout(others)
    # loop fields, header size and comment length are free
    a, b = info(1, 5000), info(1, 30000, loop=(1000, 20000))
    b.comment_length, b.header_size = 40, b.header_size + 64
    RaggedHca.layout([a, b])


def test_null_pointers_and_a_negative_count_are_refused():
    tot = RaggedTotalsC()
    one = (_lib.HcaInfoC * 1)(info(1, 5000))
    f = L().vga_hca_ragged_layout_for
    assert f(None, 1, None, None, C.byref(tot)) == _lib.VGA_ERR_ARGUMENT
    assert f(one, -1, None, None, C.byref(tot)) == _lib.VGA_ERR_ARGUMENT
    assert f(one, 1, None, None, None) == _lib.VGA_ERR_ARGUMENT
    assert L().vga_hca_ragged_create(one, 1, None) == _lib.VGA_ERR_ARGUMENT
    out = C.c_void_p()
    assert L().vga_hca_ragged_create(None, 1, C.byref(out)) == _lib.VGA_ERR_ARGUMENT and not out.value
    assert L().vga_hca_ragged_create(one, -1, C.byref(out)) == _lib.VGA_ERR_ARGUMENT and not out.value
    assert L().vga_hca_ragged_totals_of(None, C.byref(tot)) == _lib.VGA_ERR_ARGUMENT
    assert L().vga_hca_ragged_offsets(None, None, None) == _lib.VGA_ERR_ARGUMENT
    assert L().vga_hca_ragged_streams(None) == 0
    L().vga_hca_ragged_destroy(None)
    assert L().vga_hca_decode_device_v(None, None, None, None, 0, None, None) == _lib.VGA_ERR_ARGUMENT
    assert L().vga_hca_encode_device_v(None, None, None, None, None) == _lib.VGA_ERR_ARGUMENT


def test_an_info_the_decoder_refuses_is_refused_with_the_same_code():
    bad = info(2, 5000)
    bad.frame_size = 4
    other = info(2, 5000)
    other.total_band_count = 200
    for h in (bad, other):
        d = (C.c_char * 240)()
        want = L().vga_testing_hca_device_info(C.byref(h), d, 240)
        assert want < 0
        tot = RaggedTotalsC()
        assert L().vga_hca_ragged_layout_for((_lib.HcaInfoC * 2)(info(2, 800), h), 2, None, None, C.byref(tot)) == want
