"""include/vgaudio_hip_files/hca_ragged_loops.h without a GPU: the header's functions are exported and in the ctypes table with
the header's argument counts, they are declared nowhere else, the GPU file's table of cases names every one of them;
vga_hca_loop_may_read_tail against the CPU oracle (predicate 0 must mean that the audio behind SampleCount never reaches the
frames); the routing of hca.write_files; and the refusal of a null object."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

import hca_loop_cases as lc
from oracle import pyoracle as po
from vgaudio_amd import _lib, crihca, hca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "hca_ragged_loops.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_hca_ragged_loops.py")
NAMES = ["vga_hca_loop_may_read_tail", "vga_hca_encode_loops_device_v"]


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


# ---------------------------------------------------------------- the header against the library and the ctypes table
def test_header_functions_are_exported_with_the_headers_argument_counts():
    declared = _declared(HEADER)
    assert sorted(declared) == sorted(NAMES)
    assert declared == {"vga_hca_loop_may_read_tail": 1, "vga_hca_encode_loops_device_v": 5}
    lib = C.CDLL(_lib.SO_PATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    wrong = {n: (len(_lib.SIGNATURES[n][1]), c) for n, c in declared.items() if len(_lib.SIGNATURES[n][1]) != c}
    assert not wrong, f"(ctypes, header) argument counts differ: {wrong}"
    hook = _declared(os.path.join(ROOT, "include", "vgaudio_hip_testing.h"))
    assert hook["vga_testing_hca_encode_v_stats"] == len(_lib.SIGNATURES["vga_testing_hca_encode_v_stats"][1]) == 2
    assert hasattr(lib, "vga_testing_hca_encode_v_stats")


def test_the_new_names_are_declared_in_the_new_header_only():
    inc = os.path.join(ROOT, "include")
    seen = 0
    for base, _, files in os.walk(inc):
        for f in sorted(files):
            path = os.path.join(base, f)
            if f.endswith(".h") and os.path.abspath(path) != os.path.abspath(HEADER):
                seen += 1
                assert not [n for n in NAMES if n in _declared(path)], path
    assert seen >= 10
    assert not [n for n in _declared(HEADER) if n.startswith("vga_testing_")]
    # the older header keeps its list of functions: the new call did not go there
    assert "vga_hca_encode_loops_device_v" not in _strip(open(os.path.join(inc, "vgaudio_hip", "hca_ragged.h")).read())


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    assert {"test_bytes_do_not_depend_on_poison_or_run_length", "test_round_trip_on_a_busy_stream_and_two_streams_at_once",
            "test_refused_layouts_launch_nothing"} <= set(cases["vga_hca_encode_loops_device_v"])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the predicate against the oracle
def _frames_change_with_the_tail(nch, n, loop, k=3):
    """(HcaInfo, whether the oracle's frames change when the audio behind SampleCount is replaced by noise)"""
    params = lc.params_of(nch, n, loop)
    pcm = po.synth_generate(nch, n, first_channel=k)
    rc, oi, frames = po.hca_encode(pcm, params)
    assert rc == 0
    rc, _, noisy = po.hca_encode(lc.noise_behind(pcm, oi.sample_count), params)
    assert rc == 0
    return lc.info_of(params), not np.array_equal(frames, noisy)


def test_predicate_is_the_headers_formula():
    for nch in (1, 2, 6):
        for c in lc.LOOP_CASES + lc.TAIL_READERS:
            h = lc.info_of(lc.params_of(nch, c[0], c[1:]))
            post, loop_len = lc.post_and_loop(h)
            assert 256 <= post <= 383
            assert crihca.loop_may_read_tail(h) == (loop_len < post), (nch, c)
            assert L().vga_hca_loop_may_read_tail(C.byref(h)) == int(loop_len < post)
    assert crihca.loop_may_read_tail(lc.info_of(lc.params_of(2, 5000))) is False       # a stream that does not loop
    # the boundary is exact
    a, b = (lc.info_of(lc.params_of(1, 20000, (s, 15000))) for s in (14640, 14641))
    assert lc.post_and_loop(a) == (360, 360) and lc.post_and_loop(b) == (360, 359)
    assert not crihca.loop_may_read_tail(a) and crihca.loop_may_read_tail(b)


def test_predicate_refuses_a_bad_info():
    assert L().vga_hca_loop_may_read_tail(None) == _lib.VGA_ERR_ARGUMENT
    h = lc.info_of(lc.params_of(1, 5000, (0, 5000)))
    h.inserted_samples = 100                                          # less than the 128 the MDCT leads in with
    assert L().vga_hca_loop_may_read_tail(C.byref(h)) < 0
    with pytest.raises(_lib.ArgumentError):
        crihca.loop_may_read_tail(h)


def test_predicate_zero_means_the_tail_never_reaches_the_frames():
    sets = [(nch,) + c for nch in (1, 2) for c in lc.LOOP_CASES]
    rng = np.random.default_rng(20261021)
    while len(sets) < 2 * len(lc.LOOP_CASES) + 100:                   # a seeded sweep of 100 further parameter sets
        n = int(rng.integers(300, 12001))
        end = int(rng.integers(2, n + 1))
        start = int(rng.integers(0, end))
        nch = int(rng.integers(1, 3))
        if po.hca_init(lc.params_of(nch, n, (start, end)))[0] == 0:
            sets.append((nch, n, start, end))
    zeros = 0
    for nch, n, start, end in sets:
        h, changed = _frames_change_with_the_tail(nch, n, (start, end))
        if not crihca.loop_may_read_tail(h):
            zeros += 1
            assert not changed, (nch, n, start, end)
    assert zeros >= 40, "the sweep must exercise the predicate's 0 side"


@pytest.mark.parametrize("case", lc.TAIL_READERS)
def test_predicate_one_cases_do_read_the_tail(case):
    h, changed = _frames_change_with_the_tail(1, case[0], case[1:])
    assert crihca.loop_may_read_tail(h) and changed


def test_every_case_initializes_in_every_class():
    for name, streams in lc.classes().items():
        loops = [s for s in streams if s.info.looping]
        assert [(s.n,) + tuple(s.loop) for s in loops] == lc.LOOP_CASES
        assert {0, 500} <= {s.n for s in streams if not s.info.looping}
        assert any(s.info.frame_count == 1 for s in streams) and max(s.info.frame_count for s in streams) <= 24
        assert any(s.info.inserted_samples - 128 >= 1024 for s in loops) or name == "six"     # whole cleared frames
        crihca.RaggedHca.layout([s.info for s in streams])            # one shape class


# ---------------------------------------------------------------- the routing of hca.write_files
def test_write_files_routing():
    def info(nch, n, loop=None):
        return lc.info_of(lc.params_of(nch, n, loop))
    files = [
        (info(1, 5000), 5000),                                  # 0 plain mono
        (info(1, 20000, (3000, 15000)), 20000),                 # 1 looping mono, tail never read: joins
        (info(2, 7000), 7000),                                  # 2 plain stereo
        (info(1, 20000, (14641, 15000)), 20000),                # 3 reads the tail and has one: single
        (info(1, 300, (100, 300)), 300),                        # 4 would read a tail, has none: joins
        (info(2, 9000, (1024, 9000)), 9000),                    # 5 looping stereo: joins the stereo class
        (info(6, 5000, (0, 5000)), 5000),                       # 6 looping, alone in its class: single
        (info(4, 3000), 3000),                                  # 7 plain, alone in its class: stays a group
        (info(1, 0), 0),                                        # 8 no samples
    ]
    assert [crihca.loop_may_read_tail(h) for h, _ in files] == [False, False, False, True, True, False, False, False, False]
    groups, singles = hca.plan_write_groups([h for h, _ in files], [n for _, n in files])
    assert groups == [[0, 1, 4, 8], [2, 5], [7]] and singles == [3, 6]
    assert hca.plan_write_groups([], []) == ([], [])
    # a folder of looping files of one class: one group, no single
    infos = [info(2, 4000 + 700 * k, (100 * k, 3000 + 700 * k)) for k in range(6)]
    assert hca.plan_write_groups(infos, [4000 + 700 * k for k in range(6)]) == ([[0, 1, 2, 3, 4, 5]], [])
    # two files that read their tails but share a class with others: singles, the others still grouped
    infos = [info(1, 20000, (14641, 15000)), info(1, 20000, (14800, 15000)), info(1, 9000, (1024, 9000)), info(1, 8000, (0, 8000))]
    assert hca.plan_write_groups(infos, [20000, 20000, 9000, 8000]) == ([[2, 3]], [0, 1])


# ---------------------------------------------------------------- refusals that need no GPU
def test_a_null_object_is_refused_without_a_gpu():
    assert L().vga_hca_encode_loops_device_v(None, None, None, None, None) == _lib.VGA_ERR_ARGUMENT
    assert b"vga_hca_encode_loops_device_v" in L().vga_last_error()
