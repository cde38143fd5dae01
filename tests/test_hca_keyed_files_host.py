"""include/vgaudio_hip_files/hca_keyed_files.h without a GPU: the header's functions are exported and in the ctypes table with
the header's argument counts, the new names are declared in the new header only, the GPU file's table of cases names every
function and puts the two device calls through the disciplines of the sibling sets, the search's work items tile every
(file, candidate) exactly once (against a Python model), the workspace's size against that model, every refusal with its code
and message through the HIP-free host layer (vgaudio_amd/csrc/hca_keyed_files_host.hpp), the shared frame walk
(hca_keyed_walk.hpp) against the oracle for every (file, candidate) singly and for every file and candidate list -- both in a
stand-alone driver under AddressSanitizer and UBSan, a child process --, and that the case table
(tests/hca_keyed_files_cases.py), computed with the oracle alone, holds what it says it holds."""
import ast
import ctypes as C
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hca_keyed_files_cases as kc
from oracle import pyoracle as po
from test_gc_files_host import Reader, _declared
from vgaudio_amd import _lib
from vgaudio_amd.hca import HcaFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "hca_keyed_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_hca_keyed_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "hca_keyed_files_host_driver.cpp")

NAMES = ["vga_hca_find_keys_workspace_bytes", "vga_hca_find_keys_device_v", "vga_hca_read_keyed_device_v", "vga_hca_find_keys_items_for"]
DEVICE_CALLS = NAMES[1:3]
ARG, OP = _lib.VGA_ERR_ARGUMENT, -4
FIND, READ, WORKSPACE, ITEMS = range(4)
SMALL = 8                                                              # files of the sets the refusals are checked on


def L():
    return _lib.lib()


# ---------------------------------------------------------------- the header against the library and the ctypes table
def test_header_functions_are_exported_with_the_headers_argument_counts():
    declared = _declared(HEADER)
    assert sorted(declared) == sorted(NAMES)
    lib = C.CDLL(_lib.SO_PATH)
    assert not [n for n in declared if not hasattr(lib, n)]
    assert not [n for n in declared if n not in _lib.SIGNATURES]
    wrong = {n: (len(_lib.SIGNATURES[n][1]), c) for n, c in declared.items() if len(_lib.SIGNATURES[n][1]) != c}
    assert not wrong, f"(ctypes, header) argument counts differ: {wrong}"
    assert C.sizeof(_lib.HcaFindKeysItemC) == 12


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
    for name in DEVICE_CALLS:
        assert {"test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once",
                "test_refused_calls_launch_nothing"} <= set(cases[name]), name
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- an empty set and null arguments need no GPU
def test_an_empty_set_and_null_arguments():
    f = L()
    r = HcaFileSet.from_infos([])
    assert f.vga_hca_find_keys_device_v(r._h, None, None, 0, -1, None, None, None, 0, None) == 0
    assert f.vga_hca_read_keyed_device_v(r._h, None, None, 0, None, None, None, None, None) == 0
    assert f.vga_hca_find_keys_workspace_bytes(r._h, 7) == 0 and f.vga_hca_find_keys_workspace_bytes(None, 7) == 0
    r.close()
    assert f.vga_hca_find_keys_device_v(None, None, None, 1, -1, None, None, None, 0, None) == ARG
    assert f.vga_hca_read_keyed_device_v(None, None, None, 1, None, None, None, None, None) == ARG
    assert HcaFileSet.find_items([], 5) == []
    count = C.c_int64()
    assert f.vga_hca_find_keys_items_for(None, 2, 3, None, 0, C.byref(count)) == ARG
    info = kc.table()["infos"][kc.index_of("first")]
    ptrs, items = (C.c_void_p * 1)(C.addressof(info)), (_lib.HcaFindKeysItemC * 1)()
    assert f.vga_hca_find_keys_items_for(ptrs, 1, 3, items, 0, C.byref(count)) == ARG and count.value == 1
    assert f.vga_hca_find_keys_items_for(ptrs, 1, -3, items, 1, C.byref(count)) == ARG


# ---------------------------------------------------------------- the search's work items against the model
def test_find_items_tile_every_file_and_candidate_once():
    t = kc.table()
    for nkeys in (0, 1, 63, 64, 65, 130):
        items = [(i.file, i.first_key, i.key_count) for i in HcaFileSet.find_items(t["infos"], nkeys)]
        assert items == kc.find_items_model(t["types"], nkeys)
        seen = {}
        for f, first, count in items:
            assert 0 < count <= kc.KEY_BLOCK and t["types"][f] == 56
            for k in range(first, first + count):
                assert (f, k) not in seen
                seen[(f, k)] = 1
        assert len(seen) == nkeys * sum(e == 56 for e in t["types"])


# ---------------------------------------------------------------- the stand-alone driver
I, T, X, W, F = 0x10000, 0x20003, 0x30000, 0x40000, 0x50000            # images, tables (at an odd byte), index out, workspace, frames


def the_calls():
    """set name -> [(what, four addresses, (n0, n1), bytes, code, a piece of the message)]"""
    need = kc.workspace_model(SMALL, 12)
    read_calls = [
        (FIND, (I, T, X, W), (12, 12), need, 0, ""),
        (FIND, (I, T, X, W), (12, -1), need + 100, 0, ""),
        (FIND, (I, 0, X, W), (0, 5), kc.workspace_model(SMALL, 0), 0, ""),   # no candidates: no tables to read
        (FIND, (I, T, X, W), (-1, 0), need, ARG, "negative candidate count"),
        (FIND, (I, T, X, W), (12, -2), need, ARG, "type1_index -2"),
        (FIND, (I, 0, X, W), (12, 0), need, ARG, "null d_tables"),
        (FIND, (I, T, 0, W), (12, 0), need, ARG, "null d_key_index_out"),
        (FIND, (0, T, X, W), (12, 0), need, ARG, "null pointer"),
        (FIND, (I + 4, T, X, W), (12, 0), need, ARG, "16-byte alignment"),
        (FIND, (I, T, X, W), (12, 0), need - 1, ARG, "the workspace needs %d bytes" % need),
        (FIND, (I, T, X, 0), (12, 0), need, ARG, "the workspace needs %d bytes" % need),
        (FIND, (I, T, X, W + 2), (12, 0), need, ARG, "the workspace needs %d bytes" % need),
        (READ, (I, T, F), (13, 0), 0, 0, ""),
        (READ, (I, T, F), (0, 0), 0, ARG, "0 tables"),
        (READ, (I, T, F), (-3, 0), 0, ARG, "-3 tables"),
        (READ, (I, 0, F), (13, 0), 0, ARG, "null d_tables"),
        (READ, (0, T, F), (13, 0), 0, ARG, "null pointer"),
        (READ, (I, T, 0), (13, 0), 0, ARG, "null pointer"),
        (READ, (I + 1, T, F), (13, 0), 0, ARG, "alignment"),
        (READ, (I, T, F + 2), (13, 0), 0, ARG, "alignment"),
        (WORKSPACE, (), (12, 0), 0, 0, ""),
        (WORKSPACE, (), (0, 0), 0, 0, ""),
        (WORKSPACE, (), (130, 0), 0, 0, ""),
        (WORKSPACE, (), (-1, 0), 0, 0, ""),
        (ITEMS, (), (130, 0), 0, 0, ""),
    ]
    own_calls = [
        (FIND, (I, T, X, W), (12, 0), need, OP, "keys of its own"),
        (READ, (I, T, F), (13, 0), 0, OP, "keys of its own"),
    ]
    write_calls = [
        (FIND, (I, T, X, W), (12, 0), need, OP, "not made from parsed headers"),
        (READ, (I, T, F), (13, 0), 0, OP, "not made from parsed headers"),
        (WORKSPACE, (), (12, 0), 0, 0, ""),
    ]
    unusable_calls = [                                                 # only the search needs the header's channel layout
        (FIND, (I, T, X, W), (12, 0), need, ARG, "file 2: HcaInfo is inconsistent"),
        (FIND, (I, 0, X, W), (0, 0), need, ARG, "file 2: HcaInfo is inconsistent"),
        (READ, (I, T, F), (13, 0), 0, 0, ""),
    ]
    return {"read": read_calls, "own": own_calls, "write": write_calls, "unusable": unusable_calls}


SETS = [("read", 0), ("own", 1), ("write", 2), ("unusable", 3)]
LIST_NAMES = sorted(kc.LISTS)


def write_cases(path):
    t, calls = kc.table(), the_calls()
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", C.sizeof(_lib.HcaFileInfoC), kc.NCODES) + t["dec"].tobytes())
        f.write(struct.pack("<i", len(kc.FILES)))
        for n, info in enumerate(t["infos"]):
            stored = np.ascontiguousarray(t["stored"][n]).tobytes()
            f.write(bytes(info) + struct.pack("<iq", len(t["single"].get(n, [])), len(stored)) + stored)
        f.write(struct.pack("<i", len(LIST_NAMES)))
        for name in LIST_NAMES:
            codes = kc.LISTS[name]
            f.write(struct.pack("<2i%di" % len(codes), len(codes), len(codes), *codes))
        f.write(struct.pack("<i", len(SETS)))
        for name, kind in SETS:
            f.write(struct.pack("<3i", kind, SMALL, len(calls[name])))
            for what, addresses, n, nbytes, _, _ in calls[name]:
                a = list(addresses) + [0] * (4 - len(addresses))
                f.write(struct.pack("<i4q2iq", what, *a, n[0], n[1], nbytes))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers, computed once: {"files": [(first, ntest, singles, per list)], set name: [answers]}"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("hca_keyed_files_host")
    exe = str(tmp / "hca_keyed_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    write_cases(tmp / "cases.bin")
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "4 ok", r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rd = Reader(open(tmp / "results.bin", "rb").read())
    t, files = kc.table(), []
    for n in range(len(kc.FILES)):
        first, ntest = rd.take("2i")
        singles = [tuple(rd.take("2i")) for _ in t["single"].get(n, [])]
        files.append((first, ntest, singles, {name: tuple(rd.take("2i")) for name in LIST_NAMES}))
    out = {"files": files}
    for name, _ in SETS:
        answers = []
        for what in [None] + [c[0] for c in the_calls()[name]]:
            rc, n = rd.take("2i")
            msg = rd.d[rd.at:rd.at + n].decode()
            rd.at += n
            extra = None
            if what == WORKSPACE:
                extra = rd.take("q")[0]
            elif what == ITEMS:
                extra = [tuple(rd.take("3i")) for _ in range(rd.take("i")[0])]
            answers.append((rc, msg, extra))
        assert answers[0][0] == 0, answers[0]
        out[name] = answers[1:]
    assert rd.at == len(rd.d)
    return out


def test_the_shared_walk_gives_the_oracles_verdict_for_every_file_and_candidate(driver):
    t = kc.table()
    pairs = 0
    for n, (first, ntest, singles, lists) in enumerate(driver["files"]):
        assert (first, ntest) == t["first"][n], kc.NAMES[n]
        for k, got in enumerate(singles):
            assert got == ((0, 0) if t["single"][n][k] == 0 else kc.verdict(t["single"][n][k])), (kc.NAMES[n], k, got)
            pairs += 1
        for name in LIST_NAMES:
            assert lists[name] == t["found"][name][n], (kc.NAMES[n], name, lists[name])
    assert pairs > 500


def test_every_refusal_has_its_code_and_message(driver):
    for name, calls in the_calls().items():
        for (what, addresses, n, nbytes, code, piece), (rc, msg, extra) in zip(calls, driver[name]):
            assert rc == code, (name, what, addresses, n, rc, msg)
            if code:
                assert piece in msg and msg.startswith(("vga_hca_find_keys_device_v: ", "vga_hca_read_keyed_device_v: ")[what]), (name, what, msg)


def test_workspace_size_and_items_are_the_models(driver):
    sizes = [(n[0], extra) for (what, _, n, _, _, _), (_, _, extra) in zip(the_calls()["read"], driver["read"]) if what == WORKSPACE]
    assert len(sizes) == 4
    for nkeys, got in sizes:
        assert got == (kc.workspace_model(SMALL, nkeys) if nkeys >= 0 else 0), (nkeys, got)
    assert [e for (w, _, _, _, _, _), (_, _, e) in zip(the_calls()["write"], driver["write"]) if w == WORKSPACE] == [0]
    items = next(e for (w, _, _, _, _, _), (_, _, e) in zip(the_calls()["read"], driver["read"]) if w == ITEMS)
    assert items == kc.find_items_model(kc.table()["types"][:SMALL], 130)


# ---------------------------------------------------------------- the case table holds what it is for
def test_the_table_holds_what_it_says():
    t = kc.table()
    found, first, x = t["found"], t["first"], kc.index_of
    assert len(kc.FILES) >= 24 and max(f[3] for f in kc.FILES) <= 14
    assert {f[1] for f in kc.FILES} == {1, 2} and {f[2] for f in kc.FILES} == {"High", "Low"}
    assert t["types"][x("type0")] == 0 and t["types"][x("type1")] == 1
    main = found["main"]
    # the right key as first, middle and last candidate; absent; the type rules
    assert main[x("first")] == (0, 0) and main[x("middle")] == (5, 0) and main[x("last")] == (len(kc.LISTS["main"]) - 1, 0)
    assert main[x("absent")] == (-1, 1) and found["n130"][x("absent")] == (100, 0)
    assert main[x("type0")] == (-1, 0) and main[x("type1")] == (len(kc.LISTS["main"]), 0)
    # silence: every key passes; testing starts behind the silent frames; fewer than ten frames; no frames at all
    assert first[x("silent")] == (0, 10) and main[x("silent")] == (0, 0) and set(t["single"][x("silent")]) == {0}
    assert first[x("silent3")] == (3, 10) and main[x("silent3")] == (4, 0)
    assert first[x("short_tail")] == (3, 4) and main[x("short_tail")] == (6, 0)
    assert first[x("no_frames")] == (0, 0) and main[x("no_frames")] == (0, 0) and found["none"][x("no_frames")] == (-1, 1)
    # damage inside the ten tested frames changes the answer, behind them it does not
    assert main[x("damage10")] == (-1, 1) and main[x("damage11")] == (8, 0)
    # a wrong sync word in the third tested frame: with the right key in the list, and without
    assert main[x("sync_with_key")] == (-1, 2) and found["n1"][x("sync_with_key")] == (-1, 1)
    assert main[x("sync_without_key")] == (-1, 1) and found["n130"][x("sync_without_key")] == (-1, 2)
    assert t["single"][x("sync_with_key")].count(-3) == 1
    # wrong keys pass: more than one of them, so "the first passing candidate" decides; behind a frame every key passes too
    hits = [k for k, v in enumerate(t["single"][x("random_a")]) if v == 0]
    assert len(hits) >= 2 and found["n130"][x("random_a")] == (hits[0], 0) and found["n65"][x("random_a")] == (-1, 1)
    behind = [k for k, v in enumerate(t["single"][x("random_b")]) if v == 0]
    assert behind and set(behind) <= set(hits) and found["n130"][x("random_b")] == (behind[0], 0)
    assert first[x("random_b")] == (0, 2) and first[x("random_c")] == (0, 10) and found["n130"][x("random_c")] == (-1, 1)
    for name in ("random_a", "random_b", "random_c"):
        stored = t["stored"][x(name)]
        assert (stored[:, :2] == 0xFF).all() and (stored[-1:, 2] <= 0x0F).all()
    # candidate counts around the item size, the right key at 0, 63, 64 and 129
    assert [len(kc.LISTS[n]) for n in ("n1", "n63", "n64", "n65", "n130")] == [1, 63, 64, 65, 130]
    assert found["n1"][x("first")] == (0, 0) and found["n63"][x("key63")] == (-1, 1) and found["n64"][x("key63")] == (63, 0)
    assert found["n64"][x("key64")] == (-1, 1) and found["n65"][x("key64")] == (64, 0) and found["n130"][x("key129")] == (129, 0)
    # frame sizes: the parser's smallest, one past the staging threshold, 32767, both sides of the span form
    sizes = {i.hca.frame_size for i in t["infos"]}
    assert {8, kc.STAGE_MAX_FRAME + 1, 32767, 4096, 4097} <= sizes
    # every candidate survives the first frame of the files made for it, so the later frames are walked by all of them: out
    # of global memory (above STAGE_REST_BYTES together, one file also above STAGE_MAX_FRAME), and staged at the limit
    later = lambda n: (first[n][1] - 1) * t["infos"][n].hca.frame_size
    for name in ("random_b", "random_c", "lead_32767", "lead_1024", "lead_1025"):
        assert len(t["first_frame_passes"][x(name)]) == kc.NSINGLE and first[x(name)][1] > 1, name
    assert later(x("lead_1024")) == kc.STAGE_REST_BYTES and later(x("lead_1025")) == kc.STAGE_REST_BYTES + 9
    assert later(x("lead_32767")) > kc.STAGE_REST_BYTES and t["infos"][x("lead_32767")].hca.frame_size > kc.STAGE_MAX_FRAME
    assert len(t["first_frame_passes"][x("first")]) == 1 and not t["first_frame_passes"][x("absent")]
    # every status and every index rule occurs
    assert {s for row in found.values() for _, s in row} == {0, 1, 2}
    assert all(found["none"][n] == (-1, 1) for n, e in enumerate(t["types"]) if e == 56)
    # the read's indices: valid, negative and >= ntables
    idx = kc.read_key_indices()
    assert min(idx) < -1 and -1 in idx and max(idx) > kc.NCODES + 1 and kc.NCODES + 1 in idx and kc.NCODES in idx
    # the images are the oracle's: reading them back gives the header that was written
    for n, data in enumerate(t["datas"]):
        rc, info, _, etype, _, _ = po.hcafile_read(data)
        assert rc == 0 and etype == t["types"][n] and info.frame_size == t["oinfo"][n].frame_size
