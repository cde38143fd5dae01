"""include/vgaudio_hip_files/adx_keyed_files.h without a GPU: the header's functions are exported and in the ctypes table with
the header's argument counts, the new names are declared in the new header only, the GPU file's table of cases names every
function and puts the three device calls through the disciplines of the sibling sets, the search's work items tile every slot
of every file exactly once (against a Python model), the workspace's size against that model, every refusal with its code
and message through the HIP-free host layer (vgaudio_amd/csrc/adx_keyed_files_host.hpp), adx_lcg.hpp's jump against serial
stepping -- both in a stand-alone driver under AddressSanitizer and UBSan, a child process --, and that the case table
(tests/adx_keyed_files_cases.py), computed with the oracle alone, holds what it says it holds."""
import ast
import ctypes as C
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

import adx_keyed_files_cases as kc
from oracle import pyoracle as po
from oracle.pyref import crypt as pycrypt
from test_gc_files_host import Reader, _declared, check_tiling
from vgaudio_amd import _lib
from vgaudio_amd.adx import AdxFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip_files", "adx_keyed_files.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_adx_keyed_files.py")
DRIVER = os.path.join(ROOT, "tests", "host", "adx_keyed_files_host_driver.cpp")

NAMES = ["vga_adx_write_keyed_device_v", "vga_adx_read_keyed_device_v", "vga_adx_find_keys_workspace_bytes",
         "vga_adx_find_keys_device_v", "vga_adx_find_keys_items_for"]
DEVICE_CALLS = NAMES[:2] + NAMES[3:4]
ARG, OP = _lib.VGA_ERR_ARGUMENT, -4
WRITE, READ, FIND, WORKSPACE, ITEMS = range(5)


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
    assert C.sizeof(_lib.AdxFindKeysItemC) == 12 and C.sizeof(_lib.AdxKeyC) == 12


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
    s, r = AdxFileSet([]), AdxFileSet.from_infos([])
    assert f.vga_adx_write_keyed_device_v(s._h, None, None, None, 0, None, None, None, None) == 0
    assert f.vga_adx_read_keyed_device_v(r._h, None, None, 0, None, None, None, None, None) == 0
    assert f.vga_adx_find_keys_device_v(r._h, None, None, 0, 0, None, None, 0, None) == 0
    assert f.vga_adx_find_keys_workspace_bytes(r._h, 7, 9) == 0 and f.vga_adx_find_keys_workspace_bytes(None, 7, 9) == 0
    s.close()
    r.close()
    assert f.vga_adx_write_keyed_device_v(None, None, None, None, 1, None, None, None, None) == ARG
    assert f.vga_adx_read_keyed_device_v(None, None, None, 1, None, None, None, None, None) == ARG
    assert f.vga_adx_find_keys_device_v(None, None, None, 1, 1, None, None, 0, None) == ARG
    assert AdxFileSet.find_items([]) == []
    count = C.c_int64()
    assert f.vga_adx_find_keys_items_for(None, 2, None, None, 0, C.byref(count)) == ARG
    info = kc.table()["infos"][0]
    ptrs, items = (C.c_void_p * 1)(C.addressof(info)), (_lib.AdxFindKeysItemC * 1)()
    assert f.vga_adx_find_keys_items_for(ptrs, 1, None, items, 0, C.byref(count)) == ARG and count.value == 1


# ---------------------------------------------------------------- the search's work items and workspace against the model
def test_find_items_tile_every_slot_of_every_file_once():
    infos = kc.table()["infos"]
    for offs in (None, list(range(3, 3 + 2_000_000 * len(infos), 2_000_000))):
        items = [(i.file, i.first_slot, i.slot_count) for i in AdxFileSet.find_items(infos, offs)]
        assert items == kc.find_items_model(infos)
        per = {}
        for f, first, count in items:
            assert 0 < count <= kc.FIND_SPAN_SLOTS
            per.setdefault(f, []).append((first, first + count))
        for f, info in enumerate(infos):
            total = info.frame_count * info.channel_count
            if total:
                check_tiling(per[f], total, f)
            else:
                assert f not in per
    assert max(len(v) for v in per.values()) > 64                      # the file of 66 000 slots


# ---------------------------------------------------------------- the stand-alone driver
def small_write_set():
    return [kc.keyed_file(c, t) for c, t, _, _ in kc.FILES[:6]]


def small_infos():
    return kc.table()["infos"][:6]


def tiny_frame_infos():
    i = _lib.AdxFileInfoC()
    i.frame_size, i.channel_count, i.frame_count, i.audio_bytes, i.audio_offset, i.version, i.revision = 1, 2, 40, 40, 36, 3, 8
    return [small_infos()[0], i]


A, H, K, I, X, W = 0x10000, 0x20000, 0x30004, 0x40000, 0x50000, 0x60000     # audio, history, keys, images, index out, workspace


def the_calls():
    """set name -> [(what, six addresses, (n0, n1), bytes, code, a piece of the message)]"""
    need = kc.workspace_model(6, 3, 2)
    write_calls = [
        (WRITE, (A, H, K, I), (3, 0), 0, 0, ""),
        (WRITE, (A, H, K, I), (0, 0), 0, ARG, "0 keys"),
        (WRITE, (A, H, K, I), (-2, 0), 0, ARG, "-2 keys"),
        (WRITE, (A, H, 0, I), (3, 0), 0, ARG, "null d_keys"),
        (WRITE, (A, H, K, 0), (3, 0), 0, ARG, "null pointer"),
        (WRITE, (0, H, K, I), (3, 0), 0, ARG, "null pointer"),
        (WRITE, (A, 0, K, I), (3, 0), 0, ARG, "version 4 headers carry the channel histories"),
        (WRITE, (A + 4, H, K, I), (3, 0), 0, ARG, "16-byte alignment"),
        (WRITE, (A, H, K, I + 8), (3, 0), 0, ARG, "16-byte alignment"),
        (READ, (I, K, A), (3, 0), 0, OP, "not made from parsed headers"),
        (FIND, (I, K, X, W), (3, 2), need, OP, "not made from parsed headers"),
        (WORKSPACE, (), (3, 2), 0, 0, ""),
    ]
    read_calls = [
        (READ, (I, K, A), (3, 0), 0, 0, ""),
        (READ, (I + 16, K, A + 32), (1, 0), 0, 0, ""),
        (READ, (I, K, A), (0, 0), 0, ARG, "0 keys"),
        (READ, (I, K, A), (-1, 0), 0, ARG, "-1 keys"),
        (READ, (I, 0, A), (3, 0), 0, ARG, "null d_keys"),
        (READ, (0, K, A), (3, 0), 0, ARG, "null pointer"),
        (READ, (I, K, 0), (3, 0), 0, ARG, "null pointer"),
        (READ, (I + 1, K, A), (3, 0), 0, ARG, "16-byte alignment"),
        (READ, (I, K, A + 2), (3, 0), 0, ARG, "16-byte alignment"),
        (WRITE, (A, H, K, I), (3, 0), 0, OP, "made from parsed headers"),
        (FIND, (I, K, X, W), (3, 2), need, 0, ""),
        (FIND, (I, K, X, W), (3, 2), need + 100, 0, ""),
        (FIND, (I, 0, X, 0), (0, 0), 0, 0, ""),                        # no candidates: nothing to read, no workspace
        (FIND, (I, K, X, W), (-1, 2), need, ARG, "negative candidate count"),
        (FIND, (I, K, X, W), (3, -1), need, ARG, "negative candidate count"),
        (FIND, (I, 0, X, W), (3, 2), need, ARG, "null d_keys"),
        (FIND, (I, K, 0, W), (3, 2), need, ARG, "null d_key_index_out"),
        (FIND, (0, K, X, W), (3, 2), need, ARG, "null pointer"),
        (FIND, (I + 4, K, X, W), (3, 2), need, ARG, "16-byte alignment"),
        (FIND, (I, K, X, W), (3, 2), need - 1, ARG, "the workspace needs %d bytes" % need),
        (FIND, (I, K, X, 0), (3, 2), need, ARG, "the workspace needs %d bytes" % need),
        (FIND, (I, K, X, W + 2), (3, 2), need, ARG, "the workspace needs %d bytes" % need),
        (WORKSPACE, (), (3, 2), 0, 0, ""),
        (WORKSPACE, (), (0, 0), 0, 0, ""),
        (WORKSPACE, (), (32, 1), 0, 0, ""),
        (WORKSPACE, (), (-1, 4), 0, 0, ""),
        (ITEMS, (), (0, 0), 0, 0, ""),
    ]
    tiny_calls = [
        (READ, (I, K, A), (3, 0), 0, ARG, "1-byte frames"),
        (FIND, (I, K, X, W), (3, 2), 64, ARG, "1-byte frames"),
    ]
    return {"write": write_calls, "read": read_calls, "tiny": tiny_calls}


LCG_CHECKS = [1 << 15, 1 << 16, (1 << 27) - 1, (1 << 31) - 1]
LCG_PAIRS = [(0, 0), (1, 1), (255, 1), (32767, 32769), (70000, 12345), ((1 << 27) - 1, 1 << 16), ((1 << 30), (1 << 30) - 1)]


def write_cases(path):
    sets = {"write": (0, small_write_set()), "read": (1, small_infos()), "tiny": (1, tiny_frame_infos())}
    calls = the_calls()
    with open(path, "wb") as f:
        keys = list(kc.KEYS.values())
        f.write(struct.pack("<i", len(keys)) + b"".join(struct.pack("<3i", *k) for k in keys))
        f.write(struct.pack("<i%dq" % len(LCG_CHECKS), len(LCG_CHECKS), *LCG_CHECKS))
        f.write(struct.pack("<i", len(LCG_PAIRS)) + b"".join(struct.pack("<2q", *p) for p in LCG_PAIRS))
        f.write(struct.pack("<i", len(sets)))
        for name in ("write", "read", "tiny"):
            kind, files = sets[name]
            f.write(struct.pack("<3i", kind, len(files), 0))
            for x in files:
                if kind == 0:
                    f.write(struct.pack("<13i", x.channels, *[getattr(x.params, k) for k, _ in x.params._fields_]))
                else:
                    f.write(struct.pack("<7i", x.channel_count, x.frame_size, x.frame_count, x.audio_bytes, x.audio_offset, x.version, x.revision))
            f.write(struct.pack("<i", len(calls[name])))
            for what, addresses, n, nbytes, _, _ in calls[name]:
                a = list(addresses) + [0] * (6 - len(addresses))
                f.write(struct.pack("<i6q2iq", what, *a, n[0], n[1], nbytes))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers, computed once: {"lcg": (jump mismatches, compose mismatches), set name: [answers]}"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("adx_keyed_files_host")
    exe = str(tmp / "adx_keyed_files_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    write_cases(tmp / "cases.bin")
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "3 ok", r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rd = Reader(open(tmp / "results.bin", "rb").read())
    out = {"lcg": tuple(rd.take("2q"))}
    for name in ("write", "read", "tiny"):
        assert rd.take("i") == [0], name
        answers = []
        for what, _, _, _, _, _ in the_calls()[name]:
            rc, n = rd.take("2i")
            msg = rd.d[rd.at:rd.at + n].decode()
            rd.at += n
            extra = None
            if what == WORKSPACE:
                extra = rd.take("q")[0]
            elif what == ITEMS:
                count = rd.take("i")[0]
                extra = [tuple(rd.take("3i")) for _ in range(count)]
            answers.append((rc, msg, extra))
        out[name] = answers
    assert rd.at == len(rd.d)
    return out


def test_the_jump_is_serial_stepping(driver):
    """adx_lcg.hpp for every key of the table (an even multiplier, multiplier 0 and increment 0 among them): k = 0 .. 70 000 and
    2^15, 2^16, 2^27 - 1, 2^31 - 1; power(a + b) == power(a) then power(b)"""
    assert {0x4E36, 0} <= {k[1] for k in kc.KEYS.values()} and 0 in {k[2] for k in kc.KEYS.values()}
    assert driver["lcg"] == (0, 0)


def test_every_refusal_has_its_code_and_message(driver):
    for name, calls in the_calls().items():
        for (what, addresses, n, nbytes, code, piece), (rc, msg, extra) in zip(calls, driver[name]):
            assert rc == code, (name, what, addresses, n, rc, msg)
            if code:
                assert piece in msg and msg.startswith(("vga_adx_write_keyed_device_v: ", "vga_adx_read_keyed_device_v: ",
                                                        "vga_adx_find_keys_device_v: ")[what]), (name, what, msg)


def test_workspace_size_and_items_are_the_models(driver):
    sizes = [(n, extra) for (what, _, n, _, _, _), (_, _, extra) in zip(the_calls()["read"], driver["read"]) if what == WORKSPACE]
    assert len(sizes) == 4
    for (n8, n9), got in sizes:
        assert got == (kc.workspace_model(6, n8, n9) if n8 >= 0 else 0), (n8, n9, got)
    assert kc.workspace_model(6, 32, 1) == 6 * 8
    assert [e for (w, _, _, _, _, _), (_, _, e) in zip(the_calls()["write"], driver["write"]) if w == WORKSPACE] == [0]
    items = next(e for (w, _, _, _, _, _), (_, _, e) in zip(the_calls()["read"], driver["read"]) if w == ITEMS)
    assert items == kc.find_items_model(small_infos())
    assert items == [(i.file, i.first_slot, i.slot_count) for i in AdxFileSet.find_items(small_infos())]


# ---------------------------------------------------------------- the case table holds what it is for
def test_the_table_is_the_oracles_own():
    t = kc.table()
    types = [f.params.encryption_type for f in t["files"]]
    assert {0, 5, 8, 9} == set(types) and {f.params.frame_size for f in t["files"]} >= {18, 19, 36, 255}
    assert max(i.frame_count * i.channel_count for i in t["infos"]) > 1 << 16
    # reading a keyed image and decrypting returns what was written (up to what the file kept; type 9 masks the first byte)
    checked = 0
    for f, rows, dec, info in zip(t["files"], t["rows"], t["dec_rows"], t["infos"]):
        keep = min(info.audio_bytes, len(rows[0]))
        for a, b in zip(rows, dec):
            want = np.array(a[:keep], copy=True)
            if info.revision == 9:
                fs = info.frame_size
                frames = want[:keep // fs * fs].reshape(-1, fs)
                frames[frames.any(axis=1), 0] &= 0x1F
            assert np.array_equal(b[:keep], want)
            checked += keep
    assert checked > 1_000_000
    # the second oracle (pure Python) on the small files: the same images' audio, the same answers of the search
    for n, (f, rows, enc, info) in enumerate(zip(t["files"], t["rows"], t["enc_rows"], t["infos"])):
        if info.audio_bytes * info.channel_count > 4000 or info.audio_bytes == 0:
            continue
        key = po.AdxKey(*kc.KEYS[kc.FILES[n][2]])
        keep = min(info.audio_bytes, len(rows[0]))
        for c, row in enumerate(rows):
            mine = bytearray(row.tobytes())
            pycrypt.adx_crypt_channel(mine, key, info.revision, info.frame_size, c, info.channel_count)
            assert bytes(mine[:keep]) == enc[c][:keep].tobytes(), (n, c)
        for name, (k8, k9) in kc.FIND_LISTS.items():
            sub, base = (k8, 0) if info.revision == 8 else (k9, len(k8))
            hits = [base + i for i, k in enumerate(sub) if info.revision and pycrypt.adx_test_key([bytes(e) for e in enc], po.AdxKey(*kc.KEYS[k]), info.revision, info.frame_size)]
            assert t["found"][name][n] == (hits[0] if hits else -1), (n, name)


def test_the_table_reaches_what_it_is_for():
    t = kc.table()
    found, names = t["found"], [k for _, _, k, _ in kc.FILES]
    fwd8, fwd9 = kc.FIND_LISTS["forward"]
    right = [(fwd8.index(k) if i.revision == 8 else len(fwd8) + fwd9.index(k)) if i.revision else -1 for k, i in zip(names, t["infos"])]
    # a wrong earlier candidate passes by chance: exactly the tiny file made for it, among possibly others
    chance = [n for n, (got, want) in enumerate(zip(found["forward"], right)) if got >= 0 and want >= 0 and got < want]
    one_frame = next(n for n, c in enumerate(kc.FILES) if c[3] == "one_frame")
    assert one_frame in chance and found["forward"][one_frame] == fwd8.index("twin")
    assert sum(kc.FILES[n][3] == "one_frame" for n in chance) == 1
    # the right key as last candidate, as first candidate, absent; an empty type-9 sub-list; type 0 is never searched
    last = [n for n, got in enumerate(found["forward"]) if got == len(fwd8) - 1 and names[n] == "plain"]
    assert last and all(found["reverse"][n] == 0 for n in last) and all(found["absent"][n] == -1 for n in last if kc.FILES[n][3] != "zeros")
    nines = [n for n, i in enumerate(t["infos"]) if i.revision not in (0, 8)]
    assert nines and all(found["empty9"][n] == -1 for n in nines) and any(found["forward"][n] >= len(fwd8) for n in nines)
    assert all(found[name][n] == -1 for name in found for n, i in enumerate(t["infos"]) if i.revision == 0)
    zeros = next(n for n, c in enumerate(kc.FILES) if c[3] == "zeros")
    assert found["forward"][zeros] == 0 and found["reverse"][zeros] == 0 and found["absent"][zeros] == 0
    noise = [n for n, c in enumerate(kc.FILES) if c[3] == "noise" and c[0][1] > 10000]
    assert noise and all(found[name][n] == -1 for name in found for n in noise)
    # the slot-0 quirk shows: the oracle's image under a seed of 0x8000 or above differs from the one under the masked seed
    n = next(n for n, c in enumerate(kc.FILES) if c[2] == "high_seed" and c[3] == "low" and len(t["rows"][n][0]))
    seed, mult, inc = kc.KEYS["high_seed"]
    assert seed >= 0x8000
    f = t["files"][n]
    masked = po.adx_crypt(t["rows"][n], po.AdxKey(seed & 0x7FFF, mult, inc), f.params.encryption_type, f.params.frame_size)
    raw = po.adx_crypt(t["rows"][n], po.AdxKey(seed, mult, inc), f.params.encryption_type, f.params.frame_size)
    assert raw[0][0] != masked[0][0] and np.array_equal(raw[0][1:], masked[0][1:])
    # the key indices of the write and read tests: valid, -1 and == nkeys all occur
    mixed = kc.key_index_sets()["mixed"]
    assert -1 in mixed and len(kc.ALL_KEYS) in mixed and any(0 <= i < len(kc.ALL_KEYS) for i in mixed)
    # hand-made holes lie where they matter: slot 0, both sides of a span boundary, both sides of a chunk of the search
    holes = next(n for n, c in enumerate(kc.FILES) if c[3] == "holes" and c[0][0] == 2 and c[0][1] < 100000)
    empty, zero_scale = kc.hole_slots(t["files"][holes])
    span = 448 * 2
    assert {0, span - 1, span, kc.FIND_SPAN_SLOTS - 1, kc.FIND_SPAN_SLOTS} <= set(empty) and zero_scale
