"""include/vgaudio_hip/adx_ragged.h without a GPU: the header's functions are exported and in the ctypes table with the header's
argument counts (the header lies outside the directory listing tests/test_abi_exports.py reads, so the same regexes are pointed
at it here), the packed layout (vga_adx_ragged_layout_for is host code) against a model written here, the workspace cap, what
is refused, that the GPU file's table of cases names every function the header declares, and the HIP-free host layer
(vgaudio_amd/csrc/adx_host.hpp: layout, work slots, pieces, item table) on its own under AddressSanitizer and UBSan."""
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

from vgaudio_amd import _lib
from vgaudio_amd.criadx import RaggedAdx, RaggedAdxTotalsC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "adx_ragged.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_adx_ragged_device.py")
DRIVER = os.path.join(ROOT, "tests", "host", "adx_host_driver.cpp")

NAMES = ["vga_adx_ragged_layout_for", "vga_adx_ragged_create", "vga_adx_ragged_destroy", "vga_adx_ragged_channels",
         "vga_adx_ragged_totals_of", "vga_adx_ragged_offsets", "vga_adx_encode_device_v", "vga_adx_decode_device_v"]
HOOK = "vga_testing_adx_ragged_stats"


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


def params(**kw):
    p = _lib.AdxParams()
    L().vga_adx_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


PARAM_SETS = {
    "default": {},
    "version3": {"version": 3},
    "exponential": {"type": 4},
    "fixed1": {"type": 2, "filter": 1},
    "frame34": {"frame_size": 34},
    "padding10": {"padding": 10, "history": 77},
    "padding40": {"padding": 40, "history": -5},
}
EDGE_LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65]


def seeded_lengths(seed, count=150, high=40000):
    rng = np.random.default_rng(seed)
    more = [int(v) for v in rng.integers(1, high, count)]
    more[7] = more[3]                                                  # a tie: the sort is stable
    more.insert(20, 0)
    return EDGE_LENGTHS + more


# ---------------------------------------------------------------- the model
def cut_pieces(frames, want, min_frames, hook_floor, align, hook):
    segments = max(min(want, frames // min_frames), 1)
    segments = min(segments, 64)
    if hook > 0:
        segments = min(max(frames // hook_floor, 1), hook)
    segments = min(segments, 64)
    return segments, max(((frames + segments - 1) // segments + align - 1) // align * align, align)


def model(p, lengths, cus=256, hook=0):
    spf = (p.frame_size - 2) * 2
    frames = [(n + p.padding + spf - 1) // spf for n in lengths]
    m = {"frames": frames, "pcm_off": [], "adx_off": []}
    pcm_at = adx_at = 0
    for n, f in zip(lengths, frames):
        m["pcm_off"].append(pcm_at)
        m["adx_off"].append(adx_at)
        pcm_at += (n + 7) // 8 * 8
        adx_at += (f * p.frame_size + 15) // 16 * 16
    m["pcm_samples"], m["adx_bytes"], m["total_frames"] = pcm_at + 128, adx_at + 256, sum(frames)
    order = sorted(range(len(lengths)), key=lambda c: -lengths[c])       # (Python's sort is stable)
    m["order"] = order
    gf = [frames[order[g]] for g in range(0, len(lengths), 64)]
    m["group_frames"], slots = gf, 64 * len(gf)
    m["slots"] = slots
    m["time_pieces"] = p.frame_size == 18 and p.padding == 0
    scratch = m["time_pieces"] and len(lengths) > 0
    m["encode_ws"] = slots * (4 * 64 + 4 + 8 * 63) + 16 + 8 * 64 * sum(gf) if scratch else 0
    m["decode_ws"] = slots * 4 * 64 + 16 + 1024 if scratch else 0
    for name, waves, least, floor in (("enc", 2, 2560, 64), ("dec", 1, 512, 8)):
        if not gf:
            m[name] = (1, 2, [])
            continue
        # waves wanted / groups, the groups counted by the frames they hold (= len(gf) when all lengths are equal)
        want = min(64, cus * 4 * waves * gf[0] // sum(gf) if gf[0] else cus * 4 * waves // len(gf))
        segments, seg = cut_pieces(gf[0], want, least, floor, 2, hook if m["time_pieces"] else 1)
        items = [(g, k) for g in range(len(gf)) for k in range(segments) if k * seg < gf[g]]
        m[name] = (segments, seg, items)
    return m


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
    assert hook[HOOK] == len(_lib.SIGNATURES[HOOK][1]) == 3
    assert hasattr(lib, HOOK)
    v = (C.c_longlong * 10)()
    assert L().vga_testing_adx_ragged_stats(None, v, 10) == 10      # host state only: needs neither an object nor a GPU


def test_the_new_names_are_declared_in_the_new_header_only():
    inc = os.path.join(ROOT, "include")
    for f in sorted(os.listdir(inc)):
        if f.endswith(".h"):
            names = _declared(os.path.join(inc, f))
            assert not [n for n in NAMES if n in names], f
            assert "vga_adx_ragged" not in _strip(open(os.path.join(inc, f)).read()).replace(HOOK, ""), f
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
    for name in ("vga_adx_encode_device_v", "vga_adx_decode_device_v"):
        assert {"test_bytes_do_not_depend_on_poison", "test_round_trip_on_a_busy_stream_and_two_streams_at_once",
                "test_refused_layouts_launch_nothing"} <= set(cases[name])
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout
@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_layout_offsets_alignments_and_totals(name):
    p = params(**PARAM_SETS[name])
    lengths = seeded_lengths(50 + len(name))
    assert lengths.count(0) >= 2
    po, ao, tot = RaggedAdx.layout(p, lengths)
    m = model(p, lengths)
    assert len(po) == len(ao) == tot.channels == len(lengths)
    pcm_end = adx_end = 0
    for c, n in enumerate(lengths):                                   # ascending in the caller's order, no overlap
        nbytes = L().vga_adx_encoded_byte_count(n, C.byref(p))
        assert nbytes == m["frames"][c] * p.frame_size
        assert po[c] == pcm_end and po[c] % 8 == 0 and ao[c] == adx_end and ao[c] % 16 == 0, c
        pcm_end += (n + 7) // 8 * 8
        adx_end += (nbytes + 15) // 16 * 16
        # the row covers what the decoder reads too
        spf = (p.frame_size - 2) * 2
        assert (p.padding // spf + (n + spf - 1) // spf) * p.frame_size <= nbytes or n == 0
    assert list(po) == m["pcm_off"] and list(ao) == m["adx_off"]
    assert tot.pcm_samples == pcm_end + 128 == m["pcm_samples"] and tot.adx_bytes == adx_end + 256 == m["adx_bytes"]
    assert tot.total_frames == m["total_frames"]
    assert (tot.encode_workspace_bytes, tot.decode_workspace_bytes) == (m["encode_ws"], m["decode_ws"])
    for c, n in enumerate(lengths[:-1]):                              # an empty row takes no room: its offset is the next one's
        if n == 0:
            assert po[c] == po[c + 1]
        if m["frames"][c] == 0:
            assert ao[c] == ao[c + 1]
    # outputs one at a time
    arr, i64p = (C.c_int * len(lengths))(*lengths), C.POINTER(C.c_int64)
    only, one = RaggedAdxTotalsC(), np.zeros(len(lengths), np.int64)
    f = L().vga_adx_ragged_layout_for
    assert f(C.byref(p), arr, len(lengths), None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(C.byref(p), arr, len(lengths), one.ctypes.data_as(i64p), None, None) == 0 and np.array_equal(one, po)
    assert f(C.byref(p), arr, len(lengths), None, one.ctypes.data_as(i64p), None) == 0 and np.array_equal(one, ao)


def test_layout_of_an_empty_batch():
    po, ao, tot = RaggedAdx.layout(params(), [])
    assert len(po) == len(ao) == 0
    assert (tot.pcm_samples, tot.adx_bytes, tot.channels, tot.total_frames) == (128, 256, 0, 0)
    assert (tot.encode_workspace_bytes, tot.decode_workspace_bytes) == (0, 0)
    # needs no GPU: an empty object is made, asked and destroyed on any machine
    r = RaggedAdx(params(), [])
    assert r.channels == 0 and r.totals.pcm_samples == 128
    assert L().vga_adx_encode_device_v(r._h, None, None, None, None, 0, None) == 0
    assert L().vga_adx_decode_device_v(r._h, None, None, None, 0, None, None) == 0
    r.close()


@pytest.mark.parametrize("name", ["default", "version3", "exponential", "fixed1"])
def test_workspace_is_proportional_to_the_batchs_own_frames(name):
    """section 2's cap: crumbs <= 8 bytes per launched lane-frame, the rest <= 16 bytes per (slot, piece) plus 4 KiB -- for any
    plan of up to 64 pieces; one 120 s file beside 10 000 short ones stays far from longest x channels"""
    p = params(**PARAM_SETS[name])
    for lengths in (seeded_lengths(3), [120 * 48000] + [48000] * 10000, [5], [0, 0, 7]):
        m = model(p, lengths)
        _, _, tot = RaggedAdx.layout(p, lengths)
        lane_frames, slots = 64 * sum(m["group_frames"]), m["slots"]
        assert tot.encode_workspace_bytes <= 8 * lane_frames + 16 * slots * 64 + 4096
        assert tot.decode_workspace_bytes <= 16 * slots * 64 + 4096
        assert tot.encode_workspace_bytes >= 8 * lane_frames                 # (the crumbs are there)
    big = [120 * 48000] + [48000] * 10000
    _, _, tot = RaggedAdx.layout(p, big)
    assert tot.encode_workspace_bytes < 8 * (max(big) // 32) * len(big) // 50


# ---------------------------------------------------------------- refusals
def test_null_pointers_negative_counts_and_bad_parameters_are_refused():
    tot, p = RaggedAdxTotalsC(), params()
    one = (C.c_int * 3)(5000, 100, 7)
    f = L().vga_adx_ragged_layout_for
    ARG = _lib.VGA_ERR_ARGUMENT
    assert f(None, one, 3, None, None, C.byref(tot)) == ARG
    assert f(C.byref(p), None, 3, None, None, C.byref(tot)) == ARG
    assert f(C.byref(p), one, -1, None, None, C.byref(tot)) == ARG
    assert f(C.byref(p), one, 3, None, None, None) == ARG
    with pytest.raises(_lib.ArgumentError, match="channel 1 "):
        RaggedAdx.layout(p, [5000, -1, 7])
    for bad in ({"frame_size": 17}, {"frame_size": 2}, {"type": 5}, {"type": 2, "filter": 4}, {"padding": -1}, {"sample_rate": 0}):
        q = params(**bad)
        want = L().vga_adx_encoded_byte_count(100, C.byref(q))
        assert want < 0
        assert f(C.byref(q), one, 3, None, None, C.byref(tot)) == want, bad
        out = C.c_void_p()
        assert L().vga_adx_ragged_create(C.byref(q), one, 3, C.byref(out)) == want and not out.value
    assert L().vga_adx_ragged_create(C.byref(p), one, 3, None) == ARG
    out = C.c_void_p()
    assert L().vga_adx_ragged_create(None, one, 3, C.byref(out)) == ARG and not out.value
    assert L().vga_adx_ragged_create(C.byref(p), one, -1, C.byref(out)) == ARG and not out.value
    assert L().vga_adx_ragged_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_adx_ragged_offsets(None, None, None) == ARG
    assert L().vga_adx_ragged_channels(None) == 0
    L().vga_adx_ragged_destroy(None)
    assert L().vga_adx_encode_device_v(None, None, None, None, None, 0, None) == ARG
    assert L().vga_adx_decode_device_v(None, None, None, None, 0, None, None) == ARG


# ---------------------------------------------------------------- the header alone under the sanitizers
def driver_cases():
    cases = []
    for name, kw in sorted(PARAM_SETS.items()):
        p = params(**kw)
        for lengths in ([], [0], [0, 0, 0], [7], EDGE_LENGTHS, [40000] * 70, seeded_lengths(9 + len(name)),
                        seeded_lengths(4, count=300, high=3_000_000)):
            for cus, hook in ((256, 0), (256, 12), (256, 40), (8, 0), (304, 200), (256, 1)):
                cases.append((p, lengths, cus, hook, 0))
    cases.append((params(), [5, -3], 256, 0, _lib.VGA_ERR_ARGUMENT))
    cases.append((params(frame_size=7), [5, 3], 256, 0, _lib.VGA_ERR_ARGUMENT))
    cases.append((params(type=2, filter=9), [5, 3], 256, 0, _lib.VGA_ERR_ARGUMENT))
    return cases


def test_model_plans_are_what_the_issue_states():
    """1250 frames under the hook: 12 pieces of 106 frames and 19 of 66 for the encoder; the decoder's floor is 8 frames"""
    lengths = [40000] + seeded_lengths(1, count=120, high=30000)
    assert model(params(), lengths, hook=12)["enc"][:2] == (12, 106)
    assert model(params(), lengths, hook=40)["enc"][:2] == (19, 66)
    assert model(params(), lengths, hook=40)["dec"][:2] == (40, 32)
    assert model(params(), lengths, hook=0)["enc"][:2] == (1, 1250)   # below the encoder's 2560 frames a piece: one piece
    assert model(params(), lengths, hook=0)["dec"][:2] == (2, 626)    # the decoder cuts at 512
    m = model(params(), lengths, hook=200)
    assert m["enc"][0] <= 64 and m["dec"][0] == 64
    for name in ("enc", "dec"):                                        # no item lies wholly behind its group's frames
        segments, seg, items = m[name]
        assert len(items) == sum((gf + seg - 1) // seg for gf in m["group_frames"]) and len(set(items)) == len(items)


def test_host_layer_under_address_and_ub_sanitizer(tmp_path):
    """vgaudio_amd/csrc/adx_host.hpp alone, compiled for the host with AddressSanitizer and UBSan: its layout, order, plan and
    item table over seeded cases must be the model's; a child process"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    exe = str(tmp_path / "adx_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases, path = driver_cases(), tmp_path / "cases.bin"
    good = items = 0
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for p, lengths, cus, hook, rc in cases:
            n = len(lengths)
            f.write(struct.pack("<8i", p.sample_rate, p.highpass_frequency, p.frame_size, p.version, p.history, p.padding, p.type, p.filter))
            f.write(struct.pack("<4i%di" % n, cus, hook, n, rc, *lengths))
            if rc:
                continue
            m = model(p, lengths, cus, hook)
            f.write(struct.pack("<%dq" % (2 * n), *m["pcm_off"], *m["adx_off"]))
            f.write(struct.pack("<5q", m["pcm_samples"], m["adx_bytes"], m["total_frames"], m["encode_ws"], m["decode_ws"]))
            f.write(struct.pack("<%di" % n, *m["order"]))
            for name in ("enc", "dec"):
                segments, seg, table = m[name]
                f.write(struct.pack("<3i%di" % (2 * len(table)), segments, seg, len(table), *[v for it in table for v in it]))
                items += len(table)
            good += 1
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert [int(v) for v in r.stdout.split()[:3]] == [good, len(cases) - good, items]
