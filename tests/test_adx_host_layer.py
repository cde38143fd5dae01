"""The HIP-free CRI ADX host layer (vgaudio_amd/csrc/adx_host.hpp) on its own: tests/host/adx_host_driver.cpp includes the
header with a set_error of its own and is built twice with g++.  As a shared library its results are compared with the
loaded product library's, with the oracle and oracle.pyref, and with what the parent of the change that filled the header
answered (tests/adx_host_cases.py -> tests/golden/adx_host_refusals.json: the codes and messages of refused calls, the
encoded sizes and the conversions); as a stand-alone program under AddressSanitizer and UBSan it runs the same tables from a
file, as a child process, every array a heap block of exactly its size.  CPU only: no call here passes every argument test
of an entry point that goes on to the device."""
import ctypes as C
import json
import math
import os
import platform
import re
import shutil
import struct
import subprocess

import pytest

import adx_host_cases as T
from oracle import pyoracle as po
from oracle.pyref import criadx as pyref
from vgaudio_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "vgaudio_amd", "csrc")
SRC = os.path.join(HERE, "host", "adx_host_driver.cpp")
DEPS = [SRC, os.path.join(CSRC, "adx_host.hpp")]
SO = os.path.join(HERE, "host", "libadx_host_driver.so")
# as the product is built (vgaudio_amd/build.py): C# int arithmetic wraps, nothing contracts into an FMA
FLAGS = ["-std=c++17", "-Wall", "-fwrapv", "-ffp-contract=off", "-fno-fast-math"]
RECORDED = json.load(open(T.RECORD))

SAMPLE_RATES = [1, 8000, 22050, 44100, 48000, 96000]
CEIL_VALUES = sorted(set(range(-70, 71)) | {2**31 - 1 - k for k in range(71)} | {-2**31 + k for k in range(71)})
CEIL_DIVISORS = [4, 32, 64, 504]


def highpasses(rate):
    return [0, 1, 500, rate // 2]


@pytest.fixture(scope="module")
def host():
    """the driver as a shared library, built when it is older than its sources"""
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.run(["g++", "-O2", "-fPIC", "-shared"] + FLAGS + [SRC, "-o", SO], check=True)
    L = C.CDLL(SO)
    for name in T.CONVERSIONS:
        getattr(L, name.replace("vga_adx_", "ah_")).argtypes = [C.c_int, C.c_int]
    L.ah_divide_by_round_up.argtypes = [C.c_int, C.c_int]
    L.ah_encoded_byte_count.argtypes = L.ah_own_frames.argtypes = [C.c_int, C.c_void_p]
    L.ah_encoded_bytes.argtypes = L.ah_decode_bytes_read.argtypes = [C.c_int, C.c_void_p]
    L.ah_encoded_bytes.restype = L.ah_decode_bytes_read.restype = C.c_longlong
    L.ah_device_coefs.argtypes = [C.c_void_p, C.c_int]
    L.ah_figures.argtypes, L.ah_figures.restype = [C.POINTER(C.c_int)], None
    return L


def packed(c0, c1):
    """two int16 coefficients as ah_device_coefs returns them"""
    v = (int(c0) & 0xFFFF) | ((int(c1) & 0xFFFF) << 16)
    return v - 2**32 if v >= 2**31 else v


# ---------------------------------------------------------------- coefficients and the kernels' parameters
def test_coefficients_equal_the_product_librarys_the_oracles_and_pyrefs(host):
    for rate in SAMPLE_RATES:
        for highpass in highpasses(rate):
            mine, product = (C.c_int16 * 2)(), (C.c_int16 * 2)()
            assert host.ah_calculate_coefficients(highpass, rate, mine) == 0
            assert _lib.lib().vga_adx_calculate_coefficients(highpass, rate, product) == 0
            want = [int(v) for v in po.adx_calculate_coefficients(highpass, rate)]
            assert list(mine) == list(product) == want == [int(v) for v in pyref.calculate_coefficients(highpass, rate)], (highpass, rate)
    assert list(mine) != [0, 0]


def test_device_parameters_resolve_the_coefficients_once(host):
    """Fixed: Coefs[Filter] (CriAdxCodec.cs:186-191); else the encoder's 500 Hz and the decoder's own high-pass"""
    fixed = [(0, 0), (0x0F00, 0), (0x1CC0, 0xF300 - 0x10000), (0x1880, 0xF240 - 0x10000)]
    for f, (c0, c1) in enumerate(fixed):
        p = T.params_struct(dict(type=2, filter=f, sample_rate=0, history=-3, padding=7))
        assert host.ah_device_coefs(C.byref(p), 1) == host.ah_device_coefs(C.byref(p), 0) == packed(c0, c1), f
    for rate in SAMPLE_RATES:
        for highpass in highpasses(rate):
            for kind in (3, 4):
                p = T.params_struct(dict(type=kind, filter=2, sample_rate=rate, highpass_frequency=highpass, history=99))
                assert host.ah_device_coefs(C.byref(p), 1) == packed(*po.adx_calculate_coefficients(500, rate)), (rate, highpass)
                assert host.ah_device_coefs(C.byref(p), 0) == packed(*po.adx_calculate_coefficients(highpass, rate)), (rate, highpass)


# ---------------------------------------------------------------- conversions and sizes
def test_the_three_conversions_equal_the_product_librarys_the_oracles_and_the_parents(host):
    assert 0 in T.CONVERSION_INPUTS and 4097 in T.CONVERSION_INPUTS and 2**31 - 1 in T.CONVERSION_INPUTS
    for name in T.CONVERSIONS:
        mine, product = getattr(host, name.replace("vga_adx_", "ah_")), getattr(_lib.lib(), name)
        oracle = getattr(po.lib(), name.replace("vga_adx_", "vgo_adx_"))
        for fs in T.CONVERSION_FRAME_SIZES:
            want = RECORDED["conversions"]["%s/%d" % (name, fs)]
            assert len(want) == len(T.CONVERSION_INPUTS)
            assert [mine(n, fs) for n in T.CONVERSION_INPUTS] == want == [product(n, fs) for n in T.CONVERSION_INPUTS], (name, fs)
            # (near 2**31 an intermediate nibble count wraps: the oracle is not built to wrap)
            assert [oracle(n, fs) for n in range(4098)] == want[:4098], (name, fs)
            if name.endswith("sample_count_to_byte_count"):
                assert [pyref.sample_count_to_byte_count(n, fs) for n in range(4098)] == want[:4098], fs


def test_the_ceiling_is_math_ceil_for_every_int(host):
    """Extensions.cs:145 in integers: a wrapped, negative sum rounds towards zero, where v / d + (v % d != 0) would not"""
    assert 2**31 - 1 in CEIL_VALUES and -2**31 in CEIL_VALUES
    for d in CEIL_DIVISORS:
        for v in CEIL_VALUES:
            assert host.ah_divide_by_round_up(v, d) == math.ceil(v / d), (v, d)      # (exact: |v| < 2**53)
    assert host.ah_divide_by_round_up(-7, 2) == -3


def test_encoded_sizes_equal_the_product_librarys_the_oracles_and_the_parents(host):
    assert set(RECORDED["encoded_byte_count"]) == set(T.SIZE_SETS)
    for name, (_, fields) in T.SIZE_SETS.items():
        want = RECORDED["encoded_byte_count"][name]
        assert T.sizes_of(host.ah_encoded_byte_count, fields) == want == T.sizes_of(_lib.lib().vga_adx_encoded_byte_count, fields), name
        p, q = T.params_struct(fields), po.adx_params(**fields)
        spf = (p.frame_size - 2) * 2
        for n, size in zip(T.SIZE_LENGTHS, want):
            fits = n + p.padding < 2**31 and (n + p.padding + spf - 1) // spf * p.frame_size < 2**31
            # the int64 size of the ragged layout is the same number wherever the reference's ints do not wrap ...
            assert (host.ah_encoded_bytes(n, C.byref(p)) == size) == fits, (name, n)
            assert host.ah_encoded_bytes(n, C.byref(p)) == (n + p.padding + spf - 1) // spf * p.frame_size
            if fits:                                                                 # ... and there the oracle's too
                assert po.lib().vgo_adx_encoded_size(n, C.byref(q)) == size, (name, n)
    wrapped = RECORDED["encoded_byte_count"]["padding_wraps"]
    # the sum 2**31 - 1 is the last that does not wrap; then it is -2**31, -2**31 + 1, ... and the ceiling rounds towards zero
    assert wrapped[99:102] == [2**26 * 18, -2**26 * 18, -(2**26 - 1) * 18]


def test_decode_reads_and_own_frames(host):
    for fields in ({}, dict(padding=10), dict(padding=40), dict(frame_size=34, padding=100), dict(frame_size=4, padding=3), dict(frame_size=254)):
        p = T.params_struct(fields)
        spf = (p.frame_size - 2) * 2
        for n in list(range(0, 200)) + [4097, 2**31 - 1]:
            assert host.ah_decode_bytes_read(n, C.byref(p)) == (p.padding // spf + (n + spf - 1) // spf) * p.frame_size, (fields, n)
            if n + p.padding < 2**31:
                assert host.ah_own_frames(n, C.byref(p)) == (n + p.padding + 31) // 32, (fields, n)
    assert T.reads(1000, T.PAD40) == host.ah_decode_bytes_read(1000, C.byref(T.params_struct(dict(padding=40)))) == 594


# ---------------------------------------------------------------- the order of argument tests
@pytest.mark.parametrize("name", sorted(T.REFUSED_CALLS))
def test_refused_calls_keep_the_parents_code_and_message(host, name):
    """in the product library and in the header's checks alone"""
    want = RECORDED["refusals"][name]
    assert want[0] not in (0, _lib.VGA_ERR_DEVICE)             # no case is one that passes all checks
    fn, args = T.REFUSED_CALLS[name]
    assert list(T.call(_lib.lib(), "vga_adx_", _lib.SIGNATURES, fn, args)) == want
    assert list(T.call(host, "ah_", _lib.SIGNATURES, fn, args)) == want


@pytest.mark.parametrize("name", sorted(T.ACCEPTED_CALLS))
def test_accepted_calls_pass_the_headers_checks(host, name):
    fn, args = T.ACCEPTED_CALLS[name]
    assert T.call(host, "ah_", _lib.SIGNATURES, fn, args) == (0, T.KNOWN_MESSAGE)


def test_the_tables_cover_the_entry_points_and_their_branches():
    names = set(T.REFUSED_CALLS)
    assert set(RECORDED["refusals"]) == names
    assert {fn for fn, _ in T.REFUSED_CALLS.values()} == set(T.ENTRY_POINTS) and len(T.ENTRY_POINTS) == 8
    assert {fn for fn, _ in T.ACCEPTED_CALLS.values()} == set(T.ENTRY_POINTS[2:])
    for prefix in ("size/", "encode_device/", "decode_device/", "encode_batch/", "decode_batch/", "encode_v/channel_1_", "decode_v/channel_1_"):
        assert {prefix + k for k in T.BAD} <= names, prefix                          # every branch of validate
    messages = {name: m for name, (_, m) in RECORDED["refusals"].items()}
    # validate's branches tell themselves apart (the two bad sample rates share a text; the null pointer has its own)
    assert len({messages["size/" + k] for k in list(T.BAD) + ["null_params"]}) == len(T.BAD)
    assert len(set(messages.values())) >= 35
    for prefix in ("size/", "encode_device/", "decode_device/", "encode_batch/", "decode_batch/", "encode_v/", "decode_v/"):
        assert sum(n.startswith(prefix) and ("_and_" in n or "two_bad" in n) for n in names) >= 4, prefix   # calls with two faults
    assert sum(n.startswith("coefs/") and "_and_" in n for n in names) == 2          # (its one test has one pair of faults)
    for word in ("one_byte_short", "null_out_row_last", "empty_pcm"):
        assert sum(word in n for n in names) >= 3, word
    assert sum("exactly_long_enough" in n for n in T.ACCEPTED_CALLS) >= 6 and sum("empty_pcm" in n for n in T.ACCEPTED_CALLS) >= 6
    # a bad channel that is not the first, in both ragged calls
    assert messages["encode_v/channel_2_empty_pcm_of_its_own_version"].startswith("channel 2: ")
    assert messages["decode_v/channel_2_one_byte_short_with_padding"].startswith("channel 2: ")


# ---------------------------------------------------------------- one copy of every figure and formula
def csrc(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_piece_figures_have_one_copy(host):
    figures = (C.c_int * 8)()
    host.ah_figures(figures)
    assert list(figures) == [2, 2560, 64, 1, 512, 8, 2, 32]    # (tests/test_adx_ragged_device_host.py: the model's)
    kernels = csrc("adx_kernels.hip")
    assert "ADX_DIRECT_MIN_PIECE_FRAMES" not in kernels and "ADX_DIRECT_WAVES_PER_SIMD" not in kernels
    plans = re.findall(r"plan_pieces\(([^;]*)\);", kernels)
    assert len(plans) == 2
    for arguments, side in zip(plans, ("ENCODE", "DECODE")):
        assert not re.search(r"(?<![\w.])(2560|512|64|8|2)\s*(,|\)|$)", arguments), arguments   # no literal piece argument
        assert [a.strip() for a in arguments.split(",")][2:] == [side + "_MIN_PIECE_FRAMES", side + "_HOOK_FLOOR", "PIECE_ALIGN_FRAMES"]
        assert side + "_WAVES_PER_SIMD" in arguments
    assert not re.search(r"constexpr int (ENCODE|DECODE)_", kernels)


def test_formulas_refusals_and_the_status_tail_appear_once_in_csrc():
    sources = {f: csrc(f) for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    def files_with(pattern):
        return sorted(f for f, text in sources.items() if re.search(pattern, text))
    read_size = r"padding / spf\) \* [\w.\[\]]*frame_size \+"             # (the decoder kernels' first frame is half of it)
    assert files_with(read_size) == ["adx_host.hpp"] and len(re.findall(read_size, sources["adx_host.hpp"])) == 1
    # (the device-resident ragged call names its first empty channel in words of its own, capi_adx_ragged.hip)
    assert files_with(r"empty PCM: the reference reads pcm\[0\]") == ["adx_host.hpp"] and sources["adx_host.hpp"].count("the reference reads pcm[0]") == 1
    assert files_with(r"a frame names a filter") == ["adx_capi.hpp"] and sources["adx_capi.hpp"].count("a frame names a filter") == 1
    assert files_with(r"names predictor > 7") == ["gc_capi.hpp"]
    assert files_with(r"int run_status_job\(.*const char \*message\)") == ["host_batch.hpp"]
    assert files_with(r"struct AdxDeviceParams") == files_with(r"AdxDeviceParams make_device_params") == ["adx_host.hpp"]
    assert files_with(r"\{0x1CC0, ") == ["adx_host.hpp"]                          # (the table; the decoders' own is a chain of selects)
    assert "hip_runtime" not in sources["adx_host.hpp"].split("#pragma once")[1]
    for f in ("capi_adx.hip", "capi_adx_v.hip", "capi_adx_ragged.hip"):
        assert "memset(&d" not in sources[f] and "std::ceil" not in sources[f], f


# ---------------------------------------------------------------- the header alone under the sanitizers
CALL_IDS = {fn: i for i, fn in enumerate(T.ENTRY_POINTS + T.CONVERSIONS + ["ceil", "device_coefs"])}


def packed_arg(value):
    if isinstance(value, tuple):
        kind, items = value[0], value[1:]
        if kind == "rows":
            return struct.pack("<2i%dq" % len(items), 1, len(items), *[v or 0 for v in items])
        if kind == "ints":
            return struct.pack("<2i%di" % len(items), 2, len(items), *items)
        fields = [dict(T.DEFAULTS, **f) for f in items]
        return struct.pack("<2i", 3, len(items)) + b"".join(struct.pack("<8i", *[f[k] for k in T.FIELDS]) for f in fields)
    return struct.pack("<iq", 0, value or 0)


def packed_call(fn, want, message, args):
    raw = message.encode()
    return struct.pack("<3i", CALL_IDS[fn], want, len(raw)) + raw + struct.pack("<i", len(args)) + b"".join(packed_arg(a) for a in args)


def test_host_layer_under_address_and_ub_sanitizer(tmp_path):
    """the header alone, compiled for the host with AddressSanitizer and UBSan, over the refused calls (what the parent
    answered), the accepted ones, the recorded sizes and conversions, the ceilings and the coefficients; a child process"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    exe = str(tmp_path / "adx_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [SRC, "-o", exe], check=True)
    calls = [packed_call(fn, *RECORDED["refusals"][name], args) for name, (fn, args) in sorted(T.REFUSED_CALLS.items())]
    calls += [packed_call(fn, 0, "", args) for _, (fn, args) in sorted(T.ACCEPTED_CALLS.items())]
    for name, p in T.SIZE_SETS.items():
        calls += [packed_call("vga_adx_encoded_byte_count", want, "", [n, p]) for n, want in zip(T.SIZE_LENGTHS, RECORDED["encoded_byte_count"][name])]
    for name in T.CONVERSIONS:
        for fs in T.CONVERSION_FRAME_SIZES:
            calls += [packed_call(name, want, "", [n, fs]) for n, want in zip(T.CONVERSION_INPUTS, RECORDED["conversions"]["%s/%d" % (name, fs)])]
    calls += [packed_call("ceil", math.ceil(v / d), "", [v, d]) for d in CEIL_DIVISORS for v in CEIL_VALUES]
    for rate in SAMPLE_RATES:
        for highpass in highpasses(rate):
            want = packed(*po.adx_calculate_coefficients(highpass, rate))
            calls.append(packed_call("device_coefs", want, "", [T.P(sample_rate=rate, highpass_frequency=highpass), 0]))
            calls.append(packed_call("vga_adx_calculate_coefficients", 0, "", [highpass, rate, T.A]))
    calls += [packed_call("device_coefs", packed(*c), "", [T.P(type=2, filter=f), 1])
              for f, c in enumerate([(0, 0), (0x0F00, 0), (0x1CC0, 0xF300), (0x1880, 0xF240)])]
    path = tmp_path / "calls.bin"
    path.write_bytes(struct.pack("<i", len(calls)) + b"".join(calls))
    r = subprocess.run([setarch, platform.machine(), "-R", exe, "--calls", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(calls), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert len(calls) > 40000
