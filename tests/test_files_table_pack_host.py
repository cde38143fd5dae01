"""The host layer the nine "set of files on the device" objects share, without a GPU: the table pack
(vgaudio_amd/csrc/files_table_pack.hpp) on its own under AddressSanitizer and UBSan against a numpy model of its rules, and
what vgaudio_amd/csrc/files_object.hpp says for every object: the empty set, a null object in every call that writes or reads,
a null output in every create call.  The messages are the ones the C-ABI files held before the layer was shared."""
import ctypes as C
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

from vgaudio_amd import _lib
from vgaudio_amd.adx import AdxFileSet
from vgaudio_amd.dsp import DspFileSet
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.hca import HcaFileSet
from vgaudio_amd.hps import HpsFileSet
from vgaudio_amd.idsp import IdspFileSet
from vgaudio_amd.nwstm import NwFileSet, NwPcmFileSet
from vgaudio_amd.wave import WaveFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "host", "files_table_pack_driver.cpp")
ARG = _lib.VGA_ERR_ARGUMENT


# ---------------------------------------------------------------- the pack against a model
def table(size, count):
    return (0, size, count)


def raw(nbytes):
    return (1, 1, nbytes)


CASES = {                                                    # name -> parts (raw, element size, element count)
    "no_parts": [],
    "one_empty_part": [table(4, 0)],
    "empty_first_last_and_between": [table(8, 0), table(4, 3), table(12, 0), table(2, 5), table(32, 0)],
    "element_sizes": [table(1, 3), table(2, 3), table(4, 3), table(8, 3), table(12, 3), table(32, 3)],
    "byte_sizes": [table(1, 1), table(1, 15), table(1, 16), table(1, 17), table(1, 4096)],
    "byte_sizes_of_wide_elements": [table(4, 4), table(8, 2), table(12, 1), table(2, 2048), table(32, 128)],
    "raw_between_tables": [table(12, 5), raw(40), table(8, 7)],
    "raw_sizes": [raw(0), table(4, 1), raw(1), raw(16), raw(17), table(2, 1)],
    "nine_parts": [table(32, 7), table(8, 11), table(4, 11), table(2, 11), table(12, 9), table(12, 0), table(12, 2), table(12, 1),
                   table(12, 30)],
}


def pattern(part, nbytes):
    return ((part * 37 + np.arange(nbytes, dtype=np.int64) * 11 + 1) & 0xFF).astype(np.uint8)


def model(parts):
    """(offsets, total, image): every part on the next multiple of 16 after the one before, 16 bytes of slack, zeros between"""
    offsets, at = [], 0
    for _, size, count in parts:
        offsets.append(at)
        at += (size * count + 15) // 16 * 16
    image = np.zeros(at + 16, np.uint8)
    for p, (_, size, count) in enumerate(parts):
        image[offsets[p]:offsets[p] + size * count] = pattern(p, size * count)
    return offsets, at + 16, image


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """name -> (offsets, bytes(), image) as the driver wrote them, every case in one run"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("files_table_pack")
    exe = str(tmp / "files_table_pack_driver")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    names = sorted(CASES)
    with open(tmp / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(names)))
        for name in names:
            f.write(struct.pack("<i", len(CASES[name])))
            for part in CASES[name]:
                f.write(struct.pack("<3i", *part))
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(names), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr.strip(), r.stderr
    data, at, out = open(tmp / "results.bin", "rb").read(), 0, {}
    for name in names:
        n = struct.unpack_from("<i", data, at)[0]
        offsets = list(struct.unpack_from("<%dq" % n, data, at + 4))
        total, size = struct.unpack_from("<2q", data, at + 4 + 8 * n)
        at += 4 + 8 * n + 16
        out[name] = (offsets, total, np.frombuffer(data, np.uint8, size, at))
        at += size
    assert at == len(data)
    return out


def test_the_cases_hold_what_they_are_for():
    assert CASES["no_parts"] == [] and CASES["one_empty_part"][0][2] == 0
    parts = CASES["empty_first_last_and_between"]
    assert parts[0][2] == parts[2][2] == parts[-1][2] == 0 and parts[1][2] and parts[3][2]
    assert [p[1] for p in CASES["element_sizes"]] == [1, 2, 4, 8, 12, 32]
    assert [p[1] * p[2] for p in CASES["byte_sizes"]] == [1, 15, 16, 17, 4096]
    assert {p[1] * p[2] for p in CASES["byte_sizes_of_wide_elements"]} == {16, 12, 4096}
    assert [p[0] for p in CASES["raw_between_tables"]] == [0, 1, 0] and len(CASES["nine_parts"]) == 9


@pytest.mark.parametrize("name", sorted(CASES))
def test_pack_is_the_model(driver, name):
    parts = CASES[name]
    offsets, total, image = driver[name]
    want_offsets, want_total, want_image = model(parts)
    assert len(offsets) == len(parts) and all(o % 16 == 0 for o in offsets)
    rooms = [(size * count + 15) // 16 * 16 for _, size, count in parts]
    assert total == sum(rooms) + 16 == len(image)
    for p in range(1, len(parts)):                                     # in the order of add, and disjoint
        assert offsets[p] == offsets[p - 1] + rooms[p - 1]
    assert offsets == want_offsets and total == want_total
    covered = np.zeros(total, bool)
    for o, (_, size, count) in zip(offsets, parts):
        assert not covered[o:o + size * count].any()
        covered[o:o + size * count] = True
    assert not image[~covered].any(), "padding and slack are zero"
    assert not covered[total - 16:].any()
    assert image.tobytes() == want_image.tobytes()
    if name == "no_parts":
        assert total == 16 and not image.any()
    if name == "one_empty_part":
        assert offsets == [0] and total == 16


# ---------------------------------------------------------------- the nine objects without a GPU
def L():
    return _lib.lib()


def last_error():
    L().vga_last_error.restype = C.c_char_p
    return L().vga_last_error().decode()


def null_arguments(name):
    """every pointer null, every number 0"""
    return [0 if t in (C.c_int, C.c_size_t) else None for t in _lib.SIGNATURES[name][1]]


EMPTY_SETS = {"vga_gc_files": DspFileSet, "vga_gc_aligned": AlignedFileSet, "vga_nw_files": NwFileSet, "vga_nw_pcm_files": NwPcmFileSet,
              "vga_hps_files": HpsFileSet, "vga_idsp_files": IdspFileSet, "vga_wave_files": WaveFileSet, "vga_adx_files": AdxFileSet,
              "vga_hca_files": HcaFileSet}


@pytest.mark.parametrize("kind", sorted(EMPTY_SETS))
def test_the_empty_set_creates_reports_nothing_and_destroys(kind):
    s = EMPTY_SETS[kind]([])
    assert s._h and s.totals.files == 0 and s.files == 0
    if hasattr(s.totals, "channels"):
        assert s.totals.channels == 0
    s.close()
    assert not s._h
    s.close()                                                          # a second close is nothing


NULL_OBJECT = {                                              # every call that writes or reads through an object -> what it says to none
    "vga_gcadpcm_build_channels_device_v": "vga_gcadpcm_build_channels_device_v: null vga_gc_files",
    "vga_dsp_write_device_v": "vga_dsp_write_device_v: null vga_gc_files",
    "vga_dsp_read_device_v": "vga_dsp_read_device_v: null vga_gc_files",
    "vga_gcadpcm_align_channels_device_v": "vga_gcadpcm_align_channels_device_v: null vga_gc_aligned",
    "vga_nwstm_write_device_v": "vga_nwstm_write_device_v: null vga_nw_files",
    "vga_nwstm_read_device_v": "vga_nwstm_read_device_v: null vga_nw_files",
    "vga_nwstm_pcm_write_device_v": "vga_nwstm_pcm_write_device_v: null vga_nw_pcm_files",
    "vga_nwstm_pcm_read_device_v": "vga_nwstm_pcm_read_device_v: null vga_nw_pcm_files",
    "vga_hps_write_device_v": "vga_hps_write_device_v: null vga_hps_files",
    "vga_hps_read_device_v": "vga_hps_read_device_v: null vga_hps_files",
    "vga_idsp_write_device_v": "vga_idsp_write_device_v: null vga_idsp_files",
    "vga_idsp_read_device_v": "vga_idsp_read_device_v: null vga_idsp_files",
    "vga_wave_write_device_v": "vga_wave_write_device_v: null vga_wave_files",
    "vga_wave_read_device_v": "vga_wave_read_device_v: null vga_wave_files",
    "vga_adx_write_device_v": "vga_adx_write_device_v: null vga_adx_files",
    "vga_adx_read_device_v": "vga_adx_read_device_v: null vga_adx_files",
    "vga_adx_write_keyed_device_v": "vga_adx_write_keyed_device_v: null vga_adx_files",
    "vga_adx_read_keyed_device_v": "vga_adx_read_keyed_device_v: null vga_adx_files",
    "vga_adx_find_keys_device_v": "vga_adx_find_keys_device_v: null vga_adx_files",
    "vga_hca_write_device_v": "vga_hca_write_device_v: null vga_hca_files",
    "vga_hca_read_device_v": "vga_hca_read_device_v: null vga_hca_files",
    "vga_hca_find_keys_device_v": "vga_hca_find_keys_device_v: null vga_hca_files",
    "vga_hca_read_keyed_device_v": "vga_hca_read_keyed_device_v: null vga_hca_files",
}


@pytest.mark.parametrize("call", sorted(NULL_OBJECT))
def test_a_null_object_is_refused_by_name(call):
    assert getattr(L(), call)(*null_arguments(call)) == ARG
    assert last_error() == NULL_OBJECT[call]


CREATE_CALLS = ["vga_gc_files_create", "vga_gc_files_create_from_dsp", "vga_gc_aligned_create", "vga_nw_files_create",
                "vga_nw_files_create_from_infos", "vga_nw_pcm_files_create", "vga_nw_pcm_files_create_from_infos", "vga_hps_files_create",
                "vga_hps_files_create_from_infos", "vga_idsp_files_create", "vga_idsp_files_create_from_infos", "vga_wave_files_create",
                "vga_wave_files_create_from_infos", "vga_adx_files_create", "vga_adx_files_create_from_infos", "vga_hca_files_create",
                "vga_hca_files_create_from_infos"]


@pytest.mark.parametrize("call", CREATE_CALLS)
def test_a_null_output_is_refused_before_anything_else(call):
    assert getattr(L(), call)(*null_arguments(call)) == ARG
    assert last_error() == "null output"


def test_every_create_call_of_the_library_is_covered():
    creates = sorted(n for n in _lib.SIGNATURES if any(n.startswith(k + "_create") for k in EMPTY_SETS))
    assert creates == sorted(CREATE_CALLS)
