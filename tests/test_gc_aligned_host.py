"""include/vgaudio_hip/gc_files_aligned.h without a GPU: the header's functions are exported and in the ctypes table with the
header's argument counts, vga_gc_aligned_layout_for (host code) against a model built from the per-file size call
(tests/gc_aligned_cases.py), the per-channel numbers against GcAdpcmAlignment.cs:29-39 computed in Python, the work tables,
every refusal with its file and its code, that the GPU file's table of cases names every function the header declares, the
gather's index arithmetic against the oracle's re-encode, and the HIP-free host layer (vgaudio_amd/csrc/gc_aligned_host.hpp)
on its own under AddressSanitizer and UBSan."""
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

import gc_aligned_cases as ga
from oracle import pyoracle as po
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vgaudio_hip", "gc_files_aligned.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_gc_aligned.py")
DRIVER = os.path.join(ROOT, "tests", "host", "gc_aligned_host_driver.cpp")

NAMES = ["vga_gc_aligned_layout_for", "vga_gc_aligned_create", "vga_gc_aligned_destroy", "vga_gc_aligned_totals_of", "vga_gc_aligned_offsets",
         "vga_gc_aligned_ragged_in", "vga_gc_aligned_ragged_out", "vga_gcadpcm_align_channels_device_v"]
ARG, RANGE, DATA, OP = _lib.VGA_ERR_ARGUMENT, -2, -3, -4
ROW_FIELDS = ["file", "tail_row", "bytes_to_keep", "samples_to_keep", "samples_to_encode", "head", "loop_start", "loop_length",
              "loop_start_aligned", "out_samples", "out_bytes", "spacing", "entries"]
ROW_OFFSETS = ["in_pcm_off", "in_adpcm_off", "out_pcm_off", "out_adpcm_off", "tail_pcm_off", "tail_adpcm_off", "seek_off"]


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
    return ga.files_of(ga.SET)


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
    for d, _, names in os.walk(inc):
        for f in sorted(names):
            path = os.path.join(d, f)
            if f.endswith(".h") and os.path.abspath(path) != os.path.abspath(HEADER):
                assert not [n for n in NAMES if n in _declared(path)], path


def test_the_gpu_files_table_names_every_function_of_the_header():
    tree = ast.parse(open(GPU_FILE).read())
    cases = next(ast.literal_eval(n.value) for n in tree.body
                 if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    assert sorted(cases) == sorted(_declared(HEADER))
    for name, users in cases.items():
        assert users and set(users) <= tests, (name, users)
    assert {"test_bytes_do_not_depend_on_poison", "test_call_on_a_busy_stream"} <= set(cases["vga_gcadpcm_align_channels_device_v"])
    source = open(GPU_FILE).read()
    assert "vga_testing_poison_allocations" in source and "_sleep" in source


# ---------------------------------------------------------------- the layout against the model
@pytest.mark.parametrize("which", ["set", "needs", "plain", "big"])
def test_layout_is_the_per_file_calls_packed(which):
    import gc_files_cases as gf
    tuples = {"set": ga.SET, "needs": ga.NEEDS, "plain": [f + (0,) for f in gf.FILES], "big": ga.SET + ga.BIG}[which]
    files = ga.files_of(tuples)
    fc, so, tot = AlignedFileSet.layout(files)
    m = ga.model(files)
    nch = sum(f.channels for f in files)
    assert (tot.files, tot.channels, tot.aligned_channels) == (len(files), nch, len(m["tail_counts"])) and len(so) == nch
    assert list(fc) == m["first_channel"] and list(so) == m["seek_off"]
    assert (tot.pcm_samples, tot.adpcm_bytes, tot.out_pcm_samples, tot.out_adpcm_bytes, tot.seek_shorts) == \
        (m["in_pcm_samples"], m["in_adpcm_bytes"], m["out_pcm_samples"], m["out_adpcm_bytes"], m["seek_shorts"])
    assert all(o % 8 == 0 for o in so)
    for c in range(nch - 1):                                           # a channel without entries takes no room
        if m["entries"][c] == 0:
            assert so[c] == so[c + 1]
    if which == "plain":                                               # nothing to encode: the plain decode is all a call can need
        assert tot.aligned_channels == 0 and tot.workspace_bytes == tot.pcm_samples * 2
        assert (tot.out_pcm_samples, tot.out_adpcm_bytes) == (tot.pcm_samples, tot.adpcm_bytes)
    else:                                                              # + the tail batch and at least the encoder's 1024 x 12 bytes per tail
        assert tot.workspace_bytes >= m["scratch_at"] + 1024 * 12 * tot.aligned_channels
    if which == "needs":
        assert tot.aligned_channels == tot.channels
    if which == "set":
        assert any(e == 0 for e in m["entries"]) and any(n == 0 for n in m["counts"])
        assert any(o < i for i, o in zip(m["counts"], m["out_counts"])) and any(o > i for i, o in zip(m["counts"], m["out_counts"]))
    # outputs one at a time
    arr, i64p = (_lib.GcFileC * len(files))(*files), C.POINTER(C.c_int64)
    f = L().vga_gc_aligned_layout_for
    only, one = _lib.GcAlignedTotalsC(), np.zeros(nch, np.int64)
    assert f(arr, len(files), None, None, C.byref(only)) == 0
    assert all(getattr(only, k) == getattr(tot, k) for k, _ in only._fields_)
    assert f(arr, len(files), None, one.ctypes.data_as(i64p), None) == 0 and np.array_equal(one, so)
    assert f(arr, len(files), None, None, None) == ARG


def test_the_two_piece_file_spans_two_encoder_pieces_and_the_default_multiple_one():
    """tests/gc_aligned_cases.py: TWO_PIECE_MULTIPLE is the smallest multiple whose tail the ragged encoder cuts in two"""
    m = ga.model(the_files())
    groups, work = -(-len(m["tail_counts"]) // 16), 0
    by_length = sorted(m["tail_counts"], reverse=True)
    for g in range(groups):
        work += -(-by_length[16 * g] // 14)
    out5 = (C.c_int * 5)()

    def pieces(samples):
        assert L().vga_testing_gc_plan_pieces(256, groups, -(-samples // 14), work, 1, out5) == 0
        return out5[0]

    assert max(m["tail_counts"]) == ga.TWO_PIECE_MULTIPLE + 12 == 14 * 2 * ga.MIN_PIECE_FRAMES - 13
    assert pieces(max(m["tail_counts"])) == 2 and pieces(max(m["tail_counts"]) - 1) == 1 and pieces(0x3800 + 11) == 1
    assert 0x3800 + 11 in m["tail_counts"]


def test_an_empty_set_needs_no_gpu():
    fc, so, tot = AlignedFileSet.layout([])
    assert len(fc) == len(so) == 0
    assert [getattr(tot, k) for k, _ in tot._fields_] == [0, 0, 0, 128, 256, 128, 256, 0, 0]
    s = AlignedFileSet([])
    assert s.files == s.channels == 0
    assert L().vga_gcadpcm_align_channels_device_v(s._h, None, None, None, None, None, None, None, None, 0, None) == 0
    s.close()


# ---------------------------------------------------------------- refusals: the file, the per-file call's own code
REFUSED = {                                                            # name -> (the file (put at index 3), the code)
    "channels0": ((0, 50, 0, 0, 0, 14, 0), ARG),
    "channels256": ((256, 50, 0, 0, 0, 14, 0), OP),
    "negative": ((1, -1, 0, 0, 0, 14, 0), RANGE),
    "inverted": ((2, 50, 1, 30, 20, 14, 4), RANGE),
    "negative_multiple": ((1, 50, 1, 1, 20, 14, -4), RANGE),
    "overflow": ((1, 2147483000, 1, 1, 2147483000, 0, 0x3800), RANGE),
    "zero_loop": ((2, 100, 1, 15, 15, 14, 4), OP),
    "loop_past_the_row": ((2, 50, 1, 15, 57, 14, 14), RANGE),
}


def per_file_codes():
    """what the per-file calls answer to the same mistakes"""
    out = {}
    for name in ("negative", "inverted", "negative_multiple", "overflow"):
        f, lay = ga.gc_file(*REFUSED[name][0]), _lib.GcChannelLayoutC()
        out[name] = L().vga_gcadpcm_channel_layout_for(C.byref(f.channel), C.byref(lay))
    # the zero-length loop is refused by the plan of vga_gcadpcm_build_channels_device, after its argument checks and before it
    # launches anything: the pointers are never followed
    f, fake = ga.gc_file(*REFUSED["zero_loop"][0]), 0x10000
    out["zero_loop"] = L().vga_gcadpcm_build_channels_device(fake, 64, fake, 2, C.byref(f.channel), fake, 64, None, 0, None, 0, None, fake, 1 << 20, None)
    return out


def test_per_file_codes_are_the_ones_the_table_states():
    codes = per_file_codes()
    assert codes == {"negative": RANGE, "inverted": RANGE, "negative_multiple": RANGE, "overflow": RANGE, "zero_loop": OP}
    assert all(REFUSED[k][1] == codes[k] for k in codes)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_name_their_file(name):
    bad, code = REFUSED[name]
    files = the_files()[:3] + [ga.gc_file(*bad)] + the_files()[3:5]
    for call in ("layout", "create"):
        with pytest.raises(_lib._EXC[code], match=r"file 3\b"):
            AlignedFileSet.layout(files) if call == "layout" else AlignedFileSet(files)
    arr, tot, out = (_lib.GcFileC * len(files))(*files), _lib.GcAlignedTotalsC(), C.c_void_p()
    assert L().vga_gc_aligned_layout_for(arr, len(files), None, None, C.byref(tot)) == code
    assert L().vga_gc_aligned_create(arr, len(files), C.byref(out)) == code and not out.value
    if name == "loop_past_the_row":                                    # without the need to align the same loop is a good file
        files[3].channel.loop_alignment_multiple = 0
        arr = (_lib.GcFileC * len(files))(*files)
        assert L().vga_gc_aligned_layout_for(arr, len(files), None, None, C.byref(tot)) == 0


def test_gc_files_still_refuses_what_this_header_takes():
    from vgaudio_amd.dsp import DspFileSet
    with pytest.raises(_lib.InvalidOperationError, match=r"file 0\b"):
        DspFileSet.layout(the_files(), None)
    assert AlignedFileSet.layout(the_files())[2].files == len(ga.SET)


def test_null_arguments():
    tot = _lib.GcAlignedTotalsC()
    assert L().vga_gc_aligned_layout_for(None, 2, None, None, C.byref(tot)) == ARG
    assert L().vga_gc_aligned_layout_for(None, -1, None, None, C.byref(tot)) == ARG
    assert L().vga_gc_aligned_create(None, 0, None) == ARG
    assert L().vga_gc_aligned_totals_of(None, C.byref(tot)) == ARG
    assert L().vga_gc_aligned_offsets(None, None, None) == ARG
    assert not L().vga_gc_aligned_ragged_in(None) and not L().vga_gc_aligned_ragged_out(None)
    L().vga_gc_aligned_destroy(None)
    assert L().vga_gcadpcm_align_channels_device_v(None, None, None, None, None, None, None, None, None, 0, None) == ARG


# ---------------------------------------------------------------- the header alone under the sanitizers
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for files in cases:
            f.write(struct.pack("<i", len(files)))
            for x in files:
                ch = x.channel
                f.write(struct.pack("<8i", x.channels, x.sample_rate, ch.sample_count, ch.looping, ch.loop_start, ch.loop_end,
                                    ch.loop_alignment_multiple, ch.samples_per_seek_table_entry))


class Reader:
    def __init__(self, data):
        self.d, self.at = data, 0

    def take(self, fmt):
        v = struct.unpack_from("<" + fmt, self.d, self.at)
        self.at += struct.calcsize("<" + fmt)
        return list(v)

    def items(self, fmt):
        n = self.take("i")[0]
        flat = self.take(fmt * n) if n else []
        return list(zip(flat[0::2], flat[1::2]))

    def layout(self):
        rc, n = self.take("2i")
        msg = self.d[self.at:self.at + n].decode()
        self.at += n
        if rc:
            return rc, msg, None
        nf, nch, nal = self.take("3i")
        r = {"first_channel": self.take("%di" % nf), "counts": self.take("%di" % nch), "out_counts": self.take("%di" % nch),
             "tail_counts": self.take("%di" % nal), "rows": []}
        for _ in range(nch):
            v = self.take("7q15i")
            r["rows"].append(dict(zip(ROW_OFFSETS + ROW_FIELDS, v)))
        r["totals"] = self.take("6q")
        r["cut"] = dict(zip(["in_pcm", "tail_pcm", "tail_adpcm", "tail_coefs", "hist1", "hist2", "scratch", "scratch_bytes"], self.take("8q")))
        r["any_aligned"], r["any_seek"], r["any_loop_start"], r["ctx_past_file"] = self.take("4i")
        r["gather"], r["adpcm"], r["pcm"], r["meta"] = self.items("iI"), self.items("iI"), self.items("iI"), self.items("ii")
        return rc, msg, r


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the driver's answers to every case of this file, computed once"""
    import gc_files_cases as gf
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("gc_aligned_host")
    exe = str(tmp / "gc_aligned_host_driver")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    cases = {("set",): the_files(), ("needs",): ga.files_of(ga.NEEDS), ("plain",): ga.files_of([f + (0,) for f in gf.FILES]),
             ("big",): ga.files_of(ga.SET + ga.BIG), ("ctx",): ga.files_of(ga.SET[:2] + ga.REFUSED_SET), ("empty",): []}
    for name in sorted(REFUSED):
        cases[("refused", name)] = the_files()[:3] + [ga.gc_file(*REFUSED[name][0])]
    write_cases(tmp / "cases.bin", list(cases.values()))
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(cases), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    rd = Reader(open(tmp / "results.bin", "rb").read())
    out = {key: (files, rd.layout()) for key, files in cases.items()}
    assert rd.at == len(rd.d)
    return out


def check_tiling(ranges, total, what):
    """the [start, end) ranges cover [0, total) exactly once"""
    at = 0
    for start, end in sorted(ranges):
        assert start == at and end > start, (what, start, end, at)
        at = end
    assert at == total, (what, at, total)


GOOD = [("set",), ("needs",), ("plain",), ("big",), ("ctx",)]


def test_host_layer_layout_is_the_model_and_the_librarys(driver):
    for key in GOOD:
        files, (rc, msg, r) = driver[key]
        assert rc == 0, (key, msg)
        m = ga.model(files)
        assert r["first_channel"] == m["first_channel"] and r["counts"] == m["counts"] and r["out_counts"] == m["out_counts"]
        assert r["tail_counts"] == m["tail_counts"]
        fc, so, tot = AlignedFileSet.layout(files)                     # the library: the same header behind the C ABI
        assert list(fc) == r["first_channel"] and list(so) == [row["seek_off"] for row in r["rows"]]
        assert r["totals"][:5] == [tot.pcm_samples, tot.adpcm_bytes, tot.out_pcm_samples, tot.out_adpcm_bytes, tot.seek_shorts]
        assert r["totals"][:5] == [m["in_pcm_samples"], m["in_adpcm_bytes"], m["out_pcm_samples"], m["out_adpcm_bytes"], m["seek_shorts"]]
        # the workspace: the driver hands in an encoder scratch of 0 bytes, the library the encoder's
        assert r["totals"][5] == m["workspace"] and r["cut"]["scratch"] == (m["workspace"] if m["tail_counts"] else 0)
        assert tot.workspace_bytes - r["totals"][5] >= 1024 * 12 * len(m["tail_counts"])
        if m["tail_counts"]:
            cut = r["cut"]
            assert cut["in_pcm"] == 0 and cut["tail_pcm"] == m["in_pcm_samples"] * 2
            assert cut["tail_adpcm"] == cut["tail_pcm"] + ga.up(m["tail_pcm_samples"] * 2, 16)
            assert cut["tail_coefs"] == cut["tail_adpcm"] + ga.up(m["tail_adpcm_bytes"], 16)
            assert cut["hist1"] == cut["tail_coefs"] + 32 * len(m["tail_counts"]) and cut["scratch"] == m["scratch_at"]
            assert all(v % 16 == 0 for v in cut.values())
        tail_row = 0
        for c, row in enumerate(r["rows"]):
            assert [row[k] for k in ROW_OFFSETS[:4]] == [m["in_pcm_off"][c], m["in_adpcm_off"][c], m["out_pcm_off"][c], m["out_adpcm_off"][c]]
            assert row["seek_off"] == m["seek_off"][c] and row["entries"] == m["entries"][c]
            if m["rows"][c]["needed"]:
                assert row["tail_row"] == tail_row
                assert (row["tail_pcm_off"], row["tail_adpcm_off"]) == (m["tail_pcm_off"][tail_row], m["tail_adpcm_off"][tail_row])
                tail_row += 1
            else:
                assert row["tail_row"] == -1
        assert [row["file"] for row in r["rows"]] == [i for i, f in enumerate(files) for _ in range(f.channels)]
        nch = len(r["rows"])
        assert r["meta"][:nch] == [(c, 0) for c in range(nch)]
        assert sorted(r["meta"][nch:]) == [(c, e) for c in range(nch) for e in range(ga.CHUNK, r["rows"][c]["entries"], ga.CHUNK)]
        assert r["any_aligned"] == bool(m["tail_counts"])
    assert driver[("ctx",)][1][2]["ctx_past_file"] == 2 and driver[("set",)][1][2]["ctx_past_file"] == -1
    big = driver[("big",)][1][2]
    assert len(big["meta"]) > len(big["rows"]), "no seek table of more than one chunk"


def test_align_rows_are_the_references_numbers(driver):
    """GcAdpcmAlignment.cs:29-39, computed in tests/gc_aligned_cases.py"""
    seen = set()
    for key in GOOD:
        files, (rc, msg, r) = driver[key]
        c = 0
        for f in files:
            a = ga.alignment_numbers(f)
            for _ in range(f.channels):
                row = r["rows"][c]
                for k in ("bytes_to_keep", "samples_to_keep", "samples_to_encode", "head", "loop_start", "loop_length", "loop_start_aligned", "out_samples"):
                    assert row[k] == a[k], (key, c, k)
                assert row["out_bytes"] == ga.byte_count(a["out_samples"]) == row["bytes_to_keep"] + ga.byte_count(row["samples_to_encode"])
                assert row["spacing"] == f.channel.samples_per_seek_table_entry
                if a["needed"]:
                    seen |= {("head0", row["head"] == 0), ("keep0", row["samples_to_keep"] == 0), ("keep8", row["bytes_to_keep"] % 16 == 8),
                             ("loop1", row["loop_length"] == 1), ("loop>tail", row["loop_length"] > row["samples_to_encode"]),
                             ("shorter", row["out_samples"] < f.channel.sample_count), ("longer", row["out_samples"] > f.channel.sample_count)}
                c += 1
    assert all((k, True) in seen for k in ("head0", "keep0", "keep8", "loop1", "loop>tail", "shorter", "longer")), seen


def test_work_tables_cover_every_byte_once(driver):
    granules = set()
    for key in GOOD:
        files, (rc, msg, r) = driver[key]
        per = {"gather": {}, "adpcm": {}, "pcm": {}}
        for name in per:
            for x, y in r[name]:
                per[name].setdefault(x, []).append(y)
        for c, row in enumerate(r["rows"]):
            ys = per["gather"].pop(c, [])
            assert sorted(ys) == list(range(0, row["samples_to_encode"], ga.CHUNK)), (key, c)      # none without a tail, none behind it
            for name, keep, total in (("adpcm", row["bytes_to_keep"], row["out_bytes"]), ("pcm", row["samples_to_keep"] * 2, row["out_samples"] * 2)):
                ranges = []
                for y in per[name].pop(c, []):
                    start, end, gran = ga.item_range(keep, total, y)
                    assert start < total, "an item wholly outside its row"
                    # both rows of the kept part start on 16 bytes; the rest lands `keep` into the output row
                    assert gran == (16 if start < keep else 16 if keep % 16 == 0 else 8 if keep % 8 == 0 else 4), (key, c, name)
                    assert start % gran == (0 if start < keep else keep % gran)
                    granules.add((name, start >= keep, gran))
                    ranges.append((start, end))
                if total:
                    check_tiling(ranges, total, (key, c, name))
                else:
                    assert not ranges
        assert not any(per.values())
    assert {("adpcm", True, 16), ("adpcm", True, 8), ("pcm", True, 16), ("pcm", True, 8), ("pcm", True, 4)} <= granules, granules


def test_host_layer_refusals(driver):
    for name in sorted(REFUSED):
        _, (rc, msg, _) = driver[("refused", name)]
        assert rc == REFUSED[name][1] and re.search(r"file 3\b", msg), (name, rc, msg)
    _, (rc, msg, r) = driver[("empty",)]
    assert rc == 0 and r["totals"] == [128, 256, 128, 256, 0, 0] and not (r["gather"] or r["adpcm"] or r["pcm"] or r["meta"])


# ---------------------------------------------------------------- the gather's arithmetic against the oracle's re-encode
def test_emulated_gather_over_the_align_rows_is_what_the_oracle_encodes(driver):
    """newPcm of GcAdpcmAlignment.cs:44-51 by the kernel's index arithmetic (ga.emulate_gather) over the host layer's AlignRow
    table, on the oracle's plain decode: encoded with the histories of the last kept samples it is the oracle's aligned tail"""
    files, (rc, msg, r) = driver[("set",)]
    ref, c, tails = ga.reference(ga.SET), 0, 0
    for f, chans in zip(files, ref):
        for ch in chans:
            row = r["rows"][c]
            c += 1
            assert ch["rc"] == 0
            keep = row["bytes_to_keep"]
            assert np.array_equal(ch["out"][:keep], ch["adpcm"][:keep])
            if row["tail_row"] < 0:
                assert ch["out"].size == keep and np.array_equal(ch["pcm"], ch["plain"])
                continue
            new_pcm, h1, h2 = ga.emulate_gather(ch["plain"], row)
            assert np.array_equal(po.gc_encode(new_pcm, ch["coefs"], hist1=h1, hist2=h2), ch["out"][keep:]), ("channel", c - 1)
            tails += 1
    assert tails == len(ga.model(files)["tail_counts"])
