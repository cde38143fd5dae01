"""The layout layer the *_files_host.hpp headers share, without a GPU: vgaudio_amd/csrc/files_layout.hpp and
gc_files_layout.hpp on their own under AddressSanitizer and UBSan (tests/host/files_layout_driver.cpp), against a model of their
rules written here and against figures written out by hand."""
import os
import platform
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "host", "files_layout_driver.cpp")
ARG, RANGE = -1, -2
NEGATIVE, OFFSET_PAST_MAX, PAST_2GIB, TOTAL_PAST_MAX = 1, 2, 4, 8
MAX_TOTAL, MAX_COUNT, GUARD = 1 << 62, (1 << 31) - 1, 256
IMAGES, COUNTER, GC_ROWS, OVERLAP, META, ROWS, ITEMS, OPENING, REGIONS = range(9)


def pad(v, m):
    q = abs(v + m - 1) // m                                            # C++ divides towards zero
    return (q if v + m - 1 >= 0 else -q) * m


# ---------------------------------------------------------------- the cases: name -> (kind, arguments)
CASES = {
    "images_no_file": (IMAGES, ([], None)),
    "images_one_empty_file": (IMAGES, ([0], None)),
    "images_sizes_round_16": (IMAGES, ([1, 15, 16, 17], None)),
    "images_offsets_out_of_order": (IMAGES, ([100, 7, 40, 0], [4096, 0, 1024, 8])),
    "images_offset_minus_one": (IMAGES, ([10, 10], [16, -1])),
    "images_offset_2_62": (IMAGES, ([10, 0, 10], [0, MAX_TOTAL, MAX_TOTAL + 1])),
    "images_size_2_31": (IMAGES, ([MAX_COUNT, MAX_COUNT + 1], None)),
    "images_end_at_2_62": (IMAGES, ([16, 17], [MAX_TOTAL - 16, MAX_TOTAL - 16])),
    "counter_reaches_2_31_minus_1": (COUNTER, (MAX_COUNT - 5, 5, 0)),
    "counter_one_past": (COUNTER, (MAX_COUNT - 5, 6, 0)),
    "counter_one_past_rows": (COUNTER, (MAX_COUNT, 1, 1)),
    "counter_from_nothing": (COUNTER, (0, 0, 1)),
    "gc_rows_none": (GC_ROWS, ([], [])),
    "gc_rows_sample_counts": (GC_ROWS, ([0, 1, 14, 15], [0, 0, 0, 0])),
    "gc_rows_seek_entries": (GC_ROWS, ([15, 15, 15, 15, 15, 29], [0, 1, 3, 4, 5, 1])),
    "overlap_touching": (OVERLAP, ([0, 10, 20], [10, 10, 5])),
    "overlap_by_one": (OVERLAP, ([0, 9, 30], [10, 10, 5])),
    "overlap_out_of_order_by_one": (OVERLAP, ([30, 19, 0], [5, 12, 10])),
    "overlap_empty_inside": (OVERLAP, ([0, 5, 10], [10, 0, 4])),
    "overlap_equal_offsets": (OVERLAP, ([8, 0, 8], [4, 8, 4])),
    "overlap_none_given": (OVERLAP, ([], [])),
    "meta_channel_0": (META, (0,)),
    "meta_channel_1": (META, (1,)),
    "rows_packed": (ROWS, ([0, 1, 8, 9], [0, 8, 8, 16], None, MAX_TOTAL // 2)),
    "rows_offsets": (ROWS, ([5, 0, 7, 3], [8, 0, 8, 8], [100, 5000, 0, -1], MAX_TOTAL // 2)),
    "rows_limit": (ROWS, ([1, 1], [8, 8], [MAX_TOTAL // 2, MAX_TOTAL // 2 + 1], MAX_TOTAL // 2)),
    "rows_packed_past_limit": (ROWS, ([24, 8, 8], [24, 8, 8], None, 31)),
    "items_general_file": (ITEMS, (0, 3, 2, 33, 16, 0)),
    "items_fast_file": (ITEMS, (1, 3, 2, 33, 16, 4)),
    "items_exact_chunks": (ITEMS, (0, 0, 1, 32, 16, 2)),
    "items_nothing_to_move": (ITEMS, (0, 0, 3, 0, 16, 0)),
    "opening_negative_count": (OPENING, (-1, 1)),
    "opening_null_array": (OPENING, (2, 0)),
    "opening_empty_set_null_array": (OPENING, (0, 0)),
    "opening_fine": (OPENING, (2, 1)),
    "regions_count_only": (REGIONS, (5, 0, 0, 1)),
    "regions_fit": (REGIONS, (5, 5, 1, 1)),
    "regions_capacity_short": (REGIONS, (5, 4, 1, 1)),
    "regions_null_count": (REGIONS, (5, 5, 1, 0)),
}
INFO = (np.arange(46, dtype=np.int64) * 523 - 12000).astype(np.int16)   # coefs[2][16], gain[2], start[2][3], loop[2][3]


def pack_case(kind, a):
    q = lambda v: struct.pack("<%dq" % len(v), *v)
    i = lambda v: struct.pack("<%di" % len(v), *v)
    head = struct.pack("<i", kind)
    if kind == IMAGES:
        return head + i([len(a[0]), a[1] is not None]) + q(a[0]) + q(a[1] or [])
    if kind == COUNTER:
        return head + struct.pack("<qii", *a)
    if kind == GC_ROWS:
        return head + i([len(a[0])]) + i(a[0]) + i(a[1])
    if kind == OVERLAP:
        return head + i([len(a[0])]) + q(a[0]) + i(a[1])
    if kind == META:
        return head + INFO.tobytes() + i(a)
    if kind == ROWS:
        return head + i([len(a[0]), a[2] is not None]) + q([a[3]]) + q(a[0]) + q(a[1]) + q(a[2] or [])
    if kind == ITEMS:
        return head + struct.pack("<iiiqqi", *a)
    if kind == OPENING:
        return head + i(a)
    return head + struct.pack("<iqii", *a)


class Reader:
    def __init__(self, data):
        self.data, self.at = data, 0

    def get(self, fmt):
        v = struct.unpack_from("<" + fmt, self.data, self.at)
        self.at += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def message(self):
        n = self.get("i")
        self.at += n
        return self.data[self.at - n:self.at].decode()


def read_case(r, kind, a):
    if kind in (IMAGES, ROWS):
        placed = [r.get("qi") for _ in a[0]]
        return placed, r.get("qqq" if kind == IMAGES else "qq")
    if kind == COUNTER:
        return r.get("i"), r.get("q"), r.message()
    if kind == GC_ROWS:
        return [r.get("qqq") for _ in a[0]], r.get("iqqq")
    if kind == OVERLAP:
        return r.get("iii")
    if kind == META:
        return list(r.get("23h"))
    if kind == ITEMS:
        tables = [[r.get("iI") for _ in range(r.get("i"))] for _ in range(2)]
        return tables, r.get("i")
    if kind == OPENING:
        return r.get("i"), r.message(), r.get("i"), r.message()
    rc, msg, count = r.get("i"), r.message(), r.get("q")
    return rc, msg, count, [r.get("q") for _ in range(r.get("i"))]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """name -> what the driver wrote for the case, every case in one run"""
    gxx, setarch = shutil.which("g++"), shutil.which("setarch")
    assert gxx and setarch, "g++ and setarch (util-linux) are part of the image"
    tmp = tmp_path_factory.mktemp("files_layout")
    exe = str(tmp / "files_layout_driver")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-fwrapv", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", DRIVER, "-o", exe], check=True)
    names = sorted(CASES)
    with open(tmp / "cases.bin", "wb") as f:
        f.write(struct.pack("<i", len(names)))
        for name in names:
            f.write(pack_case(*CASES[name]))
    r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp / "cases.bin"), str(tmp / "results.bin")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "%d ok" % len(names), r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr.strip(), r.stderr
    reader = Reader(open(tmp / "results.bin", "rb").read())
    out = {name: read_case(reader, *CASES[name]) for name in names}
    assert reader.at == len(reader.data)
    return out


# ---------------------------------------------------------------- image placement
def model_images(sizes, offsets):
    at, end, placed = 0, 0, []
    for k, size in enumerate(sizes):
        here = at if offsets is None else offsets[k]
        at = pad(here + size, 16)
        end = max(end, at)
        placed.append((here, (here < 0) * NEGATIVE | (here > MAX_TOTAL) * OFFSET_PAST_MAX | (size > MAX_COUNT) * PAST_2GIB |
                       (at > MAX_TOTAL) * TOTAL_PAST_MAX))
    return placed, (at, end, end + GUARD)


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][0] == IMAGES))
def test_images_are_the_model(driver, name):
    assert driver[name] == model_images(*CASES[name][1])


def test_images_by_hand(driver):
    assert driver["images_no_file"] == ([], (0, 0, GUARD))
    assert driver["images_one_empty_file"] == ([(0, 0)], (0, 0, GUARD))
    assert driver["images_sizes_round_16"] == ([(0, 0), (16, 0), (32, 0), (48, 0)], (80, 80, 80 + GUARD))
    # the caller's offsets in any order: the total reaches behind the farthest image, 4096 + 100 rounded up, not the last
    placed, (at, end, total) = driver["images_offsets_out_of_order"]
    assert [p[0] for p in placed] == [4096, 0, 1024, 8] and not any(p[1] for p in placed)
    assert (at, end, total) == (16, 4208, 4208 + GUARD)
    assert driver["images_offset_minus_one"][0] == [(16, 0), (-1, NEGATIVE)]
    # an offset of 2^62 exactly is fine (an empty image there ends at it), one more is not
    assert [p[1] for p in driver["images_offset_2_62"][0]] == [0, 0, OFFSET_PAST_MAX | TOTAL_PAST_MAX]
    assert [p[1] for p in driver["images_size_2_31"][0]] == [0, PAST_2GIB]
    # an image that ends at 2^62 exactly is fine, one byte more is not
    assert [p[1] for p in driver["images_end_at_2_62"][0]] == [0, TOTAL_PAST_MAX]


# ---------------------------------------------------------------- row placement
def model_rows(lengths, rooms, offsets, limit):
    at, end, placed = 0, 0, []
    for k, (length, room) in enumerate(zip(lengths, rooms)):
        here = at if offsets is None else offsets[k]
        if offsets is None:
            at += room
            end = at
        elif length > 0:
            end = max(end, here + length)
        placed.append((here, (here < 0) * NEGATIVE | (here > limit) * OFFSET_PAST_MAX | (at > limit) * TOTAL_PAST_MAX))
    return placed, (at, end)


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][0] == ROWS))
def test_rows_are_the_model(driver, name):
    assert driver[name] == model_rows(*CASES[name][1])


def test_rows_by_hand(driver):
    assert driver["rows_packed"] == ([(0, 0), (0, 0), (8, 0), (16, 0)], (32, 32))
    # at the caller's offsets nothing is packed, and an empty row (at 5000) does not count towards the end
    assert driver["rows_offsets"] == ([(100, 0), (5000, 0), (0, 0), (-1, NEGATIVE)], (0, 105))
    assert [p[1] for p in driver["rows_limit"][0]] == [0, OFFSET_PAST_MAX]
    assert [p[1] for p in driver["rows_packed_past_limit"][0]] == [0, TOTAL_PAST_MAX, OFFSET_PAST_MAX | TOTAL_PAST_MAX]


# ---------------------------------------------------------------- the counter
def test_counter(driver):
    assert driver["counter_reaches_2_31_minus_1"] == (0, MAX_COUNT, "")
    assert driver["counter_one_past"] == (ARG, MAX_COUNT - 5, "file 7: more than 2^31 channels")
    assert driver["counter_one_past_rows"] == (ARG, MAX_COUNT, "file 7: more than 2^31 rows")
    assert driver["counter_from_nothing"] == (0, 0, "")


# ---------------------------------------------------------------- rows of the GC-ADPCM family
def gc_bytes(samples):
    nibbles = samples // 14 * 16 + (samples % 14 + 2 if samples % 14 else 0)
    return (nibbles + 1) // 2


def model_gc_rows(samples, entries):
    pcm = np.concatenate([[0], np.cumsum([pad(n, 8) for n in samples], dtype=np.int64)])
    adpcm = np.concatenate([[0], np.cumsum([pad(gc_bytes(n), 16) for n in samples], dtype=np.int64)])
    seek = np.concatenate([[0], np.cumsum([pad(2 * e, 8) for e in entries], dtype=np.int64)])
    rows = [(int(pcm[c]), int(adpcm[c]), int(seek[c])) for c in range(len(samples))]
    return rows, (len(samples), int(pcm[-1]) + GUARD // 2, int(adpcm[-1]) + GUARD, int(seek[-1]))


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][0] == GC_ROWS))
def test_gc_rows_are_the_model(driver, name):
    assert driver[name] == model_gc_rows(*CASES[name][1])


def test_gc_rows_by_hand(driver):
    assert driver["gc_rows_none"] == ([], (0, 128, 256, 0))
    # 0, 1, 14 and 15 samples are 0, 2, 8 and 10 bytes: rooms of 0, 8, 16, 16 samples and 0, 16, 16, 16 bytes
    rows, totals = driver["gc_rows_sample_counts"]
    assert [r[0] for r in rows] == [0, 0, 8, 24] and [r[1] for r in rows] == [0, 0, 16, 32] and totals == (4, 40 + 128, 48 + 256, 0)
    # 0, 1, 3, 4, 5 and 1 seek entries take 0, 8, 8, 8, 16 and 8 shorts
    rows, totals = driver["gc_rows_seek_entries"]
    assert [r[2] for r in rows] == [0, 0, 8, 16, 24, 40] and totals[3] == 48


# ---------------------------------------------------------------- the overlap check
def model_overlap(off, length):
    order = sorted((c for c in range(len(off)) if length[c] > 0), key=lambda c: (off[c], c))
    for a, b in zip(order, order[1:]):
        if off[a] + length[a] > off[b]:
            return (1, a, b)
    return (0, -1, -1)


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][0] == OVERLAP))
def test_overlap_is_the_model(driver, name):
    assert driver[name] == model_overlap(*CASES[name][1])


def test_overlap_by_hand(driver):
    assert driver["overlap_touching"] == (0, -1, -1)
    assert driver["overlap_by_one"] == (1, 0, 1)
    assert driver["overlap_out_of_order_by_one"] == (1, 1, 0)          # range 1 (19 .. 31) lies in front of range 0 (30 ..)
    assert driver["overlap_empty_inside"] == (0, -1, -1)
    assert driver["overlap_equal_offsets"] == (1, 0, 2)                # 1 (0 .. 8) touches; of the two at 8 the lower index is in front
    assert driver["overlap_none_given"] == (0, -1, -1)


# ---------------------------------------------------------------- channel metadata
@pytest.mark.parametrize("c", [0, 1])
def test_fill_meta_is_the_23_shorts(driver, c):
    coefs, gain, start, loop = INFO[:32].reshape(2, 16), INFO[32:34], INFO[34:40].reshape(2, 3), INFO[40:46].reshape(2, 3)
    by_hand = [int(coefs[c][k]) for k in range(16)] + [int(gain[c])] + [int(start[c][0]), int(start[c][1]), int(start[c][2])] + \
              [int(loop[c][0]), int(loop[c][1]), int(loop[c][2])]
    assert len(by_hand) == 23 and driver["meta_channel_%d" % c] == by_hand
    assert len(set(INFO.tolist())) == 46, "every short of the info is its own value"


# ---------------------------------------------------------------- work items, the opening checks, the regions
def model_items(fast, first, count, per, unit, nfast):
    general = [(first + k, y) for k in range(count) for y in range((per + unit - 1) // unit)]
    front = [(100 + k, k) for k in range(nfast)]
    return [front + ([] if fast else general), general], nfast


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n][0] == ITEMS))
def test_items_are_the_model(driver, name):
    assert driver[name] == model_items(*CASES[name][1])


def test_items_by_hand(driver):
    general = [(3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2)]        # 33 bytes in chunks of 16: three per owner
    assert driver["items_general_file"] == ([general, general], 0)
    assert driver["items_fast_file"] == ([[(100, 0), (101, 1), (102, 2), (103, 3)], general], 4)
    assert driver["items_exact_chunks"] == ([[(100, 0), (101, 1), (0, 0), (0, 1)], [(0, 0), (0, 1)]], 2)
    assert driver["items_nothing_to_move"] == ([[], []], 0)


def test_opening_checks_and_name_file(driver):
    named = (RANGE, "file 3: inner 5")
    assert driver["opening_negative_count"] == (ARG, "negative file count") + named
    assert driver["opening_null_array"] == (ARG, "null infos") + named
    assert driver["opening_empty_set_null_array"] == (0, "") + named
    assert driver["opening_fine"] == (0, "") + named


def test_regions(driver):
    assert driver["regions_count_only"] == (0, "", 5, [])
    assert driver["regions_fit"] == (0, "", 5, [1000, 1001, 1002, 1003, 1004])
    assert driver["regions_capacity_short"] == (ARG, "5 regions: capacity 4", 5, [])
    assert driver["regions_null_count"] == (ARG, "null count", -1, [])


def test_the_cases_hold_what_they_are_for():
    assert CASES["images_sizes_round_16"][1][0] == [1, 15, 16, 17]
    assert CASES["images_offset_2_62"][1][1][1:] == [2 ** 62, 2 ** 62 + 1] and -1 in CASES["images_offset_minus_one"][1][1]
    assert CASES["images_size_2_31"][1][0] == [2 ** 31 - 1, 2 ** 31]
    offsets = CASES["images_offsets_out_of_order"][1][1]
    assert offsets != sorted(offsets)
    assert sum(CASES["counter_reaches_2_31_minus_1"][1][:2]) == 2 ** 31 - 1 and sum(CASES["counter_one_past"][1][:2]) == 2 ** 31
    assert CASES["gc_rows_sample_counts"][1][0] == [0, 1, 14, 15] and CASES["gc_rows_seek_entries"][1][1][:5] == [0, 1, 3, 4, 5]
