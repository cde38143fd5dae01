"""include/vgaudio_hip_files/wave_files.h on the GPU: the rows read out of a set of WAVE images of different shapes against the
oracle's WaveReader and against the per-file device calls, for packed rows and rows at the caller's odd offsets, images packed
and at offsets of residues 1, 2, 4 and 8; the images written from rows against the oracle's WaveWriter (a model for 8-bit
files) and the per-file calls; all inside junk-filled buffers whose every byte outside the rows / images is checked; write ->
vga_wave_parse -> read; the forced general form against the mixed forms; poison mode; a busy caller stream; two streams at
once; refused calls; the object's numbers; the GC ragged offsets; the chain through a ragged ADX object both ways; the Python
mirror; offsets past 4 GiB.  The cases are tests/wave_files_cases.py's; tests/test_wave_files_host.py checks that CASES names
every function of the header."""
import ctypes as C

import numpy as np
import pytest

import wave_files_cases as wc
from far_memory import GIB, FarBuffer, need, release
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd import wave
from vgaudio_amd.gcadpcm import Pcm16Format
from vgaudio_amd.wave import WaveFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_wave_files_layout_for": ["test_object_numbers_are_the_host_layouts", "test_write_files_is_the_writers_get_file"],
    "vga_wave_files_create": ["test_images_are_the_oracles_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_wave_files_create_from_infos": ["test_read_gives_the_oracles_and_the_per_file_rows", "test_write_parse_read_returns_the_rows"],
    "vga_wave_files_destroy": ["test_images_are_the_oracles_and_the_per_file_calls"],
    "vga_wave_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_wave_files_offsets": ["test_object_numbers_are_the_host_layouts", "test_packed_rows_are_the_gc_ragged_offsets"],
    "vga_wave_write_device_v": [
        "test_images_are_the_oracles_and_the_per_file_calls", "test_write_parse_read_returns_the_rows",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_write_files_is_the_writers_get_file",
        "test_chain_through_a_ragged_adx_object", "test_offsets_past_4_gib"],
    "vga_wave_read_device_v": [
        "test_read_gives_the_oracles_and_the_per_file_rows", "test_write_parse_read_returns_the_rows",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_read_files_is_the_readers_read_format",
        "test_chain_through_a_ragged_adx_object", "test_offsets_past_4_gib"],
    "vga_wave_files_write_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_wave_files_read_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_wave_files_stats": ["test_forced_general_form_gives_the_same_bytes", "test_object_numbers_are_the_host_layouts"],
    "vga_wave_files_force_general_this_thread": ["test_forced_general_form_gives_the_same_bytes"],
}

JUNK = 0xEE
JUNK16 = np.array([0xEEEE], np.uint16).view(np.int16)[0]
EXTRA = 64                                                             # junk in front of and behind every buffer (keeps 16-byte alignment)
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def dev(a):
    return torch().from_numpy(np.array(a, copy=True, order="C")).cuda()


def host(t):
    return t.cpu().numpy()


def stream_ptr(stream=None):
    return C.c_void_p((stream if stream is not None else torch().cuda.current_stream()).cuda_stream)


def junk16(fill):
    return np.array([fill * 0x101], np.uint16).view(np.int16)[0]


class WriteSet:
    """the reference's files as a set for writing: name "packed" or "explicit" (rows at any sample boundary, images at odd bytes)"""

    def __init__(self, name="packed"):
        self.cases, self.files, self.rows, self.want = wc.reference()
        sizes = [len(w) for w in self.want]
        self.po = wc.explicit_pcm_offsets(wc.counts_of(self.files)) if name == "explicit" else None
        self.io = wc.image_offsets_at(sizes, 5) if name == "explicit" else None
        self.s = WaveFileSet(self.files, self.po, self.io)

    def close(self):
        self.s.close()

    def pcm(self, fill=JUNK):
        """the rows inside a junk-filled buffer: junk in the rounding gaps, between the rows and in the guard"""
        a = np.full(self.s.totals.pcm_samples, junk16(fill), np.int16)
        for c, row in enumerate(self.rows):
            a[self.s.pcm_offsets[c]:self.s.pcm_offsets[c] + len(row)] = row
        return dev(a)

    def images(self, fill=JUNK):
        return torch().full((self.s.totals.image_bytes + 2 * EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def run(self, pcm, images, stream=None):
        _lib.check(L().vga_wave_write_device_v(self.s._h, pcm.data_ptr(), images.data_ptr() + EXTRA, stream_ptr(stream)))
        return images

    def check(self, images, what, fill=JUNK):
        """every image is the reference's, every other byte of the buffer is what it was"""
        got = host(images).copy()
        assert np.all(got[:EXTRA] == fill) and np.all(got[-EXTRA:] == fill), (what, "outside the buffer")
        got = got[EXTRA:-EXTRA]
        for f, (at, want) in enumerate(zip(self.s.image_offsets, self.want)):
            mine = got[at:at + len(want)]
            if not np.array_equal(mine, want):
                bad = np.flatnonzero(mine != want)
                raise AssertionError((what, "file", f, self.cases[f], "first bad byte", int(bad[0]), "of", len(want), "bad bytes", len(bad)))
            got[at:at + len(want)] = fill
        assert np.all(got == fill), (what, "bytes outside the images were written", np.flatnonzero(got != fill)[:8])


_read_side = []


class ReadSet:
    """the read side's images as a set for reading: rows "packed" or "explicit", images "packed" or at a residue of 16"""

    def __init__(self, rows="packed", residue=None):
        if not _read_side:
            images, want = wc.read_side()
            _read_side.append((images, want, [wc.parse(i) for i in images]))
        self.images_, self.want, self.infos = _read_side[0]
        sizes = [len(i) for i in self.images_]
        self.po = wc.explicit_pcm_offsets([[i.sample_count] * i.channel_count for i in self.infos]) if rows == "explicit" else None
        self.io = wc.image_offsets_at(sizes, residue) if residue is not None else None
        self.s = WaveFileSet.from_infos(self.infos, self.po, self.io)
        assert self.s.image_sizes == sizes

    def close(self):
        self.s.close()

    def images(self, fill=JUNK):
        """the images inside a junk-filled buffer"""
        a = np.full(self.s.totals.image_bytes, fill, np.uint8)
        for image, at in zip(self.images_, self.s.image_offsets):
            a[at:at + len(image)] = image
        return dev(a)

    def pcm(self, fill=JUNK):
        return torch().full((self.s.totals.pcm_samples + EXTRA,), int(junk16(fill)), dtype=torch().int16, device="cuda")

    def run(self, images, pcm, stream=None):
        _lib.check(L().vga_wave_read_device_v(self.s._h, images.data_ptr(), pcm.data_ptr() + EXTRA, stream_ptr(stream)))
        return pcm

    def check(self, pcm, what, fill=JUNK):
        """every row is the reader's, every other sample of the buffer is what it was"""
        got, j = host(pcm).copy(), junk16(fill)
        assert np.all(got[:EXTRA // 2] == j), (what, "in front of the buffer")
        got = got[EXTRA // 2:]
        c = 0
        for f, (info, rows) in enumerate(zip(self.infos, self.want)):
            for ch in range(info.channel_count):
                at, n = int(self.s.pcm_offsets[c]), info.sample_count
                if not np.array_equal(got[at:at + n], rows[ch][:n]):
                    bad = np.flatnonzero(got[at:at + n] != rows[ch][:n])
                    raise AssertionError((what, "file", f, "channel", ch, "of", info.channel_count, "bits", info.bits_per_sample, "first bad sample",
                                          int(bad[0]), "of", n, "bad samples", len(bad)))
                got[at:at + n] = j
                c += 1
        assert np.all(got == j), (what, "samples outside the rows were written", np.flatnonzero(got != j)[:8])


# ---------------------------------------------------------------- 1. read
_want_checked = []


def want_is_the_oracles_and_the_per_file_calls(r):
    """`want`, the rows every read result of this file is compared with, IS what the oracle's reader (16-bit images) and the
    per-file device calls (every image alone) deliver: shown once per session, asked for by every read case"""
    if _want_checked:
        return
    t = torch()
    images, infos, want_rows = r.images_, r.infos, r.want
    # the oracle's reader for the 16-bit images, and the per-file device calls for every image alone
    for f, (image, info, want) in enumerate(zip(images, infos, want_rows)):
        if info.bits_per_sample == 16:
            rc, _, chans = po.wave_read(image.tobytes())
            assert rc == 0 and all(np.array_equal(a, b) for a, b in zip(chans, want)), f
        n, nch = info.sample_count, info.channel_count
        if n == 0:
            continue
        d_file = dev(image)
        out = t.full((nch, n + 3), int(JUNK16), dtype=t.int16, device="cuda")
        if info.bits_per_sample == 16:
            _lib.check(L().vga_wave_deinterleave_pcm16_device(d_file.data_ptr() + info.data_offset, n, nch, out.data_ptr(), n + 3, stream_ptr()))
        else:
            _lib.check(L().vga_wave_deinterleave_pcm8_device(d_file.data_ptr() + info.data_offset, n, nch, out.data_ptr(), 0, n + 3, stream_ptr()))
        got = host(out)
        assert all(np.array_equal(got[ch, :n], want[ch][:n]) for ch in range(nch)), ("per-file call", f)
    _want_checked.append(True)


@pytest.mark.parametrize("rows,residue", [("packed", None), ("explicit", 1), ("packed", 2), ("explicit", 4), ("packed", 8)])
def test_read_gives_the_oracles_and_the_per_file_rows(rows, residue):
    t = torch()
    r = ReadSet(rows, residue)
    try:
        assert residue is None or all(o % 16 == residue for o in r.s.image_offsets)
        pcm = r.run(r.images(), r.pcm())
        t.cuda.synchronize()
        r.check(pcm, (rows, residue))
        want_is_the_oracles_and_the_per_file_calls(r)
    finally:
        r.close()


# ---------------------------------------------------------------- 2. write
@pytest.mark.parametrize("name", ["packed", "explicit"])
def test_images_are_the_oracles_and_the_per_file_calls(name):
    t = torch()
    a = WriteSet(name)
    try:
        images = a.run(a.pcm(), a.images())
        t.cuda.synchronize()
        a.check(images, name)
        if name != "packed":
            return
        # the per-file device calls for every file alone, from rows staged at a pitch
        at = 0
        for f, file in enumerate(a.files):
            n, nch = file.params.sample_count, file.channels
            pitch = n + 5
            staged = np.full((nch, pitch), JUNK16, np.int16)
            for c in range(nch):
                staged[c, :n] = a.rows[at + c]
            d_rows = dev(staged)
            d_file = t.full((len(a.want[f]) + 32,), JUNK, dtype=t.uint8, device="cuda")
            if file.bits == 16:
                _lib.check(L().vga_wave_write_pcm16_device(d_rows.data_ptr(), pitch, nch, C.byref(file.params), d_file.data_ptr(), stream_ptr()))
            else:
                _lib.check(L().vga_wave_write_pcm8_device(d_rows.data_ptr(), 0, pitch, nch, C.byref(file.params), d_file.data_ptr(), stream_ptr()))
            got = host(d_file)
            assert np.array_equal(got[:len(a.want[f])], a.want[f]) and np.all(got[len(a.want[f]):] == JUNK), ("per-file call", f)
            at += nch
        # ... and the host forms of the per-file calls, whose size and header code moved (wave_file_host.hpp)
        f = next(k for k, c in enumerate(a.cases) if c[0] == 3 and c[3])
        first = int(a.s.first_channel[f])
        fmt = Pcm16Format([a.rows[first + c] for c in range(3)], 44100).WithLoop(True, *a.cases[f][3])
        codec = wave.WaveCodec.Pcm16Bit if a.cases[f][1] == 16 else wave.WaveCodec.Pcm8Bit
        assert wave.WaveWriter.GetFile(fmt, codec) == a.want[f].tobytes()
    finally:
        a.close()


def test_write_parse_read_returns_the_rows():
    """write, vga_wave_parse of every image on the host, a set from the infos over the SAME buffers, read: the rows"""
    t = torch()
    a = WriteSet("explicit")
    try:
        images = a.run(a.pcm(), a.images())
        t.cuda.synchronize()
        files_bytes = a.s.images(host(images)[EXTRA:-EXTRA])
        infos = []
        for b, case in zip(files_bytes, a.cases):                      # (WaveReader refuses a file without samples: described by hand)
            infos.append(wave.WaveReader.ReadMetadata(b) if case[2] else _lib.WaveInfoC(case[0], 44100, case[1], 0, 0, 0, 0, 0, len(b), 0, 0))
        r = WaveFileSet.from_infos(infos, a.po, [int(o) for o in a.s.image_offsets])
        try:
            assert (r.totals.pcm_samples, r.totals.image_bytes) == (a.s.totals.pcm_samples, a.s.totals.image_bytes)
            rows = t.full((r.totals.pcm_samples,), int(JUNK16), dtype=t.int16, device="cuda")
            _lib.check(L().vga_wave_read_device_v(r._h, images.data_ptr() + EXTRA, rows.data_ptr(), stream_ptr()))
            t.cuda.synchronize()
            got, c = host(rows).copy(), 0
            for f, (case, info) in enumerate(zip(a.cases, infos)):
                assert (info.channel_count, info.bits_per_sample, info.sample_count) == case[:3]
                if case[2]:
                    assert (bool(info.looping), info.loop_start, info.loop_end) == ((True,) + case[3] if case[3] else (False, 0, 0))
                for ch in range(case[0]):
                    at = int(r.pcm_offsets[c])
                    assert np.array_equal(got[at:at + case[2]], wc.row_as_read(a.rows[c], case[1])), (f, ch)
                    got[at:at + case[2]] = JUNK16
                    c += 1
            assert np.all(got == JUNK16)
        finally:
            r.close()
    finally:
        a.close()


# ---------------------------------------------------------------- 3. forms
def test_forced_general_form_gives_the_same_bytes():
    t = torch()
    a, r = WriteSet("packed"), ReadSet("explicit", 1)
    try:
        mixed_w, mixed_r = a.s.stats(), r.s.stats()
        assert min(mixed_w) > 0 and min(mixed_r) > 0, (mixed_w, mixed_r)
        assert L().vga_wave_files_force_general_this_thread(1) == 0
        try:
            forced_w, forced_r = a.s.stats(), r.s.stats()
            assert forced_w[0] == forced_w[2] == 0 and forced_w[1] == mixed_w[0] + mixed_w[1] and forced_w[3] > mixed_w[3]
            assert forced_r[0] == forced_r[2] == 0 and forced_r[1] == mixed_r[0] + mixed_r[1]
            images = a.run(a.pcm(), a.images())
            pcm = r.run(r.images(), r.pcm())
            t.cuda.synchronize()
        finally:
            assert L().vga_wave_files_force_general_this_thread(0) == 1
        a.check(images, "forced general")
        r.check(pcm, "forced general")
        assert a.s.stats() == mixed_w
        again = a.run(a.pcm(), a.images())
        t.cuda.synchronize()
        assert t.equal(again, images)
    finally:
        r.close()
        a.close()


def test_object_numbers_are_the_host_layouts():
    for name in ("packed", "explicit"):
        a = WriteSet(name)
        try:
            fc, po_, io_, tot = WaveFileSet.layout(a.files, a.po, a.io)
            assert list(a.s.first_channel) == list(fc) and list(a.s.pcm_offsets) == list(po_) and list(a.s.image_offsets) == list(io_)
            assert all(getattr(a.s.totals, k) == getattr(tot, k) for k, _ in tot._fields_)
            assert a.s.image_sizes == [len(w) for w in a.want]
            items = [i for i in WaveFileSet.write_items(a.files, a.po, a.io) if i.form != wc.HEADER_ITEM]
            st = a.s.stats()
            assert (st[2], st[3]) == (sum(i.form == wc.TILE for i in items), sum(i.form == wc.GENERAL for i in items))
            assert st[0] == len({i.file for i in items if i.form == wc.TILE}) and st[1] == len({i.file for i in items if i.form == wc.GENERAL})
        finally:
            a.close()
    r = ReadSet("explicit", 4)
    try:
        items = WaveFileSet.read_items(r.infos, r.po, r.io)
        st = r.s.stats()
        assert (st[2], st[3]) == (sum(i.form == wc.TILE for i in items), sum(i.form == wc.GENERAL for i in items))
        assert r.s.channels == sum(i.channel_count for i in r.infos) and r.s.files == len(r.infos)
        assert list(r.s.pcm_offsets) == r.po and list(r.s.image_offsets) == r.io
    finally:
        r.close()


def test_packed_rows_are_the_gc_ragged_offsets():
    a = WriteSet("packed")
    try:
        counts = [n for per in wc.counts_of(a.files) for n in per]
        arr, h = (C.c_int * len(counts))(*counts), C.c_void_p()
        _lib.check(L().vga_gcadpcm_ragged_create(arr, len(counts), C.byref(h)))
        try:
            want = np.zeros(len(counts), np.int64)
            _lib.check(L().vga_gcadpcm_ragged_offsets(h, want.ctypes.data_as(C.POINTER(C.c_int64)), None))
            assert list(a.s.pcm_offsets) == list(want)
            assert L().vga_gcadpcm_ragged_pcm_samples(h) <= a.s.totals.pcm_samples + 128      # the caller allocates the larger
        finally:
            L().vga_gcadpcm_ragged_destroy(h)
    finally:
        a.close()


# ---------------------------------------------------------------- 4. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    t = torch()
    old = L().vga_testing_poison_allocations(value)
    try:
        a = WriteSet("packed")                                         # (created under the mode: its tables are poisoned first)
        try:
            images = a.run(a.pcm(value ^ 0x3C), a.images(value ^ 0x3C))
            t.cuda.synchronize()
            a.check(images, ("poison", value), fill=value ^ 0x3C)
        finally:
            a.close()
        r = ReadSet("packed", 1)
        try:
            pcm = r.run(r.images(value), r.pcm(value ^ 0x3C))
            t.cuda.synchronize()
            r.check(pcm, ("poison", value), fill=value ^ 0x3C)
        finally:
            r.close()
    finally:
        t.cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 5. streams
_streams = []


def some_streams(n):
    """Streams for this file, taken once and so that the files that run after it find torch's stream pool as they would without
    it (tests/test_gpu_nw_files.py: some_streams): one whole turn of the pool with the imported `delay` fixture's, every stream
    used once, in order."""
    t = torch()
    if not _streams:
        _streams.extend(t.cuda.Stream() for _ in range(POOL_STREAMS - 1))
        for s in _streams:
            with t.cuda.stream(s):
                t.zeros(1, device="cuda")
        t.cuda.synchronize()
    return _streams[:n]


def test_calls_on_a_busy_stream(delay):  # noqa: F811
    """both calls queued behind a delay on the caller's stream: they do not wait for it, and they are ordered after it -- their
    inputs are written on the same stream after the delay"""
    t = torch()
    cycles, ms = delay
    a, r = WriteSet("packed"), ReadSet("packed", 2)
    try:
        (S,) = some_streams(1)
        source, packed = a.pcm(), r.images()
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                d_source, d_images = t.zeros_like(source), t.zeros_like(packed)
                images, pcm = a.images(), r.pcm()
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                d_source.copy_(source, non_blocking=True)              # the inputs arrive behind the delay
                d_images.copy_(packed, non_blocking=True)
                a.run(d_source, images, stream=S)
                r.run(d_images, pcm, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, "busy stream")
        r.check(pcm, "busy stream")
    finally:
        r.close()
        a.close()


def test_two_streams_at_once():
    """one object for each direction, two streams each"""
    t = torch()
    a, r = WriteSet("explicit"), ReadSet("explicit", 8)
    try:
        S1, S2 = some_streams(2)
        d_pcm, i1, i2 = a.pcm(), a.images(), a.images(0x11)
        d_images, p1, p2 = r.images(), r.pcm(), r.pcm(0x11)
        t.cuda.synchronize()
        a.run(d_pcm, i1, stream=S1)
        a.run(d_pcm, i2, stream=S2)
        r.run(d_images, p1, stream=S1)
        r.run(d_images, p2, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(i1, "stream 1")
        a.check(i2, "stream 2", fill=0x11)
        r.check(p1, "stream 1")
        r.check(p2, "stream 2", fill=0x11)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 6. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    a, r = WriteSet("packed"), ReadSet("packed", None)
    try:
        d_pcm, images, d_images, pcm = a.pcm(), a.images(), r.images(), r.pcm()
        w, rd = L().vga_wave_write_device_v, L().vga_wave_read_device_v
        st, base, rows = stream_ptr(), images.data_ptr() + EXTRA, pcm.data_ptr() + EXTRA
        assert rd(a.s._h, base, rows, st) == -4                                             # a set for writing refuses the read call
        assert w(r.s._h, rows, base, st) == -4                                              # ... and the other way round
        assert w(a.s._h, None, base, st) == -1
        assert w(a.s._h, d_pcm.data_ptr(), None, st) == -1
        assert w(a.s._h, d_pcm.data_ptr() + 1, base, st) == -1                              # alignment
        assert rd(r.s._h, None, rows, st) == -1
        assert rd(r.s._h, d_images.data_ptr(), None, st) == -1
        assert rd(r.s._h, d_images.data_ptr(), rows + 1, st) == -1
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(pcm) == JUNK16)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 7. the chain: WAV images -> rows -> a ragged ADX object, and back
def test_chain_through_a_ragged_adx_object():
    """vga_wave_read_device_v leaves its rows where RaggedAdx.encode_device takes them, in the SAME buffer: the bytes are
    CriAdxCodec.Encode's per channel; the other way, the rows RaggedAdx.decode_device leaves are vga_wave_write_device_v's input"""
    t = torch()
    from vgaudio_amd.criadx import CriAdxParameters, RaggedAdx
    rng = np.random.default_rng(0xC4A1)
    shapes = [(2, 16, 1000), (1, 16, 4097), (2, 8, 333), (6, 16, 64), (1, 8, 17), (2, 16, 31)]
    chans = [[rng.integers(-20000, 20000, n).astype(np.int16) for _ in range(nch)] for nch, bits, n in shapes]
    files = [po.wave_write(c, 48000)[1].tobytes() if bits == 16 else wc.wave8(c, 48000) for c, (nch, bits, n) in zip(chans, shapes)]
    pcm, offsets, infos = wave.read_files_device(files)
    counts = [i.sample_count for i in infos for _ in range(i.channel_count)]
    params = CriAdxParameters(SampleRate=48000)
    ragged = RaggedAdx(params, counts)
    try:
        assert list(ragged.pcm_offsets) == list(offsets)
        buffer = t.zeros(max(ragged.totals.pcm_samples, pcm.numel()), dtype=t.int16, device="cuda")
        buffer[:pcm.numel()] = pcm
        adx = t.zeros(ragged.totals.adx_bytes, dtype=t.uint8, device="cuda")
        ws = t.empty(max(ragged.totals.encode_workspace_bytes, ragged.totals.decode_workspace_bytes, 16), dtype=t.uint8, device="cuda")
        ragged.encode_device(buffer, adx, ws)
        got = host(adx)
        p = po.adx_params(sample_rate=48000)
        want_adx, decoded, c = [], [], 0
        for mine, (nch, bits, n) in zip(chans, shapes):
            rows = [wc.row_as_read(r, bits) for r in mine]
            if n:
                enc, _ = po.adx_encode_batch(np.stack(rows), p)
            for ch in range(nch):
                if n:
                    at = int(ragged.adx_offsets[c])
                    assert np.array_equal(got[at:at + enc.shape[1]], enc[ch]), ("encode", c)
                    decoded.append(po.adx_decode(enc[ch], n, p))
                else:
                    decoded.append(np.zeros(0, np.int16))
                c += 1
        # the other way: decode into a fresh buffer, write 16-bit files from it
        back, status = t.zeros_like(buffer), t.zeros(max(ragged.channels, 1), dtype=t.int32, device="cuda")
        ragged.decode_device(adx, back, ws, status)
        described = [_lib.WaveFileC(nch, 16, _lib.WaveParamsC(48000, n, 0, 0, 0)) for nch, bits, n in shapes]
        s = WaveFileSet(described)
        try:
            assert list(s.pcm_offsets) == list(ragged.pcm_offsets)
            images = t.full((s.totals.image_bytes,), JUNK, dtype=t.uint8, device="cuda")
            s.write_device(back, images)
            out, c = s.images(images), 0
            for k, (nch, bits, n) in enumerate(shapes):
                rc, want = po.wave_write(decoded[c:c + nch], 48000)
                assert rc == 0 and out[k] == want.tobytes(), ("write", k)
                c += nch
        finally:
            s.close()
    finally:
        ragged.close()


# ---------------------------------------------------------------- 8. the Python layer: files in, images out
def small_files():
    rng = np.random.default_rng(0x5EED)
    out = []
    for nch, n, rate, loop in ((1, 1000, 48000, None), (2, 777, 44100, (5, 700)), (2, 64, 48000, None), (1, 0, 32000, None),
                               (6, 1200, 44100, (32, 1100)), (2, 9000, 48000, (5, 600)), (1, 31, 22050, None)):
        f = Pcm16Format([rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(nch)], rate)
        if loop:
            f.WithLoop(True, loop[0], loop[1])
        out.append(f)
    return out


@pytest.mark.parametrize("codec", [wave.WaveCodec.Pcm16Bit, wave.WaveCodec.Pcm8Bit], ids=["pcm16", "pcm8"])
def test_write_files_is_the_writers_get_file(codec):
    files = small_files()
    got = wave.write_files(files, codec)
    assert len(got) == len(files)
    for k, f in enumerate(files):
        assert got[k] == wave.WaveWriter.GetFile(f, codec), ("file", k)
        if codec == wave.WaveCodec.Pcm16Bit:
            rc, want = po.wave_write(f.Channels, f.SampleRate, f.Looping, f.LoopStart, f.LoopEnd)
            assert rc == 0 and got[k] == want.tobytes(), ("oracle", k)
        else:
            assert got[k] == wc.wave8(f.Channels, f.SampleRate, f.Looping, f.LoopStart, f.LoopEnd), ("model", k)
    assert wave.write_files([], codec) == []
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        wave.write_files([files[0], "not a format"], codec)


def test_read_files_is_the_readers_read_format():
    files = [f for f in small_files() if f.SampleCount]                # (WaveReader refuses a file without samples)
    images = [po.wave_write(f.Channels, f.SampleRate, f.Looping, f.LoopStart, f.LoopEnd)[1].tobytes() for f in files]
    images.append(wc.wave8(files[1].Channels, 44100, True, 5, 700))
    got = wave.read_files(images)
    assert len(got) == len(images)
    for k, (image, fmt) in enumerate(zip(images[:-1], got)):
        one = wave.WaveReader.ReadFormat(image)
        assert (fmt.ChannelCount, fmt.SampleRate, fmt.SampleCount) == (one.ChannelCount, one.SampleRate, one.SampleCount)
        assert (fmt.Looping, fmt.LoopStart, fmt.LoopEnd) == (one.Looping, one.LoopStart, one.LoopEnd) == (
            files[k].Looping, files[k].LoopStart, files[k].LoopEnd)
        assert all(np.array_equal(x, y) for x, y in zip(fmt.Channels, one.Channels)), k
        assert all(np.array_equal(x, y) for x, y in zip(fmt.Channels, files[k].Channels)), k
    eight = wave.WaveReader.ReadPcm8Format(images[-1]).ToPcm16()
    assert all(np.array_equal(x, y) for x, y in zip(got[-1].Channels, eight.Channels)) and got[-1].LoopEnd == 700
    assert wave.read_files([]) == []


# ---------------------------------------------------------------- 9. offsets past 4 GiB
def test_offsets_past_4_gib():
    """Six files whose images lie at the caller's offsets around 2^32 bytes and whose rows lie behind 2^32 BYTES of d_pcm, both
    ways.  Both buffers are longer than 4 GiB, so an offset cut to 32 bits lands inside the allocation: wrong bytes in a window
    or changed junk outside them, not a fault."""
    t = torch()
    extent = 4 * GIB + (1 << 20)
    need(2 * extent)
    general = wc.first_general_channels(16)
    shapes = [(2, 16, 5000, None), (1, 16, 9001, (7, 9000)), (2, 8, 3001, None), (3, 16, 1000, None), (general, 16, 9, None), (6, 8, 2001, (0, 2000))]
    files = wc.files_of(shapes)
    rng = np.random.default_rng(0xFA4)
    rows = [rng.integers(-32768, 32768, n).astype(np.int16) for nch, bits, n, loop in shapes for _ in range(nch)]
    want, c = [], 0
    for nch, bits, n, loop in shapes:
        mine, looping = rows[c:c + nch], loop is not None
        ls, le = loop if looping else (0, 0)
        want.append(po.wave_write(mine, 44100, looping, ls, le)[1] if bits == 16 else np.frombuffer(wc.wave8(mine, 44100, looping, ls, le), np.uint8))
        c += nch
    sizes = [len(w) for w in want]
    # images: the first ends 3 bytes short of 2^32, the second straddles it, the others follow at odd offsets
    image_offs = [(1 << 32) - 1001 - sizes[0] - 3, (1 << 32) - 1001]
    for k in range(2, len(shapes)):
        image_offs.append(image_offs[-1] + sizes[k - 1] + 7)
    # rows: from 2^31 + 5 samples (2^32 + 10 bytes) on, at odd and even sample boundaries; the read side's rows behind them
    counts = wc.counts_of(files)
    write_offs = [(1 << 31) + o for o in wc.explicit_pcm_offsets(counts, start=5)]
    read_offs = [o + 200000 for o in write_offs]
    assert max(read_offs) * 2 + 20000 < extent and max(image_offs) + max(sizes) < extent
    pcm, images = FarBuffer(extent), FarBuffer(extent)
    s = r = None
    try:
        s = WaveFileSet(files, write_offs, image_offs)
        assert s.totals.pcm_samples * 2 <= extent and s.totals.image_bytes <= extent
        pcm_windows = [pcm.put(2 * o, row) for o, row in zip(write_offs, rows) if len(row)]
        _lib.check(L().vga_wave_write_device_v(s._h, pcm.ptr, images.ptr, stream_ptr()))
        t.cuda.synchronize()
        image_windows = []
        for k, (at, w) in enumerate(zip(image_offs, want)):
            assert np.array_equal(images.get(at, len(w)), w), ("image", k, shapes[k])
            image_windows.append((at, len(w)))
        assert images.untouched(image_windows) is None, images.changed
        assert pcm.untouched(pcm_windows) is None, pcm.changed
        # the other way, out of the images the set just wrote
        infos = [wc.parse(w) for w in want]
        r = WaveFileSet.from_infos(infos, read_offs, image_offs)
        _lib.check(L().vga_wave_read_device_v(r._h, images.ptr, pcm.ptr, stream_ptr()))
        t.cuda.synchronize()
        c = 0
        for k, (nch, bits, n, loop) in enumerate(shapes):
            for ch in range(nch):
                got = pcm.get(2 * read_offs[c], 2 * n, np.int16)
                assert np.array_equal(got, wc.row_as_read(rows[c], bits)), ("row", k, ch)
                pcm_windows.append((2 * read_offs[c], 2 * n))
                c += 1
        assert pcm.untouched(pcm_windows) is None, pcm.changed
        assert images.untouched(image_windows) is None, images.changed
    finally:
        for x in (s, r):
            if x is not None:
                x.close()
        release(pcm, images)
