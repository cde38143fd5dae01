"""include/vgaudio_hip_files/nw_pcm_files.h on the GPU: the images a set writes from rows against tests/nwstm_pcm_ref.py's
restatement of the reference's writers and against vga_nwstm_pcm_write_device for every file alone, for every named
configuration of tests/nw_pcm_files_cases.py, packed and with the caller's rows at odd samples and images on 16; the rows a set
reads against vga_nwstm_pcm_read_device and the restatement's parser, images packed and at odd bytes; all inside junk-filled
buffers whose every byte outside the rows / images is checked; a mixed reading set; the chain WAV images -> rows -> images ->
rows on the device; the PCM8 round trip; the forced general form; poison mode; a busy caller stream; two streams at once;
refused calls; the object's numbers; the Python mirror; offsets past 4 GiB.  tests/test_nw_pcm_files_host.py checks that
CASES names every function of the header."""
import ctypes as C

import numpy as np
import pytest

import nw_pcm_files_cases as nc
import nwstm_pcm_ref as ref
from far_memory import GIB, FarBuffer, need, release
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib, nwstm, wave
from vgaudio_amd.gcadpcm import Pcm16Format
from vgaudio_amd.nwstm import NwPcmFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_nw_pcm_files_layout_for": ["test_object_numbers_are_the_host_layouts", "test_write_files_is_the_writers_get_file"],
    "vga_nw_pcm_files_create": ["test_images_are_the_references_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_nw_pcm_files_create_from_infos": ["test_read_gives_the_per_file_and_the_references_rows", "test_a_mixed_set_is_taken_apart_in_one_call"],
    "vga_nw_pcm_files_destroy": ["test_images_are_the_references_and_the_per_file_calls"],
    "vga_nw_pcm_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_nw_pcm_files_offsets": ["test_object_numbers_are_the_host_layouts", "test_the_chain_stays_on_the_device"],
    "vga_nwstm_pcm_write_device_v": [
        "test_images_are_the_references_and_the_per_file_calls", "test_forced_general_form_gives_the_same_bytes",
        "test_the_chain_stays_on_the_device", "test_write_then_read_round_trips_pcm8", "test_an_empty_set_launches_nothing",
        "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_streams_at_once",
        "test_refused_calls_launch_nothing", "test_offsets_past_4_gib", "test_write_files_is_the_writers_get_file"],
    "vga_nwstm_pcm_read_device_v": [
        "test_read_gives_the_per_file_and_the_references_rows", "test_a_mixed_set_is_taken_apart_in_one_call",
        "test_forced_general_form_gives_the_same_bytes", "test_the_chain_stays_on_the_device",
        "test_write_then_read_round_trips_pcm8", "test_an_empty_set_launches_nothing", "test_bytes_do_not_depend_on_poison",
        "test_calls_on_a_busy_stream", "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_offsets_past_4_gib",
        "test_read_pcm_files_is_the_readers_read_format"],
    "vga_nw_pcm_files_write_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_nw_pcm_files_read_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_nw_pcm_files_stats": ["test_forced_general_form_gives_the_same_bytes", "test_object_numbers_are_the_host_layouts"],
    "vga_nw_pcm_files_force_general_this_thread": ["test_forced_general_form_gives_the_same_bytes"],
}

JUNK = 0xEE
EXTRA = 64                                                             # junk in front of and behind every buffer (keeps 16-byte alignment)
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin
NAMES = sorted(nc.CONFIGS)


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


def aligned_image_offsets(sizes):
    """every image on 16 bytes, gaps between them, the first not at 0"""
    return [o + 48 for o in nc.image_offsets_at(sizes, 0, gap=21)]


class WriteSet:
    """a named configuration's files as a set for writing: "packed", or "explicit" (rows at odd samples, images on 16 with gaps)"""

    def __init__(self, name, layout="packed"):
        self.name, self.codec = name, nc.CONFIGS[name][1]
        self.cases, self.rows, self.want = nc.reference(name)
        self.files = nc.files_of(self.cases)
        self.cfg, _ = nc.config_c(name)
        sizes = [len(w) for w in self.want]
        self.po = nc.explicit_pcm_offsets(nc.counts_of(self.cases)) if layout == "explicit" else None
        self.io = aligned_image_offsets(sizes) if layout == "explicit" else None
        self.s = NwPcmFileSet(self.files, self.cfg.target, self.configuration(), self.po, self.io)
        assert self.s.image_sizes == sizes

    def configuration(self):
        target, codec, endian, version, spi, _ = nc.CONFIGS[self.name]
        c = nwstm.BxstmConfiguration(Codec=nwstm.NwCodec(codec))
        if spi:
            c.SamplesPerInterleave = spi
        if endian is not None:
            c.Endianness = nwstm.Endianness(endian)
        if version:
            c.Version = nwstm.NwVersion.FromPacked(version)
        return c

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
        _lib.check(L().vga_nwstm_pcm_write_device_v(self.s._h, pcm.data_ptr(), images.data_ptr() + EXTRA, stream_ptr(stream)))
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
                raise AssertionError((what, self.name, "file", f, self.cases[f], "first bad byte", int(bad[0]), "of", len(want), "bad bytes", len(bad)))
            got[at:at + len(want)] = fill
        assert np.all(got == fill), (what, "bytes outside the images were written", np.flatnonzero(got != fill)[:8])


_parsed = {}


def read_side(name):
    """(images, infos, want rows per file) of a named configuration, or of the mixed set: the rows from the restatement's parser"""
    if name not in _parsed:
        images = nc.mixed_read_side()[0] if name == "mixed" else nc.reference(name)[2]
        infos, want = [nc.parse(i) for i in images], []
        for image in images:
            p = ref.parse_image(image.tobytes())
            want.append(p["channels"] if p["codec"] == nc.PCM16 else [ref.decode_signed(c) for c in p["channels"]])
        _parsed[name] = (images, infos, want)
    return _parsed[name]


class ReadSet:
    """a configuration's images as a set for reading: rows "packed" or "explicit", images packed or at a residue of 16"""

    def __init__(self, name, rows="packed", residue=None):
        self.name = name
        self.images_, self.infos, self.want = read_side(name)
        sizes = [len(i) for i in self.images_]
        self.po = nc.explicit_pcm_offsets([[i.sample_count] * i.channel_count for i in self.infos]) if rows == "explicit" else None
        self.io = nc.image_offsets_at(sizes, residue) if residue is not None else None
        self.s = NwPcmFileSet.from_infos(self.infos, self.po, self.io)
        assert self.s.image_sizes == sizes                              # (the audio ends the file)

    def close(self):
        self.s.close()

    def images(self, fill=JUNK):
        a = np.full(self.s.totals.image_bytes, fill, np.uint8)
        for image, at in zip(self.images_, self.s.image_offsets):
            a[at:at + len(image)] = image
        return dev(a)

    def pcm(self, fill=JUNK):
        return torch().full((self.s.totals.pcm_samples + EXTRA,), int(junk16(fill)), dtype=torch().int16, device="cuda")

    def run(self, images, pcm, stream=None):
        _lib.check(L().vga_nwstm_pcm_read_device_v(self.s._h, images.data_ptr(), pcm.data_ptr() + EXTRA, stream_ptr(stream)))
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
                assert len(rows[ch]) == n
                if not np.array_equal(got[at:at + n], rows[ch]):
                    bad = np.flatnonzero(got[at:at + n] != rows[ch])
                    raise AssertionError((what, self.name, "file", f, "channel", ch, "of", info.channel_count, "codec", info.codec,
                                          "first bad sample", int(bad[0]), "of", n, "bad samples", len(bad)))
                got[at:at + n] = j
                c += 1
        assert np.all(got == j), (what, "samples outside the rows were written", np.flatnonzero(got != j)[:8])


# ---------------------------------------------------------------- 1. write
def per_file_images(a):
    """vga_nwstm_pcm_write_device for every file alone with tracks = NULL, from rows staged at a pitch"""
    t = torch()
    at = 0
    for f, file in enumerate(a.files):
        n, nch = file.sample_count, file.channels
        pitch = n + 5
        staged = np.full((nch, pitch), junk16(JUNK), np.int16)
        for c in range(nch):
            staged[c, :n] = a.rows[at + c]
        d_rows = dev(staged)
        d_file = t.full((len(a.want[f]) + 32,), JUNK, dtype=t.uint8, device="cuda")
        p = NwPcmFileSet.file_params(file, a.cfg)
        _lib.check(L().vga_nwstm_pcm_write_device(C.byref(p), a.codec, nch, 1, None, d_rows.data_ptr(), 0, pitch, d_file.data_ptr(),
                                                  len(a.want[f]), stream_ptr()))
        got = host(d_file)
        assert np.array_equal(got[:len(a.want[f])], a.want[f]) and np.all(got[len(a.want[f]):] == JUNK), ("per-file call", a.name, f)
        at += nch


@pytest.mark.parametrize("layout", ["packed", "explicit"])
@pytest.mark.parametrize("name", NAMES)
def test_images_are_the_references_and_the_per_file_calls(name, layout):
    t = torch()
    a = WriteSet(name, layout)
    try:
        if layout == "explicit":
            assert any(o % 8 for o in a.s.pcm_offsets) and all(o % 16 == 0 for o in a.s.image_offsets)
            assert a.s.stats()[1] > 0, "rows off 8 samples take the general form"
        images = a.run(a.pcm(), a.images())
        t.cuda.synchronize()
        a.check(images, layout)
        if layout == "packed":
            per_file_images(a)
    finally:
        a.close()


# ---------------------------------------------------------------- 2. read
_per_file_checked = set()


def want_is_the_per_file_calls(r):
    """`want`, the restatement's rows every read result is compared with, IS what vga_nwstm_pcm_read_device delivers for every
    image alone: shown once per configuration"""
    if r.name in _per_file_checked:
        return
    t = torch()
    for f, (image, info, want) in enumerate(zip(r.images_, r.infos, r.want)):
        n, nch = info.sample_count, info.channel_count
        if n == 0:
            continue
        d_file = dev(image)
        out = t.full((nch, n + 3), int(junk16(JUNK)), dtype=t.int16, device="cuda")
        _lib.check(L().vga_nwstm_pcm_read_device(C.byref(info), d_file.data_ptr(), len(image), 1, out.data_ptr(), 0, n + 3, stream_ptr()))
        got = host(out)
        assert all(np.array_equal(got[ch, :n], want[ch]) for ch in range(nch)) and np.all(got[:, n:] == junk16(JUNK)), ("per-file call", r.name, f)
    _per_file_checked.add(r.name)


@pytest.mark.parametrize("rows,residue", [("packed", None), ("explicit", 1), ("packed", 7)])
@pytest.mark.parametrize("name", NAMES)
def test_read_gives_the_per_file_and_the_references_rows(name, rows, residue):
    t = torch()
    r = ReadSet(name, rows, residue)
    try:
        assert residue is None or all(o % 16 == residue for o in r.s.image_offsets)
        if residue is not None or rows == "explicit":
            assert r.s.stats()[0] == 0, "odd image offsets and rows off 8 samples take the general form"
        pcm = r.run(r.images(), r.pcm())
        t.cuda.synchronize()
        r.check(pcm, (rows, residue))
        # the rows are also the samples the files were written from, cut where a looping file is cut
        cases, source, _ = nc.reference(name)
        c = 0
        for (nch, n, looping, ls, le), want in zip(cases, r.want):
            for ch in range(nch):
                assert np.array_equal(want[ch], nc.row_as_read(source[c], nc.CONFIGS[name][1], le if looping else n))
                c += 1
        want_is_the_per_file_calls(r)
    finally:
        r.close()


def test_a_mixed_set_is_taken_apart_in_one_call():
    """BRSTM PCM16, BCSTM PCM8 and BFSTM PCM16 little-endian files in ONE set"""
    t = torch()
    r = ReadSet("mixed")
    try:
        kinds = {(i.target, i.codec, i.endianness) for i in r.infos}
        assert {(nc.RSTM, nc.PCM16, 1), (nc.CSTM, nc.PCM8, 0), (nc.FSTM, nc.PCM16, 0), (nc.FSTM, nc.PCM8, 1)} <= kinds
        st = r.s.stats()
        assert st[0] > 0 and st[1] > 0, st
        pcm = r.run(r.images(), r.pcm())
        t.cuda.synchronize()
        r.check(pcm, "mixed")
    finally:
        r.close()


# ---------------------------------------------------------------- 3. forms
@pytest.mark.parametrize("name", NAMES)
def test_forced_general_form_gives_the_same_bytes(name):
    t = torch()
    a, r = WriteSet(name), ReadSet(name)
    try:
        mixed_w, mixed_r = a.s.stats(), r.s.stats()
        assert L().vga_nw_pcm_files_force_general_this_thread(1) == 0
        try:
            forced_w, forced_r = a.s.stats(), r.s.stats()
            assert forced_w[0] == forced_w[2] == 0 and forced_w[1] == mixed_w[0] + mixed_w[1] and forced_w[3] == mixed_w[2] + mixed_w[3]
            assert forced_r[0] == forced_r[2] == 0 and forced_r[1] == mixed_r[0] + mixed_r[1] and forced_r[3] == mixed_r[2] + mixed_r[3]
            images = a.run(a.pcm(), a.images())
            pcm = r.run(r.images(), r.pcm())
            t.cuda.synchronize()
        finally:
            assert L().vga_nw_pcm_files_force_general_this_thread(0) == 1
        a.check(images, "forced general")
        r.check(pcm, "forced general")
        assert a.s.stats() == mixed_w
        # a d_pcm that is not on 16 bytes takes the general form for every file too: the same bytes
        shifted = t.full((a.s.totals.pcm_samples + 8,), int(junk16(JUNK)), dtype=t.int16, device="cuda")
        shifted[1:1 + a.s.totals.pcm_samples] = a.pcm()
        again = a.images()
        _lib.check(L().vga_nwstm_pcm_write_device_v(a.s._h, shifted.data_ptr() + 2, again.data_ptr() + EXTRA, stream_ptr()))
        t.cuda.synchronize()
        assert t.equal(again, images)
    finally:
        r.close()
        a.close()


def test_object_numbers_are_the_host_layouts():
    for name, layout in (("rstm16_default", "packed"), ("cstm8_be_i1001", "explicit"), ("fstm16_le_i5", "packed")):
        a = WriteSet(name, layout)
        try:
            fc, po_, io_, tot = NwPcmFileSet.layout(a.files, a.cfg.target, a.configuration(), a.po, a.io)
            assert list(a.s.first_channel) == list(fc) and list(a.s.pcm_offsets) == list(po_) and list(a.s.image_offsets) == list(io_)
            assert all(getattr(a.s.totals, k) == getattr(tot, k) for k, _ in tot._fields_)
            assert [list(x) for x in a.s.offsets()] == [list(fc), list(po_), list(io_)]
            items = [i for i in NwPcmFileSet.write_items(a.files, a.cfg.target, a.configuration(), a.po, a.io) if i.form != nc.HEADER_ITEM]
            st = a.s.stats()
            assert (st[2], st[3]) == (sum(i.form == nc.VECTOR for i in items), sum(i.form == nc.GENERAL for i in items))
            assert st[0] == len({i.file for i in items if i.form == nc.VECTOR}) and st[1] == len({i.file for i in items if i.form == nc.GENERAL})
        finally:
            a.close()
    r = ReadSet("mixed", "explicit", 4)
    try:
        items = NwPcmFileSet.read_items(r.infos, r.po, r.io)
        st = r.s.stats()
        assert (st[2], st[3]) == (sum(i.form == nc.VECTOR for i in items), sum(i.form == nc.GENERAL for i in items))
        assert r.s.channels == sum(i.channel_count for i in r.infos) and r.s.files == len(r.infos)
        assert list(r.s.pcm_offsets) == r.po and list(r.s.image_offsets) == r.io
    finally:
        r.close()


def test_an_empty_set_launches_nothing():
    t = torch()
    s, r = NwPcmFileSet([], nc.RSTM, nwstm.BxstmConfiguration(Codec=nwstm.NwCodec.Pcm16Bit)), NwPcmFileSet.from_infos([])
    try:
        assert (s.totals.files, s.totals.channels, s.totals.pcm_samples, s.totals.image_bytes) == (0, 0, 128, 256)
        pcm = t.full((128,), int(junk16(JUNK)), dtype=t.int16, device="cuda")
        images = t.full((256,), JUNK, dtype=t.uint8, device="cuda")
        s.write(pcm, images)
        r.read(images, pcm)
        assert L().vga_nwstm_pcm_write_device_v(s._h, None, None, stream_ptr()) == 0
        assert L().vga_nwstm_pcm_read_device_v(r._h, None, None, stream_ptr()) == 0
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(pcm) == junk16(JUNK)) and s.stats() == (0, 0, 0, 0)
    finally:
        s.close()
        r.close()


# ---------------------------------------------------------------- 4. the chain and the round trip
def test_the_chain_stays_on_the_device():
    """WAV images -> wave.read_files_device -> NwPcmFileSet.write from the SAME tensor -> from_infos(...).read: the samples"""
    t = torch()
    from oracle import pyoracle as po
    rng = np.random.default_rng(0xC4A2)
    shapes = [(2, 1000), (1, 4097), (2, 9000), (6, 64), (1, 17), (2, 31)]
    chans = [[rng.integers(-32768, 32768, n).astype(np.int16) for _ in range(nch)] for nch, n in shapes]
    wavs = [po.wave_write(c, 48000)[1].tobytes() for c in chans]
    pcm, offsets, infos = wave.read_files_device(wavs)
    files = [(i.channel_count, i.sample_rate, i.sample_count) for i in infos]
    for target in (nc.RSTM, nc.FSTM):
        s = NwPcmFileSet(files, target, nwstm.BxstmConfiguration(Codec=nwstm.NwCodec.Pcm16Bit))
        try:
            assert list(s.offsets()[1]) == list(offsets) and s.totals.pcm_samples <= pcm.numel()
            images = t.full((s.totals.image_bytes,), JUNK, dtype=t.uint8, device="cuda")
            s.write(pcm, images)
            parsed = [nwstm.parse_pcm(b) for b in s.images(images)]
            r = NwPcmFileSet.from_infos(parsed, image_offsets=[int(o) for o in s.image_offsets])
            try:
                back = t.full((r.totals.pcm_samples,), int(junk16(JUNK)), dtype=t.int16, device="cuda")
                r.read(images, back)
                got, c = host(back), 0
                for mine in chans:
                    for row in mine:
                        at = int(r.pcm_offsets[c])
                        assert np.array_equal(got[at:at + len(row)], row), (target, c)
                        c += 1
            finally:
                r.close()
        finally:
            s.close()


def test_write_then_read_round_trips_pcm8():
    """DecodeSigned(EncodeSigned(x)) for every row, over the same image buffer"""
    t = torch()
    a = WriteSet("fstm8_be_default")
    try:
        images = a.run(a.pcm(), a.images())
        t.cuda.synchronize()
        parsed = [nwstm.parse_pcm(b) for b in a.s.images(host(images)[EXTRA:-EXTRA])]
        r = NwPcmFileSet.from_infos(parsed, image_offsets=[int(o) for o in a.s.image_offsets])
        try:
            back = t.full((r.totals.pcm_samples,), int(junk16(JUNK)), dtype=t.int16, device="cuda")
            _lib.check(L().vga_nwstm_pcm_read_device_v(r._h, images.data_ptr() + EXTRA, back.data_ptr(), stream_ptr()))
            got, c = host(back).copy(), 0
            for nch, n, looping, ls, le in a.cases:
                stored = le if looping else n
                for ch in range(nch):
                    at = int(r.pcm_offsets[c])
                    assert np.array_equal(got[at:at + stored], ref.decode_signed(ref.encode_signed(a.rows[c][:stored]))), c
                    got[at:at + stored] = junk16(JUNK)
                    c += 1
            assert np.all(got == junk16(JUNK))
        finally:
            r.close()
    finally:
        a.close()


# ---------------------------------------------------------------- 5. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    t = torch()
    old = L().vga_testing_poison_allocations(value)
    try:
        for name in ("rstm16_default", "cstm8_be_i1001"):
            a = WriteSet(name)                                         # (created under the mode: its tables are poisoned first)
            try:
                images = a.run(a.pcm(value ^ 0x3C), a.images(value ^ 0x3C))
                t.cuda.synchronize()
                a.check(images, ("poison", value), fill=value ^ 0x3C)
            finally:
                a.close()
        r = ReadSet("mixed", "packed", 1)
        try:
            pcm = r.run(r.images(value), r.pcm(value ^ 0x3C))
            t.cuda.synchronize()
            r.check(pcm, ("poison", value), fill=value ^ 0x3C)
        finally:
            r.close()
    finally:
        t.cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 6. streams
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
    a, r = WriteSet("rstm16_default"), ReadSet("mixed")
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
    a, r = WriteSet("cstm8_be_i1001", "explicit"), ReadSet("mixed", "explicit", 8)
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


# ---------------------------------------------------------------- 7. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    a, r = WriteSet("rstm16_i8"), ReadSet("rstm16_i8")
    try:
        d_pcm, images, d_images, pcm = a.pcm(), a.images(), r.images(), r.pcm()
        w, rd = L().vga_nwstm_pcm_write_device_v, L().vga_nwstm_pcm_read_device_v
        st, base, rows = stream_ptr(), images.data_ptr() + EXTRA, pcm.data_ptr() + EXTRA
        assert rd(a.s._h, base, rows, st) == -4                                             # a set for writing refuses the read call
        assert w(r.s._h, rows, base, st) == -4                                              # ... and the other way round
        assert w(a.s._h, None, base, st) == -1
        assert w(a.s._h, d_pcm.data_ptr(), None, st) == -1
        assert w(a.s._h, d_pcm.data_ptr() + 1, base, st) == -1                              # alignment
        assert w(a.s._h, d_pcm.data_ptr(), base + 8, st) == -1
        assert rd(r.s._h, None, rows, st) == -1
        assert rd(r.s._h, d_images.data_ptr(), None, st) == -1
        assert rd(r.s._h, d_images.data_ptr(), rows + 1, st) == -1
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(pcm) == junk16(JUNK))
    finally:
        r.close()
        a.close()


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


def writer_of(target, configuration):
    return nwstm.BrstmWriter(configuration) if target == nwstm.NwTarget.Revolution else nwstm.BCFstmWriter(target, configuration)


@pytest.mark.parametrize("codec", [nwstm.NwCodec.Pcm16Bit, nwstm.NwCodec.Pcm8Bit], ids=["pcm16", "pcm8"])
@pytest.mark.parametrize("target", [nwstm.NwTarget.Revolution, nwstm.NwTarget.Ctr, nwstm.NwTarget.Cafe], ids=["brstm", "bcstm", "bfstm"])
def test_write_files_is_the_writers_get_file(target, codec):
    files = small_files()
    configuration = nwstm.BxstmConfiguration(Codec=codec)
    got = nwstm.write_files(files, target, configuration)
    assert len(got) == len(files)
    for k, f in enumerate(files):
        assert got[k] == writer_of(target, configuration).GetFile(f), ("file", k)
    assert nwstm.write_files([], target, configuration) == []
    with pytest.raises(_lib.ArgumentError, match=r"file 1\b"):
        nwstm.write_files([files[0], "not a format"], target, configuration)


def test_read_pcm_files_is_the_readers_read_format():
    files = small_files()
    images, readers = [], []
    for target, codec in ((nwstm.NwTarget.Revolution, nwstm.NwCodec.Pcm16Bit), (nwstm.NwTarget.Ctr, nwstm.NwCodec.Pcm8Bit),
                          (nwstm.NwTarget.Cafe, nwstm.NwCodec.Pcm16Bit)):
        configuration = nwstm.BxstmConfiguration(Codec=codec)
        for f in files[:3] + files[4:6]:
            images.append(writer_of(target, configuration).GetFile(f))
            readers.append(nwstm.BrstmReader() if target == nwstm.NwTarget.Revolution else nwstm.BCFstmReader())
    got = nwstm.read_pcm_files(images)
    assert len(got) == len(images)
    for k, (image, reader, fmt) in enumerate(zip(images, readers, got)):
        one = reader.ReadAnyFormat(image)
        if not isinstance(one, Pcm16Format):
            one = one.ToPcm16()
        assert (fmt.ChannelCount, fmt.SampleRate, fmt.SampleCount) == (one.ChannelCount, one.SampleRate, one.SampleCount), k
        assert (fmt.Looping, fmt.LoopStart, fmt.LoopEnd) == (one.Looping, one.LoopStart, one.LoopEnd), k
        assert all(np.array_equal(x, y) for x, y in zip(fmt.Channels, one.Channels)), k
    assert nwstm.read_pcm_files([]) == []


# ---------------------------------------------------------------- 9. offsets past 4 GiB
def test_offsets_past_4_gib():
    """Six files whose images lie at the caller's offsets around 2^32 bytes and whose rows lie behind 2^32 BYTES of d_pcm, both
    ways.  Both buffers are longer than 4 GiB, so an offset cut to 32 bits lands inside the allocation: wrong bytes in a window
    or changed junk outside them, not a fault."""
    t = torch()
    extent = 4 * GIB + (1 << 20)
    need(2 * extent)
    cases = [(2, 5000, 0, 0, 0), (1, 9001, 1, 7, 9000), (2, 3001, 0, 0, 0), (3, 1000, 0, 0, 0), (255, 9, 0, 0, 0), (6, 2001, 1, 0, 2000)]
    files = nc.files_of(cases)
    rng = np.random.default_rng(0xFA5)
    rows = [rng.integers(-32768, 32768, n).astype(np.int16) for nch, n, _, _, _ in cases for _ in range(nch)]
    configuration = nwstm.BxstmConfiguration(Codec=nwstm.NwCodec.Pcm16Bit)           # BRSTM, 4096 samples per interleave: vector
    want, c = [], 0
    for nch, n, looping, ls, le in cases:
        want.append(np.frombuffer(bytes(ref.build_image(nc.RSTM, nc.PCM16, nc.RATE, rows[c:c + nch], bool(looping), ls, le)), np.uint8))
        c += nch
    sizes = [len(w) for w in want]
    # images: the first ends short of 2^32, the second straddles it, the others follow; all on 16 bytes
    image_offs = [(1 << 32) - 1008 - nc.up(sizes[0], 16) - 16, (1 << 32) - 1008]
    for k in range(2, len(cases)):
        image_offs.append(nc.up(image_offs[-1] + sizes[k - 1] + 7, 16))
    # rows: from 2^31 + 8 samples on; every other file's rows on 8 samples (vector), the others at odd boundaries (general)
    counts = nc.counts_of(cases)
    write_offs, at = [], (1 << 31) + 8
    for f, per in enumerate(counts):
        for n in per:
            at = nc.up(at, 8) + (f % 2) * 3
            write_offs.append(at)
            at += n + 5
    read_offs = [o + 400000 for o in write_offs]
    assert max(read_offs) * 2 + 20000 < extent and max(image_offs) + max(sizes) < extent
    pcm, images = FarBuffer(extent), FarBuffer(extent)
    s = r = None
    try:
        s = NwPcmFileSet(files, nc.RSTM, configuration, write_offs, image_offs)
        assert s.totals.pcm_samples * 2 <= extent and s.totals.image_bytes <= extent and min(s.stats()) > 0, s.stats()
        pcm_windows = [pcm.put(2 * o, row) for o, row in zip(write_offs, rows) if len(row)]
        _lib.check(L().vga_nwstm_pcm_write_device_v(s._h, pcm.ptr, images.ptr, stream_ptr()))
        t.cuda.synchronize()
        image_windows = []
        for k, (at, w) in enumerate(zip(image_offs, want)):
            assert np.array_equal(images.get(at, len(w)), w), ("image", k, cases[k])
            image_windows.append((at, len(w)))
        assert images.untouched(image_windows) is None, images.changed
        assert pcm.untouched(pcm_windows) is None, pcm.changed
        # the other way, out of the images the set just wrote
        infos = [nc.parse(w) for w in want]
        r = NwPcmFileSet.from_infos(infos, read_offs, image_offs)
        assert min(r.stats()) > 0, r.stats()
        _lib.check(L().vga_nwstm_pcm_read_device_v(r._h, images.ptr, pcm.ptr, stream_ptr()))
        t.cuda.synchronize()
        c = 0
        for k, (nch, n, looping, ls, le) in enumerate(cases):
            stored = le if looping else n
            for ch in range(nch):
                got = pcm.get(2 * read_offs[c], 2 * stored, np.int16)
                assert np.array_equal(got, rows[c][:stored]), ("row", k, ch)
                pcm_windows.append((2 * read_offs[c], 2 * stored))
                c += 1
        assert pcm.untouched(pcm_windows) is None, pcm.changed
        assert images.untouched(image_windows) is None, images.changed
    finally:
        for x in (s, r):
            if x is not None:
                x.close()
        release(pcm, images)
