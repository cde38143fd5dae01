"""include/vgaudio_hip/hca_files.h on the GPU: the images of a set of HCA files of different shapes and keys against the oracle
(CryptFrame, then HcaWriter) and against vga_hca_crypt_device plus vga_hca_write_device file by file; the frames and bad-CRC
counts read back against the oracle and against vga_hca_read_device plus vga_hca_crypt_device; both inside junk-filled
buffers whose every byte outside the images / streams / rounding zeros is checked, the inputs included; write ->
vga_hca_parse -> read with the inverse tables; the forced general form against the mixed forms; poison mode; a busy caller
stream; two streams at once; hca.write_files / hca.read_files against the oracle's encoder, crypt, writer and decoder.  The
cases are tests/hca_files_cases.py's; tests/test_hca_files_host.py checks that CASES names every function of the header."""
import ctypes as C

import numpy as np
import pytest

import hca_files_cases as hc
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd import crihca, hca
from vgaudio_amd.gcadpcm import Pcm16Format
from vgaudio_amd.hca import HcaFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_hca_files_layout_for": ["test_object_numbers_are_the_host_layouts", "test_write_files_is_the_writers_get_file"],
    "vga_hca_files_create": ["test_images_are_the_oracles_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_hca_files_create_from_infos": ["test_read_gives_the_oracles_and_the_per_file_frames", "test_write_parse_read_returns_the_frames"],
    "vga_hca_files_destroy": ["test_images_are_the_oracles_and_the_per_file_calls"],
    "vga_hca_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_hca_files_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_hca_write_device_v": [
        "test_images_are_the_oracles_and_the_per_file_calls", "test_write_parse_read_returns_the_frames",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_write_files_is_the_writers_get_file"],
    "vga_hca_read_device_v": [
        "test_read_gives_the_oracles_and_the_per_file_frames", "test_write_parse_read_returns_the_frames",
        "test_read_without_counts", "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison",
        "test_calls_on_a_busy_stream", "test_two_streams_at_once", "test_refused_calls_launch_nothing",
        "test_read_files_is_the_readers_read_format"],
    "vga_hca_files_write_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_hca_files_read_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_hca_files_stats": ["test_forced_general_form_gives_the_same_bytes", "test_object_numbers_are_the_host_layouts"],
    "vga_hca_files_force_general_this_thread": ["test_forced_general_form_gives_the_same_bytes"],
}

JUNK = 0xEE
EXTRA = 64                                                             # junk in front of and behind every buffer (keeps 16-byte alignment)
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin
CRYPT_MAX = 4096                                                       # vga_hca_crypt_device's largest frame


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


def u8(a):
    return a.ctypes.data_as(_lib.u8p)


_reference = {}


def reference():
    """the files, the keys' tables, the frames to write (some damaged) with the oracle's image of every file, and the images
    to read (some stored frames damaged) with the oracle's frames and bad-CRC counts: computed once, never changed"""
    if not _reference:
        dec, enc = hc.key_tables()
        cases = hc.CASES
        frames = hc.input_frames(cases, hc.BAD_FRAMES)
        want = []
        for case, fr in zip(cases, frames):
            rc, image = hc.oracle_image(case, fr, enc)
            assert rc == 0
            want.append(image)
        stored, infos, back, bad = [], [], [], []
        for i, case in enumerate(cases):
            rc, image = hc.oracle_image(case, hc.valid_frames(1000 + i, case[0], case[1]), enc)
            assert rc == 0
            info = hca.parse(image.tobytes())
            for f, k in hc.BAD_FRAMES:
                if f == i:
                    hc.damage(image[info.frames_offset:], case[0], k)
            out, n = hc.oracle_read(image, info.frames_offset, case[0], case[1], dec[case[8]] if case[8] >= 0 else None)
            stored.append(image)
            infos.append(info)
            back.append(out)
            bad.append(n)
        assert bad == [sum(1 for f, _ in hc.BAD_FRAMES if f == i) for i in range(len(cases))] and sum(bad) == len(hc.BAD_FRAMES)
        for a in frames + want + stored + back + [dec, enc]:
            a.setflags(write=False)
        _reference.update(files=hc.files_of(cases), dec=dec, enc=enc, frames=frames, want=want, stored=stored, infos=infos, back=back, bad=bad)
    return _reference


def frame_offsets(name, files):
    return {"packed": None, "explicit": hc.explicit_frame_offsets(files), "explicit_gaps": hc.explicit_frame_offsets(files, 12)}[name]


class WriteSet:
    def __init__(self, offsets_name="packed"):
        r = reference()
        self.files, self.frames, self.want = r["files"], r["frames"], r["want"]
        self.offs = frame_offsets(offsets_name, self.files)
        self.s = HcaFileSet(self.files, self.offs, r["enc"])

    def close(self):
        self.s.close()

    def source(self, fill=JUNK):
        """the streams inside a junk-filled buffer: junk in the rounding, between the streams, in the slack and around"""
        a = np.full(self.s.totals.frame_bytes + 2 * EXTRA, fill, np.uint8)
        for at, fr in zip(self.s.frame_offsets, self.frames):
            a[EXTRA + at:EXTRA + at + len(fr)] = fr
        return dev(a)

    def images(self, fill=JUNK):
        return torch().full((self.s.totals.image_bytes + 2 * EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def run(self, source, images, stream=None):
        _lib.check(L().vga_hca_write_device_v(self.s._h, source.data_ptr() + EXTRA, images.data_ptr() + EXTRA, stream_ptr(stream)))
        return images

    def check(self, images, what, fill=JUNK, source=None):
        """every image is the oracle's, every other byte of the buffer is what it was, and so is every byte of the frames"""
        got = host(images).copy()
        for f, (at, want) in enumerate(zip(self.s.image_offsets, self.want)):
            mine = got[EXTRA + at:EXTRA + at + len(want)]
            assert np.array_equal(mine, want), (what, "file", f, hc.CASES[f], int(np.flatnonzero(mine != want)[0]))
            mine[:] = fill
        assert np.all(got == fill), (what, "bytes outside the images", np.flatnonzero(got != fill)[:8])
        if source is not None:
            assert np.array_equal(host(source), host(self.source(fill))), (what, "d_frames was written")


class ReadSet:
    def __init__(self, image_offsets="packed", offsets_name="packed", keyed=True):
        r = reference()
        self.r, self.infos, self.keyed = r, r["infos"], keyed
        sizes = [len(s) for s in r["stored"]]
        self.image_offs = hc.odd_image_offsets(sizes) if image_offsets == "odd" else None
        self.offs = frame_offsets(offsets_name, r["files"])
        keys = [c[8] for c in hc.CASES] if keyed else None
        self.s = HcaFileSet.from_infos(self.infos, self.image_offs, keys, r["dec"] if keyed else None, self.offs)
        self.back = r["back"] if keyed else [s[i.frames_offset:] for s, i in zip(r["stored"], self.infos)]

    def close(self):
        self.s.close()

    def images(self, fill=JUNK):
        a = np.full(self.s.totals.image_bytes + 2 * EXTRA, fill, np.uint8)
        for at, image in zip(self.s.image_offsets, self.r["stored"]):
            a[EXTRA + at:EXTRA + at + len(image)] = image
        return dev(a)

    def frames(self, fill=JUNK):
        return torch().full((self.s.totals.frame_bytes + 2 * EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def counts(self):
        return torch().zeros(self.s.files, dtype=torch().int32, device="cuda")

    def run(self, images, frames, bad, stream=None):
        _lib.check(L().vga_hca_read_device_v(self.s._h, images.data_ptr() + EXTRA, frames.data_ptr() + EXTRA,
                                             bad.data_ptr() if bad is not None else None, stream_ptr(stream)))

    def check(self, frames, bad, what, fill=JUNK, images=None, times=1):
        got = host(frames).copy()
        for f, (at, want) in enumerate(zip(self.s.frame_offsets, self.back)):
            mine = got[EXTRA + at:EXTRA + at + len(want)]
            assert np.array_equal(mine, want), (what, "file", f, hc.CASES[f], int(np.flatnonzero(mine != want)[0]) // hc.CASES[f][0])
            mine[:] = fill
            pad = got[EXTRA + at + len(want):EXTRA + at + hc.up(len(want), 4)]
            assert np.all(pad == 0), (what, "rounding zeros of file", f)
            pad[:] = fill
        assert np.all(got == fill), (what, "bytes outside the streams", np.flatnonzero(got != fill)[:8])
        if bad is not None:
            assert list(host(bad)) == [times * n for n in self.r["bad"]], (what, "bad-CRC counts")
        if images is not None:
            assert np.array_equal(host(images), host(self.images(fill))), (what, "d_images was written")


# ---------------------------------------------------------------- 1. write
def per_file_image(case, f, frames, enc):
    """vga_hca_crypt_device (keyed) then vga_hca_write_device, on a copy"""
    t = torch()
    h = f.hca
    n = h.frame_count * h.frame_size
    d = t.zeros(n + 8, dtype=t.uint8, device="cuda")
    d[:n] = dev(frames)
    if f.key >= 0:
        _lib.check(L().vga_hca_crypt_device(d.data_ptr(), n + 8, 1, h.frame_count, h.frame_size, u8(enc[f.key]), stream_ptr()))
    size = h.header_size + n
    out = t.full((size + 16,), JUNK, dtype=t.uint8, device="cuda")
    _lib.check(L().vga_hca_write_device(C.byref(h), d.data_ptr(), n + 8, 1, f.comment, f.volume, f.encryption_type, f.encrypted_ids,
                                        out.data_ptr(), size, stream_ptr()))
    return host(out)[:size]


@pytest.mark.parametrize("offsets_name", ["packed", "explicit", "explicit_gaps"])
def test_images_are_the_oracles_and_the_per_file_calls(offsets_name):
    a = WriteSet(offsets_name)
    try:
        source = a.source()
        images = a.run(source, a.images())
        torch().cuda.synchronize()
        a.check(images, offsets_name, source=source)
        if offsets_name == "packed":
            got, compared = a.s.images(images[EXTRA:]), 0
            for i, (case, f) in enumerate(zip(hc.CASES, a.files)):
                if f.key >= 0 and case[0] > CRYPT_MAX:
                    continue                                           # (the per-file crypt call stops at 4096-byte frames)
                assert got[i] == per_file_image(case, f, a.frames[i], reference()["enc"]).tobytes(), ("per-file", i, case)
                compared += 1
            assert compared == len(hc.CASES) - 2
    finally:
        a.close()


# ---------------------------------------------------------------- 2. read
def per_file_frames(info, case, image, dec):
    """vga_hca_read_device, then vga_hca_crypt_device if the file has a key: (frames, bad-CRC count)"""
    t = torch()
    fs, fc = case[0], case[1]
    n = fs * fc
    pitch = hc.up(n + 8, 4)
    d_file = dev(np.concatenate([np.zeros(3, np.uint8), image]))      # (at an odd address)
    out, bad = t.zeros(pitch, dtype=t.uint8, device="cuda"), t.zeros(1, dtype=t.int32, device="cuda")
    _lib.check(L().vga_hca_read_device(C.byref(info), d_file.data_ptr() + 3, len(image), 1, out.data_ptr(), pitch, bad.data_ptr(), stream_ptr()))
    if case[8] >= 0:
        _lib.check(L().vga_hca_crypt_device(out.data_ptr(), pitch, 1, fc, fs, u8(dec[case[8]]), stream_ptr()))
    return host(out)[:n], int(host(bad)[0])


@pytest.mark.parametrize("image_offsets,offsets_name", [("packed", "packed"), ("odd", "explicit"), ("odd", "explicit_gaps")])
def test_read_gives_the_oracles_and_the_per_file_frames(image_offsets, offsets_name):
    r = ReadSet(image_offsets, offsets_name)
    try:
        images, frames, bad = r.images(), r.frames(), r.counts()
        r.run(images, frames, bad)
        torch().cuda.synchronize()
        r.check(frames, bad, (image_offsets, offsets_name), images=images)
        r.run(images, frames, bad)                                     # the counts are ADDED
        torch().cuda.synchronize()
        r.check(frames, bad, "second call", times=2)
        if image_offsets == "packed":
            ref = reference()
            for i, case in enumerate(hc.CASES):
                if case[8] >= 0 and case[0] > CRYPT_MAX:
                    continue
                got, n = per_file_frames(r.infos[i], case, ref["stored"][i], ref["dec"])
                assert n == ref["bad"][i] and np.array_equal(got, ref["back"][i]), ("per-file", i, case)
    finally:
        r.close()


def test_read_without_counts():
    """d_bad_crc == NULL: the same frames; and without keys the stored bytes as they are, bad frames included"""
    for keyed in (True, False):
        r = ReadSet("odd", "packed", keyed=keyed)
        try:
            images, frames = r.images(), r.frames()
            r.run(images, frames, None)
            torch().cuda.synchronize()
            r.check(frames, None, ("no counts", keyed), images=images)
            if not keyed:
                bad = r.counts()
                r.run(images, frames, bad)
                torch().cuda.synchronize()
                r.check(frames, bad, "counts without keys")
        finally:
            r.close()


# ---------------------------------------------------------------- 3. round trip
def test_write_parse_read_returns_the_frames():
    t = torch()
    ref = reference()
    a = WriteSet("explicit")
    try:
        images = a.run(a.source(), a.images())
        files = a.s.images(images[EXTRA:])
        infos = []
        for image, f in zip(files, a.files):
            info = hca.parse(image)
            assert (info.frames_offset, info.hca.frame_count, info.hca.frame_size, info.encryption_type) == (
                f.hca.header_size, f.hca.frame_count, f.hca.frame_size, f.encryption_type)
            infos.append(info)
        r = HcaFileSet.from_infos(infos, None, [f.key for f in a.files], ref["dec"])
        try:
            assert list(r.image_offsets) == list(a.s.image_offsets)
            frames, bad = t.zeros(r.totals.frame_bytes, dtype=t.uint8, device="cuda"), t.zeros(r.files, dtype=t.int32, device="cuda")
            r.read_device(images[EXTRA:], frames, bad)
            got, counts = host(frames), host(bad)
            for i, (at, fr, f) in enumerate(zip(r.frame_offsets, a.frames, a.files)):
                fs = f.hca.frame_size
                mine, damaged = got[at:at + len(fr)], sorted(k for g, k in hc.BAD_FRAMES if g == i)
                if f.key < 0:                                          # copied as they were, bad CRCs included
                    assert np.array_equal(mine, fr) and counts[i] == len(damaged), i
                else:                                                  # the CRC was refreshed on the way in: valid now, and so it stays
                    assert counts[i] == 0, i
                    x, y = mine.reshape(-1, fs), np.asarray(fr).reshape(-1, fs)
                    assert np.array_equal(x[:, :-2], y[:, :-2])
                    assert [k for k in range(len(x)) if not np.array_equal(x[k, -2:], y[k, -2:])] == damaged, i
        finally:
            r.close()
    finally:
        a.close()


# ---------------------------------------------------------------- 4. forms
def test_forced_general_form_gives_the_same_bytes():
    a, r = WriteSet("explicit"), ReadSet("odd", "explicit")
    try:
        own_w, own_r = a.s.stats(), r.s.stats()
        moving = sum(1 for c in hc.CASES if c[1])
        assert own_w[0] > 0 and own_w[1] > 0 and own_w[0] + own_w[1] == moving and own_w == own_r
        old = L().vga_hca_files_force_general_this_thread(1)
        try:
            assert old == 0
            st = a.s.stats()
            assert st[0] == st[2] == 0 and st[1] == moving and st[3] == own_w[2] + own_w[3] and r.s.stats() == st
            source = a.source()
            images = a.run(source, a.images())
            d_images, frames, bad = r.images(), r.frames(), r.counts()
            r.run(d_images, frames, bad)
            torch().cuda.synchronize()
        finally:
            assert L().vga_hca_files_force_general_this_thread(old) == 1
        a.check(images, "general", source=source)
        r.check(frames, bad, "general", images=d_images)
        assert a.s.stats() == own_w
    finally:
        a.close()
        r.close()


def test_object_numbers_are_the_host_layouts():
    for name in ("packed", "explicit"):
        a = WriteSet(name)
        try:
            fo, io, tot = HcaFileSet.layout(a.files, a.offs)
            assert list(a.s.frame_offsets) == list(fo) and list(a.s.image_offsets) == list(io)
            assert all(getattr(a.s.totals, k) == getattr(tot, k) for k, _ in tot._fields_)
            items = [i for i in HcaFileSet.write_items(a.files, a.offs) if i.form]
            st = a.s.stats()
            assert (st[2], st[3]) == (sum(i.form == 1 for i in items), sum(i.form == 2 for i in items))
            assert st[0] == len({i.file for i in items if i.form == 1}) and st[1] == len({i.file for i in items if i.form == 2})
        finally:
            a.close()
    r = ReadSet("odd", "explicit")
    try:
        items = HcaFileSet.read_items(r.infos, r.image_offs, r.offs)
        st = r.s.stats()
        assert (st[2], st[3]) == (sum(i.form == 1 for i in items), sum(i.form == 2 for i in items))
        assert r.s.files == len(r.infos) and list(r.s.image_offsets) == r.image_offs and list(r.s.frame_offsets) == r.offs
        assert r.s.totals.total_frames == sum(c[1] for c in hc.CASES)
    finally:
        r.close()


# ---------------------------------------------------------------- 5. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    t = torch()
    old = L().vga_testing_poison_allocations(value)
    try:
        a = WriteSet("packed")                                         # (created under the mode: its tables are poisoned first)
        try:
            source = a.source(value ^ 0x3C)
            images = a.run(source, a.images(value ^ 0x3C))
            t.cuda.synchronize()
            a.check(images, ("poison", value), fill=value ^ 0x3C, source=source)
        finally:
            a.close()
        r = ReadSet("odd", "packed")
        try:
            images, frames, bad = r.images(value), r.frames(value ^ 0x3C), r.counts()
            r.run(images, frames, bad)
            t.cuda.synchronize()
            r.check(frames, bad, ("poison", value), fill=value ^ 0x3C)
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
    a, r = WriteSet("packed"), ReadSet("odd", "packed")
    try:
        (S,) = some_streams(1)
        source, packed = a.source(), r.images()
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                d_source, d_images = t.zeros_like(source), t.zeros_like(packed)
                images, frames, bad = a.images(), r.frames(), r.counts()
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                d_source.copy_(source, non_blocking=True)              # the inputs arrive behind the delay
                d_images.copy_(packed, non_blocking=True)
                a.run(d_source, images, stream=S)
                r.run(d_images, frames, bad, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, "busy stream", source=d_source)
        r.check(frames, bad, "busy stream", images=d_images)
    finally:
        r.close()
        a.close()


def test_two_streams_at_once():
    """one object for each direction, two streams each"""
    t = torch()
    a, r = WriteSet("explicit"), ReadSet("odd", "explicit")
    try:
        S1, S2 = some_streams(2)
        source, i1, i2 = a.source(), a.images(), a.images(0x11)
        d_images, f1, f2, b1, b2 = r.images(), r.frames(), r.frames(0x11), r.counts(), r.counts()
        t.cuda.synchronize()
        a.run(source, i1, stream=S1)
        a.run(source, i2, stream=S2)
        r.run(d_images, f1, b1, stream=S1)
        r.run(d_images, f2, b2, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(i1, "stream 1", source=source)
        a.check(i2, "stream 2", fill=0x11)
        r.check(f1, b1, "stream 1", images=d_images)
        r.check(f2, b2, "stream 2", fill=0x11)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 7. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    a, r = WriteSet("packed"), ReadSet("packed", "packed")
    try:
        source, images, frames, bad = a.source(), a.images(), r.frames(), r.counts()
        w, rd = L().vga_hca_write_device_v, L().vga_hca_read_device_v
        st, base, src, out = stream_ptr(), images.data_ptr() + EXTRA, source.data_ptr() + EXTRA, frames.data_ptr() + EXTRA
        assert rd(a.s._h, base, out, bad.data_ptr(), st) == -4                              # a set for writing refuses the read call
        assert w(r.s._h, src, base, st) == -4                                               # ... and the other way round
        assert w(a.s._h, None, base, st) == -1
        assert w(a.s._h, src, None, st) == -1
        assert w(a.s._h, src + 2, base, st) == -1                                           # alignment
        assert w(a.s._h, src, base + 8, st) == -1
        assert w(None, src, base, st) == -1
        assert rd(r.s._h, base + 1, out, bad.data_ptr(), st) == -1
        assert rd(r.s._h, base, out + 2, bad.data_ptr(), st) == -1
        assert rd(r.s._h, None, out, bad.data_ptr(), st) == -1
        assert rd(None, base, out, bad.data_ptr(), st) == -1
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(frames) == JUNK) and not host(bad).any()
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 8. the Python layer: files in, images out
def small_files():
    """seeded PCM: mono and stereo, two sample rates, one looping file; two files share a shape class"""
    rng = np.random.default_rng(0x5EED)
    out = []
    for nch, n, rate, loop in ((1, 3000, 48000, None), (2, 2500, 44100, None), (2, 5000, 48000, (1000, 4500)), (2, 1100, 44100, None),
                               (1, 700, 44100, None)):
        f = Pcm16Format([rng.integers(-20000, 20000, n).astype(np.int16) for _ in range(nch)], rate)
        if loop:
            f.Looping, f.LoopStart, f.LoopEnd = True, loop[0], loop[1]
        out.append(f)
    return out


def oracle_file(f, key):
    """the oracle's encoder, crypt and writer for one Pcm16Format: (image, info, plain frames)"""
    looping = bool(f.Looping)
    p = po.hca_params(f.ChannelCount, f.SampleCount, f.SampleRate, looping=looping, loop_start=f.LoopStart if looping else 0,
                      loop_end=f.LoopEnd if looping else 0)
    rc, info, frames = po.hca_encode(np.stack([np.asarray(ch, np.int16) for ch in f.Channels]), p)
    assert rc == 0
    body = po.hca_crypt(frames, info.frame_size, key.EncryptionTable) if key is not None else frames
    rc, image = po.hcafile_write(info, body, None, 1.0, key.KeyType if key is not None else 0, key is not None)
    assert rc == 0
    return image.tobytes(), info, frames


@pytest.mark.parametrize("code", [None, 0xCC55463930DBE1AB], ids=["plain", "keyed"])
def test_write_files_is_the_writers_get_file(code):
    files = small_files()
    key = crihca.CriHcaKey(code) if code is not None else None
    config = hca.HcaConfiguration(EncryptionKey=key)
    got = hca.write_files(files, config)
    assert len(got) == len(files)
    for k, f in enumerate(files):
        assert got[k] == oracle_file(f, key)[0], ("file", k)
    assert hca.write_files([], config) == []


@pytest.mark.parametrize("code", [None, 0xCC55463930DBE1AB], ids=["plain", "keyed"])
def test_read_files_is_the_readers_read_format(code):
    files = small_files()
    key = crihca.CriHcaKey(code) if code is not None else None
    made = [oracle_file(f, key) for f in files]
    images = [bytearray(m[0]) for m in made]
    images[1][made[1][1].header_size + 5] ^= 0x40                      # a damaged frame: counted, kept
    formats, bad = hca.read_files(images, EncryptionKey=key)
    assert bad == [0, 1, 0, 0, 0] and len(formats) == len(files)
    for k, (fmt, (_, info, frames)) in enumerate(zip(formats, made)):
        assert fmt.Hca.EncryptionType == 0 and fmt.Hca.FrameCount == info.frame_count and fmt.Hca.SampleCount == info.sample_count
        if k != 1:
            assert np.array_equal(fmt.AudioData, frames), k
    keep = [k for k in range(len(files)) if k != 1]
    pcm = crihca.decode_files([formats[k] for k in keep])
    for k, p in zip(keep, pcm):
        rc, want = po.hca_decode(made[k][1], made[k][2])
        assert rc == 0 and np.array_equal(np.stack([np.asarray(c) for c in p.Channels]), want), k
    if key is not None:
        left, _ = hca.read_files(images[:1], Decrypt=False)            # frames and type as they are
        assert left[0].Hca.EncryptionType == 56 and not np.array_equal(left[0].AudioData, made[0][2])
        with pytest.raises(_lib.InvalidDataError, match=r"file 0: Cannot find key"):
            hca.read_files(images[:1])
    assert hca.read_files([]) == ([], [])
