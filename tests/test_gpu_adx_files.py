"""include/vgaudio_hip/adx_files.h on the GPU: the images of a set of ADX files of different shapes against the oracle's AdxWriter
and against vga_adx_write_device file by file, the rows read back against the oracle's AdxReader and vga_adx_read_device, both
inside junk-filled buffers whose every byte outside the images / rows is checked; write -> vga_adx_parse -> read; the forced
general form against the mixed forms; poison mode; a busy caller stream; two streams at once; adx.write_files / adx.read_files
against the oracle's encoder, writer and reader.  The cases are tests/adx_files_cases.py's; tests/test_adx_files_host.py checks
that CASES names every function of the header."""
import ctypes as C

import numpy as np
import pytest

import adx_files_cases as ac
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd import adx
from vgaudio_amd.adx import AdxFileSet
from vgaudio_amd.gcadpcm import Pcm16Format

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_adx_files_layout_for": ["test_object_numbers_are_the_host_layouts", "test_write_files_is_the_writers_get_file"],
    "vga_adx_files_create": ["test_images_are_the_oracles_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_adx_files_create_from_infos": ["test_read_gives_the_oracles_and_the_per_file_rows", "test_write_parse_read_returns_the_rows"],
    "vga_adx_files_destroy": ["test_images_are_the_oracles_and_the_per_file_calls"],
    "vga_adx_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_adx_files_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_adx_write_device_v": [
        "test_images_are_the_oracles_and_the_per_file_calls", "test_write_parse_read_returns_the_rows",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_write_files_is_the_writers_get_file"],
    "vga_adx_read_device_v": [
        "test_read_gives_the_oracles_and_the_per_file_rows", "test_write_parse_read_returns_the_rows",
        "test_forced_general_form_gives_the_same_bytes", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_two_streams_at_once", "test_refused_calls_launch_nothing", "test_read_files_is_the_readers_read_format"],
    "vga_adx_files_write_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_adx_files_read_items_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_adx_files_stats": ["test_forced_general_form_gives_the_same_bytes", "test_object_numbers_are_the_host_layouts"],
    "vga_adx_files_force_general_this_thread": ["test_forced_general_form_gives_the_same_bytes"],
}

JUNK = 0xEE
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


def oracle_params(p):
    return po.adxfile_params(p.sample_rate, p.sample_count, p.looping, p.loop_start, p.loop_end, p.alignment_samples, p.frame_size, p.version,
                             p.type, p.highpass_frequency, p.encryption_type, p.trim_file)


_reference = {}


def reference(offsets_name):
    """files, row offsets, random rows and histories, and the oracle's image of every file: computed once, never changed"""
    if offsets_name not in _reference:
        files = ac.files_of(ac.CASES)
        offs = {"packed": None, "explicit16": ac.explicit_offsets(files, 0), "explicit4": ac.explicit_offsets(files, 4)}[offsets_name]
        rng = np.random.default_rng(0xAD0F11E5)
        rows, hist, want = [], [], []
        for f in files:
            n = ac.row_bytes(f)
            mine = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(f.channels)]
            h = rng.integers(-32768, 32768, f.channels).astype(np.int16)
            rc, image = po.adxfile_write(mine if n else [np.zeros(1, np.uint8)[:0]] * f.channels, h, oracle_params(f.params))
            assert rc == 0
            rows += mine
            hist += list(h)
            want.append(image)
        for a in rows + want:
            a.setflags(write=False)
        _reference[offsets_name] = (files, offs, rows, np.array(hist, np.int16), want)
    return _reference[offsets_name]


class WriteSet:
    def __init__(self, offsets_name="packed"):
        self.files, self.offs, self.rows, self.hist, self.want = reference(offsets_name)
        self.s = AdxFileSet(self.files, self.offs)

    def close(self):
        self.s.close()

    def audio(self, fill=JUNK):
        """the rows inside a junk-filled buffer: junk in the rounding gaps, between the rows and in the guard"""
        a = np.full(self.s.totals.audio_bytes, fill, np.uint8)
        for c, row in enumerate(self.rows):
            a[self.s.audio_offsets[c]:self.s.audio_offsets[c] + len(row)] = row
        return dev(a)

    def images(self, fill=JUNK):
        return torch().full((self.s.totals.image_bytes + 2 * EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def run(self, audio, images, stream=None, history=None):
        history = history if history is not None else dev(self.hist)
        self.keep = history
        _lib.check(L().vga_adx_write_device_v(self.s._h, audio.data_ptr(), history.data_ptr(), images.data_ptr() + EXTRA, stream_ptr(stream)))
        return images

    def check(self, images, what, fill=JUNK):
        """every image is the oracle's, every other byte of the buffer is what it was"""
        got = host(images).copy()
        assert np.all(got[:EXTRA] == fill) and np.all(got[-EXTRA:] == fill), (what, "outside the buffer")
        got = got[EXTRA:-EXTRA]
        for f, (at, want) in enumerate(zip(self.s.image_offsets, self.want)):
            mine = got[at:at + len(want)]
            if not np.array_equal(mine, want):
                bad = np.flatnonzero(mine != want)
                raise AssertionError((what, "file", f, ac.CASES[f], "first bad byte", int(bad[0]), "of", len(want), "bad bytes", len(bad)))
            got[at:at + len(want)] = fill
        assert np.all(got == fill), (what, "bytes outside the images were written", np.flatnonzero(got != fill)[:8])


# ---------------------------------------------------------------- 1. write
@pytest.mark.parametrize("offsets", ["packed", "explicit16", "explicit4"])
def test_images_are_the_oracles_and_the_per_file_calls(offsets):
    a = WriteSet(offsets)
    try:
        images = a.run(a.audio(), a.images())
        torch().cuda.synchronize()
        a.check(images, offsets)
        # vga_adx_write_device for every file alone, from rows staged at a pitch
        at = 0
        for f, file in enumerate(a.files):
            n, nch = ac.row_bytes(file), file.channels
            pitch = ac.up(max(n, 1), 16)
            staged = np.full((nch, pitch), JUNK, np.uint8)
            for c in range(nch):
                staged[c, :n] = a.rows[at + c]
            d_rows, d_hist = dev(staged), dev(a.hist[at:at + nch])
            d_file = torch().full((len(a.want[f]) + 32,), JUNK, dtype=torch().uint8, device="cuda")
            _lib.check(L().vga_adx_write_device(d_rows.data_ptr(), pitch, n, d_hist.data_ptr(), nch, C.byref(file.params), d_file.data_ptr(), stream_ptr()))
            assert np.array_equal(host(d_file)[:len(a.want[f])], a.want[f]), ("per-file call", f)
            at += nch
    finally:
        a.close()


# ---------------------------------------------------------------- 2. read
def read_reference():
    """the oracle's images of the packed cases, their parsed headers, and what the oracle's reader takes out of them"""
    files, _, rows, hist, want = reference("packed")
    infos, audio = [], []
    for image in want:
        infos.append(adx.parse(image.tobytes()))
        rc, h, hh, chans = po.adxfile_read(image.tobytes())
        assert rc == 0
        audio.append(chans)
    return files, want, infos, audio


def pack_images(want, offsets, total, fill=JUNK):
    packed = np.full(total + 2 * 16, fill, np.uint8)                     # (the set's own guard lies behind the last image)
    for image, at in zip(want, offsets):
        n = len(image)
        packed[at:at + n] = image
    return packed[:total]


def check_rows(s, infos, audio, got, what, fill=JUNK):
    got = got.copy()
    c = 0
    for f, info in enumerate(infos):
        for ch in range(info.channel_count):
            n, at = info.audio_bytes, int(s.audio_offsets[c])
            assert np.array_equal(got[at:at + n], audio[f][ch][:n]), (what, "file", f, "channel", ch)
            got[at:at + n] = fill
            c += 1
    assert np.all(got == fill), (what, "bytes outside the rows were written", np.flatnonzero(got != fill)[:8])


@pytest.mark.parametrize("offsets", ["packed", "odd"])
def test_read_gives_the_oracles_and_the_per_file_rows(offsets):
    t = torch()
    files, want, infos, audio = read_reference()
    # the reader sees the image up to the end of its audio
    sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
    offs = ac.odd_image_offsets(sizes) if offsets == "odd" else None
    s = AdxFileSet.from_infos(infos, offs)
    try:
        assert s.image_sizes == sizes and (offs is None or list(s.image_offsets) == offs)
        d_images = dev(pack_images([w[:n] for w, n in zip(want, sizes)], s.image_offsets, s.totals.image_bytes))
        rows = t.full((s.totals.audio_bytes,), JUNK, dtype=t.uint8, device="cuda")
        hist = t.full((s.channels + 8,), 0x7777, dtype=t.int16, device="cuda")
        s.read_device(d_images, rows, history=hist)
        t.cuda.synchronize()
        check_rows(s, infos, audio, host(rows), offsets)
        h = host(hist)
        assert list(h[:s.channels]) == [int(i.history[c][0]) for i in infos for c in range(i.channel_count)] and np.all(h[s.channels:] == 0x7777)
        # vga_adx_read_device for every file alone
        for f, info in enumerate(infos):
            if info.audio_bytes == 0:
                continue
            pitch = ac.up(info.audio_bytes, 16)
            d_file = dev(want[f][:sizes[f]])
            out = t.full((info.channel_count, pitch), JUNK, dtype=t.uint8, device="cuda")
            _lib.check(L().vga_adx_read_device(C.byref(info), d_file.data_ptr(), sizes[f], 1, out.data_ptr(), pitch, stream_ptr()))
            got = host(out)
            for ch in range(info.channel_count):
                assert np.array_equal(got[ch, :info.audio_bytes], audio[f][ch][:info.audio_bytes]), ("per-file call", f, ch)
    finally:
        s.close()


def test_write_parse_read_returns_the_rows():
    """write, vga_adx_parse of every image, a set from the infos over the SAME buffer, read: the rows, up to what the file kept"""
    t = torch()
    a = WriteSet("packed")
    try:
        images = a.run(a.audio(), a.images())
        t.cuda.synchronize()
        files_bytes = a.s.images(host(images)[EXTRA:-EXTRA])
        infos = [adx.parse(b) for b in files_bytes]
        r = AdxFileSet.from_infos(infos, [int(o) for o in a.s.image_offsets])
        try:
            rows = t.full((r.totals.audio_bytes,), JUNK, dtype=t.uint8, device="cuda")
            view = images[EXTRA:EXTRA + max(r.totals.image_bytes, 1)]
            assert r.totals.image_bytes <= a.s.totals.image_bytes
            _lib.check(L().vga_adx_read_device_v(r._h, view.data_ptr(), rows.data_ptr(), None, stream_ptr()))
            t.cuda.synchronize()
            got, c, longer = host(rows), 0, 0
            for f, (file, info) in enumerate(zip(a.files, infos)):
                held = ac.row_bytes(file)
                for ch in range(file.channels):
                    at, n = int(r.audio_offsets[c]), info.audio_bytes
                    keep = min(n, held)                                # a trimmed file keeps fewer frames, or asks for more than the rows held
                    assert np.array_equal(got[at:at + keep], a.rows[c][:keep]), (f, ch)
                    if n > held:                                       # ... then come the footer's bytes and its zeros, as the reference reads them
                        longer += 1
                    c += 1
            assert longer
        finally:
            r.close()
    finally:
        a.close()


# ---------------------------------------------------------------- 3. forms
def test_forced_general_form_gives_the_same_bytes():
    t = torch()
    a = WriteSet("packed")
    files, want, infos, audio = read_reference()
    r = AdxFileSet.from_infos(infos)
    try:
        mixed_w, mixed_r = a.s.stats(), r.stats()
        assert mixed_w[0] > 0 and mixed_w[1] > 0 and mixed_w[2] > 0 and mixed_w[3] > 0, mixed_w
        assert mixed_r[0] > 0 and mixed_r[1] > 0 and mixed_r[2] > 0 and mixed_r[3] > 0, mixed_r
        sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
        d_images = dev(pack_images([w[:n] for w, n in zip(want, sizes)], r.image_offsets, r.totals.image_bytes))
        assert L().vga_adx_files_force_general_this_thread(1) == 0
        try:
            forced_w, forced_r = a.s.stats(), r.stats()
            assert forced_w[0] == forced_w[2] == 0 and forced_w[1] == mixed_w[0] + mixed_w[1] and forced_w[3] > mixed_w[3]
            assert forced_r[0] == forced_r[2] == 0 and forced_r[1] == mixed_r[0] + mixed_r[1]
            images = a.run(a.audio(), a.images())
            rows = t.full((r.totals.audio_bytes,), JUNK, dtype=t.uint8, device="cuda")
            r.read_device(d_images, rows)
            t.cuda.synchronize()
        finally:
            assert L().vga_adx_files_force_general_this_thread(0) == 1
        a.check(images, "forced general")
        check_rows(r, infos, audio, host(rows), "forced general")
        assert a.s.stats() == mixed_w
        again = a.run(a.audio(), a.images())
        t.cuda.synchronize()
        assert t.equal(again, images)
    finally:
        r.close()
        a.close()


def test_object_numbers_are_the_host_layouts():
    for name in ("packed", "explicit4"):
        a = WriteSet(name)
        try:
            fc, ao, io, tot = AdxFileSet.layout(a.files, a.offs)
            assert list(a.s.first_channel) == list(fc) and list(a.s.audio_offsets) == list(ao) and list(a.s.image_offsets) == list(io)
            assert all(getattr(a.s.totals, k) == getattr(tot, k) for k, _ in tot._fields_)
            items = AdxFileSet.write_items(a.files, a.offs)
            audio_items = [i for i in items if i.form in (1, 2)]
            st = a.s.stats()
            assert (st[2], st[3]) == (sum(i.form == 1 for i in audio_items), sum(i.form == 2 for i in audio_items))
            assert st[0] == len({i.file for i in audio_items if i.form == 1}) and st[1] == len({i.file for i in audio_items if i.form == 2})
        finally:
            a.close()
    files, want, infos, audio = read_reference()
    r = AdxFileSet.from_infos(infos)
    try:
        items = AdxFileSet.read_items(infos)
        st = r.stats()
        assert (st[2], st[3]) == (sum(i.form == 1 for i in items), sum(i.form == 2 for i in items))
        assert r.channels == sum(i.channel_count for i in infos) and r.files == len(infos)
    finally:
        r.close()


# ---------------------------------------------------------------- 4. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    t = torch()
    old = L().vga_testing_poison_allocations(value)
    try:
        a = WriteSet("packed")                                         # (created under the mode: its tables are poisoned first)
        try:
            images = a.run(a.audio(value ^ 0x3C), a.images(value ^ 0x3C))
            t.cuda.synchronize()
            a.check(images, ("poison", value), fill=value ^ 0x3C)
        finally:
            a.close()
        files, want, infos, audio = read_reference()
        r = AdxFileSet.from_infos(infos)
        try:
            sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
            d_images = dev(pack_images([w[:n] for w, n in zip(want, sizes)], r.image_offsets, r.totals.image_bytes, value))
            rows = t.full((r.totals.audio_bytes,), value ^ 0x3C, dtype=t.uint8, device="cuda")
            r.read_device(d_images, rows)
            t.cuda.synchronize()
            check_rows(r, infos, audio, host(rows), ("poison", value), fill=value ^ 0x3C)
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
    a = WriteSet("packed")
    files, want, infos, audio = read_reference()
    r = AdxFileSet.from_infos(infos)
    try:
        (S,) = some_streams(1)
        sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
        source, d_packed = a.audio(), dev(pack_images([w[:n] for w, n in zip(want, sizes)], r.image_offsets, r.totals.image_bytes))
        d_hist = dev(a.hist)
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                d_audio, d_images = t.zeros_like(source), t.zeros_like(d_packed)
                images, rows = a.images(), t.full((r.totals.audio_bytes,), JUNK, dtype=t.uint8, device="cuda")
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                d_audio.copy_(source, non_blocking=True)               # the inputs arrive behind the delay
                d_images.copy_(d_packed, non_blocking=True)
                a.run(d_audio, images, stream=S, history=d_hist)
                r.read_device(d_images, rows, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, "busy stream")
        check_rows(r, infos, audio, host(rows), "busy stream")
    finally:
        r.close()
        a.close()


def test_two_streams_at_once():
    """one object for each direction, two streams each"""
    t = torch()
    a = WriteSet("explicit16")
    files, want, infos, audio = read_reference()
    r = AdxFileSet.from_infos(infos)
    try:
        S1, S2 = some_streams(2)
        sizes = [i.audio_offset + i.audio_bytes * i.channel_count for i in infos]
        d_audio, i1, i2, d_hist = a.audio(), a.images(), a.images(0x11), dev(a.hist)
        d_images = dev(pack_images([w[:n] for w, n in zip(want, sizes)], r.image_offsets, r.totals.image_bytes))
        r1, r2 = (t.full((r.totals.audio_bytes,), fill, dtype=t.uint8, device="cuda") for fill in (JUNK, 0x11))
        t.cuda.synchronize()
        a.run(d_audio, i1, stream=S1, history=d_hist)
        a.run(d_audio, i2, stream=S2, history=d_hist)
        r.read_device(d_images, r1, stream=S1)
        r.read_device(d_images, r2, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(i1, "stream 1")
        a.check(i2, "stream 2", fill=0x11)
        check_rows(r, infos, audio, host(r1), "stream 1")
        check_rows(r, infos, audio, host(r2), "stream 2", fill=0x11)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 6. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    a = WriteSet("packed")
    files, want, infos, audio = read_reference()
    r = AdxFileSet.from_infos(infos)
    try:
        d_audio, images, d_hist = a.audio(), a.images(), dev(a.hist)
        rows = t.full((r.totals.audio_bytes,), JUNK, dtype=t.uint8, device="cuda")
        w, rd = L().vga_adx_write_device_v, L().vga_adx_read_device_v
        st, base = stream_ptr(), images.data_ptr() + EXTRA
        assert rd(a.s._h, base, d_audio.data_ptr(), None, st) == -4                         # a set for writing refuses the read call
        assert w(r._h, rows.data_ptr(), d_hist.data_ptr(), base, st) == -4                  # ... and the other way round
        assert w(a.s._h, d_audio.data_ptr(), None, base, st) == -1                          # version 4 files need the histories
        assert w(a.s._h, None, d_hist.data_ptr(), base, st) == -1
        assert w(a.s._h, d_audio.data_ptr(), d_hist.data_ptr(), None, st) == -1
        assert w(a.s._h, d_audio.data_ptr() + 4, d_hist.data_ptr(), base, st) == -1          # alignment
        assert w(a.s._h, d_audio.data_ptr(), d_hist.data_ptr(), base + 8, st) == -1
        assert rd(r._h, base + 1, rows.data_ptr(), None, st) == -1
        assert rd(r._h, base, rows.data_ptr() + 2, None, st) == -1
        assert rd(r._h, None, rows.data_ptr(), None, st) == -1
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(rows) == JUNK)
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 7. the Python layer: files in, images out
def small_files():
    """seeded PCM: mixed rates, looping and not, mono and stereo; two files share a codec parameter set"""
    rng = np.random.default_rng(0x5EED)
    out = []
    for nch, n, rate, loop in ((1, 1000, 48000, None), (2, 777, 44100, (5, 700)), (2, 64, 48000, None), (1, 500, 32000, (33, 480)),
                               (2, 1200, 44100, (32, 1100)), (2, 900, 48000, (5, 600)), (1, 31, 22050, None)):
        f = Pcm16Format([rng.integers(-20000, 20000, n).astype(np.int16) for _ in range(nch)], rate)
        if loop:
            f.Looping, f.LoopStart, f.LoopEnd = True, loop[0], loop[1]
        out.append(f)
    return out


def oracle_file(f, cfg):
    """the oracle's encoder and writer for one Pcm16Format"""
    spf = (cfg.FrameSize - 2) * 2
    start = f.LoopStart if f.Looping else 0
    a = ac.up(start, spf * 2 if f.ChannelCount == 1 else spf) - start
    p = po.adx_params(sample_rate=f.SampleRate, frame_size=cfg.FrameSize, version=cfg.Version, type=cfg.Type, filter=cfg.Filter, padding=a)
    chans, hist = po.adx_encode_batch(np.stack([np.asarray(ch, np.int16) for ch in f.Channels]), p)
    chans = list(chans)
    looping = bool(f.Looping)
    fp = po.adxfile_params(f.SampleRate, f.SampleCount + a, looping, (f.LoopStart if looping else 0) + a, (f.LoopEnd if looping else 0) + a, a,
                           cfg.FrameSize, cfg.Version, cfg.Type, 500, cfg.EncryptionType, cfg.TrimFile)
    rc, image = po.adxfile_write(chans, hist, fp)
    assert rc == 0
    return image.tobytes(), chans


@pytest.mark.parametrize("cfg", [dict(), dict(Version=3, TrimFile=False)], ids=["default", "v3-untrimmed"])
def test_write_files_is_the_writers_get_file(cfg):
    files = small_files()
    config = adx.AdxConfiguration(**cfg)
    got = adx.write_files(files, config)
    assert len(got) == len(files)
    for k, f in enumerate(files):
        want, _ = oracle_file(f, config)
        assert got[k] == want, ("file", k)
    if not cfg:
        assert got[1] == adx.AdxWriter(config).GetFile(files[1])
        empty = Pcm16Format([np.zeros(0, np.int16)], 48000)
        with pytest.raises(_lib.ArgumentError, match=r"file 2\b"):
            adx.write_files(files[:2] + [empty], config)
    assert adx.write_files([], config) == []


def test_read_files_is_the_readers_read_format():
    files = small_files()
    config = adx.AdxConfiguration()
    images = [oracle_file(f, config)[0] for f in files]
    got = adx.read_files(images)
    assert len(got) == len(files)
    for k, (image, fmt) in enumerate(zip(images, got)):
        rc, h, hist, chans = po.adxfile_read(image)
        assert rc == 0
        assert fmt.ChannelCount == h.channel_count and fmt.SampleRate == h.sample_rate and fmt.Looping == bool(h.looping)
        assert fmt.SampleCount == h.sample_count and fmt.AlignmentSamples == h.inserted_samples
        for c in range(h.channel_count):
            assert np.array_equal(np.asarray(fmt.Channels[c].Audio), chans[c]) and fmt.Channels[c].History == int(hist[c]), (k, c)
        one = adx.AdxReader().ReadFormat(image)
        assert all(np.array_equal(x.Audio, y.Audio) for x, y in zip(fmt.Channels, one.Channels))
        assert (fmt.LoopStart, fmt.LoopEnd, fmt.UnalignedSampleCount) == (one.LoopStart, one.LoopEnd, one.UnalignedSampleCount)
    assert adx.read_files([]) == []
