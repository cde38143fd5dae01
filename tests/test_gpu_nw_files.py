"""Sets of BRSTM / BCSTM / BFSTM files on the device (include/vgaudio_hip/nw_files.h): vga_nwstm_write_device_v and
vga_nwstm_read_device_v on the packed rows of one set of files (tests/nw_files_cases.py: the smallest shapes at which each
branch can go wrong, every version of the writers, interleaves of 8, 16 and 0x2000 bytes).  Every image must be
tests/nwstm_ref.build_image's (the restatement of the reference's writers) fed with the oracle's channels, and what
vga_nwstm_write_device writes for that file alone; every row read back must be vga_nwstm_read_device's.  All buffers are larger
than needed and full of junk, and every byte outside the images, rows and per-channel arrays is compared afterwards.  The header
is outside the lists the older test files enumerate, so this file carries its own table (CASES); tests/test_nw_files_host.py
holds that table to the header."""
import ctypes as C

import numpy as np
import pytest

import gc_aligned_cases as ga
import nw_files_cases as nf
from oracle import pyoracle as po
from test_gpu_device_streams import delay  # noqa: F401  (the calibrated GPU delay that makes a caller's stream busy)
from vgaudio_amd import _lib
from vgaudio_amd.gcadpcm import AlignedFileSet
from vgaudio_amd.nwstm import NwFileSet

pytestmark = pytest.mark.gpu

# function of the header -> the tests below that call it
CASES = {
    "vga_nw_files_layout_for": ["test_object_numbers_are_the_host_layouts"],
    "vga_nw_files_create": ["test_images_are_the_reference_writers_and_the_per_file_calls", "test_object_numbers_are_the_host_layouts"],
    "vga_nw_files_create_from_infos": ["test_read_gives_the_per_file_rows_and_the_decode_follows", "test_refused_calls_launch_nothing"],
    "vga_nw_files_destroy": ["test_images_are_the_reference_writers_and_the_per_file_calls"],
    "vga_nw_files_totals_of": ["test_object_numbers_are_the_host_layouts"],
    "vga_nw_files_offsets": ["test_object_numbers_are_the_host_layouts"],
    "vga_nw_files_gc_files": ["test_object_numbers_are_the_host_layouts", "test_chain_from_pcm_stays_on_the_device"],
    "vga_nw_files_ragged": ["test_object_numbers_are_the_host_layouts", "test_read_gives_the_per_file_rows_and_the_decode_follows"],
    "vga_nwstm_write_device_v": [
        "test_images_are_the_reference_writers_and_the_per_file_calls", "test_chain_from_pcm_stays_on_the_device",
        "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream", "test_two_calls_on_two_streams",
        "test_refused_calls_launch_nothing", "test_an_empty_set_launches_nothing", "test_write_files_is_the_writers_get_file"],
    "vga_nwstm_read_device_v": [
        "test_read_gives_the_per_file_rows_and_the_decode_follows", "test_bytes_do_not_depend_on_poison", "test_calls_on_a_busy_stream",
        "test_refused_calls_launch_nothing", "test_an_empty_set_launches_nothing"],
}

SENTINEL = 0x7777
JUNK = 0xEE
EXTRA = 64
POOL_STREAMS = 32                                                      # torch hands out this many streams, round robin


def torch():
    import torch as t
    return t


def L():
    return _lib.lib()


def dev(a):
    return torch().from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def stream_ptr(stream=None):
    return C.c_void_p((stream if stream is not None else torch().cuda.current_stream()).cuda_stream)


def ptr(t):
    return t.data_ptr() if t is not None else None


def row_offsets(ragged, nch):
    """(pcm offsets, adpcm offsets) of a ragged batch's rows"""
    po_, ao = np.zeros(max(nch, 1), np.int64), np.zeros(max(nch, 1), np.int64)
    i64p = C.POINTER(C.c_int64)
    _lib.check(L().vga_gcadpcm_ragged_offsets(ragged, po_.ctypes.data_as(i64p), ao.ctypes.data_as(i64p)))
    return po_[:nch], ao[:nch]


# ---------------------------------------------------------------- one set for writing, its inputs from the oracle
_per_file = {}


class WriteSet:
    def __init__(self, name):
        self.name = name
        self.cfg, self.tuples = nf.CONFIGS[name]
        self.files = nf.files_of(self.tuples)
        self.s = NwFileSet(self.files, configuration=self.cfg)
        self.m = nf.model(self.files, self.cfg)
        self.t = self.s.totals
        self.gc = nf.gc_tuples(self.files, self.cfg)
        self.ref = ga.reference(self.gc)                               # per file, per channel: the oracle's encode and build
        self.chans = [ch for f in self.ref for ch in f]
        assert all(ch["rc"] == 0 for ch in self.chans)
        self.nch = len(self.chans)
        rng = np.random.default_rng(5)
        self.gain = rng.integers(-3000, 3000, self.nch).astype(np.int16)
        self.start = rng.integers(-30000, 30000, (self.nch, 3)).astype(np.int16)
        self.loop = np.stack([ch["ctx"] for ch in self.chans]).astype(np.int16)

    def close(self):
        self.s.close()

    def inputs(self):
        """the packed rows and tables (junk in every gap and guard) and the per-channel arrays, on the device"""
        adpcm = np.full(self.t.adpcm_bytes + EXTRA, JUNK, np.uint8)
        seek = np.full(self.t.seek_shorts + EXTRA, SENTINEL, np.int16)
        for c, ch in enumerate(self.chans):
            a, so = self.m["adpcm_off"][c], self.m["seek_off"][c]
            adpcm[a:a + len(ch["out"])] = ch["out"]
            seek[so:so + len(ch["seek"])] = ch["seek"]
            assert len(ch["seek"]) == 2 * self.m["entries"][c]
        coefs = np.stack([ch["coefs"] for ch in self.chans]).astype(np.int16)
        return {"adpcm": dev(adpcm), "seek": dev(seek), "coefs": dev(coefs), "gain": dev(self.gain), "start": dev(self.start), "loop": dev(self.loop)}

    def images(self, fill=JUNK):
        return torch().full((self.t.image_bytes + EXTRA,), fill, dtype=torch().uint8, device="cuda")

    def run(self, b, images, nulls=False, stream=None):
        _lib.check(L().vga_nwstm_write_device_v(self.s._h, ptr(b["adpcm"]), ptr(b["coefs"]), None if nulls else ptr(b["gain"]),
                                                None if nulls else ptr(b["start"]), None if nulls else ptr(b["loop"]), ptr(b["seek"]),
                                                ptr(images), stream_ptr(stream)))
        return images

    def per_file(self, nulls):
        """vga_nwstm_write_device on every file alone (tracks NULL), from the same channels: one `bytes` per file"""
        key = (self.name, nulls)
        if key in _per_file:
            return _per_file[key]
        t, out, c = torch(), [], 0
        for f, lay, chans in zip(self.files, self.m["layouts"], self.ref):
            nch, p = f.channels, nf.params_of(f, self.cfg)
            n, e = lay.channel_adpcm_bytes, lay.channel_seek_entries
            pitch, seek_pitch = max(nf.up(n, 16), 16), max(nf.up(2 * e, 8), 8)
            rows, seek = np.full((nch, pitch), 0x5A, np.uint8), np.full((nch, seek_pitch), SENTINEL, np.int16)
            for i, ch in enumerate(chans):
                rows[i, :n] = ch["out"]
                seek[i, :2 * e] = ch["seek"]
            d_rows, d_seek, d_coefs = dev(rows), dev(seek), dev(np.stack([ch["coefs"] for ch in chans]).astype(np.int16))
            d_gain, d_start, d_loop = dev(self.gain[c:c + nch]), dev(self.start[c:c + nch]), dev(self.loop[c:c + nch])
            image = t.full((lay.file_size + 16,), JUNK, dtype=t.uint8, device="cuda")
            _lib.check(L().vga_nwstm_write_device(C.byref(p), nch, 1, None, ptr(d_rows) if n else None, pitch, n, ptr(d_coefs),
                                                  None if nulls else ptr(d_gain), None if nulls else ptr(d_start), None if nulls else ptr(d_loop),
                                                  ptr(d_seek) if e else None, seek_pitch, e, ptr(image), lay.file_size, stream_ptr()))
            t.cuda.synchronize()
            got = host(image)
            assert np.all(got[lay.file_size:] == JUNK)
            out.append(got[:lay.file_size].tobytes())
            c += nch
        _per_file[key] = out
        return out

    def reference_images(self, nulls):
        out, c = [], 0
        for f, lay, chans in zip(self.files, self.m["layouts"], self.ref):
            k = f.channels
            out.append(nf.reference_image(f, self.cfg, lay, chans) if nulls else
                       nf.reference_image(f, self.cfg, lay, chans, [int(v) for v in self.gain[c:c + k]], self.start[c:c + k].tolist(),
                                          self.loop[c:c + k].tolist()))
            c += k
        return out

    def check(self, images, nulls, what, fill=JUNK, reference=True):
        """every image is the per-file call's (and the reference writers'); every byte outside the images is untouched"""
        got = host(images)
        mask = np.ones(got.size, bool)
        want_own = self.per_file(nulls)
        want_ref = self.reference_images(nulls) if reference else want_own
        for f, (at, size) in enumerate(zip(self.m["image_off"], self.m["image_size"])):
            image = got[at:at + size].tobytes()
            assert image == want_own[f], (what, "file", f, "differs from vga_nwstm_write_device")
            assert image == want_ref[f], (what, "file", f, "differs from the reference writers")
            mask[at:at + size] = False
        assert np.all(got[mask] == fill), (what, "bytes outside the images were written")


# ---------------------------------------------------------------- 1. write, per configuration
@pytest.mark.parametrize("name", sorted(nf.CONFIGS))
def test_images_are_the_reference_writers_and_the_per_file_calls(name):
    a = WriteSet(name)
    try:
        b = a.inputs()
        given, nulls = a.run(b, a.images()), a.run(b, a.images(), nulls=True)
        torch().cuda.synchronize()
        a.check(given, False, (name, "arrays given"))
        a.check(nulls, True, (name, "NULL arrays"))
        assert host(given)[:4].tobytes() == {0: b"RSTM", 1: b"CSTM", 2: b"FSTM"}[a.cfg.target]
        for k in ("adpcm", "seek"):                                    # the inputs are read only
            fresh = a.inputs()
            assert np.array_equal(host(b[k]), host(fresh[k]))
    finally:
        a.close()


# ---------------------------------------------------------------- 2. the chain
@pytest.mark.parametrize("name", ["rstm", "rstm-default", "cstm-2.1"])
def test_chain_from_pcm_stays_on_the_device(name):
    """vga_gcadpcm_coefs_device_v -> vga_gcadpcm_encode_device_v -> vga_gcadpcm_align_channels_device_v -> vga_nwstm_write_device_v on
    one set, no host step between them: the images are the per-file route's"""
    t = torch()
    a = WriteSet(name)
    al = AlignedFileSet(a.s.gc_files())
    try:
        tot, nch = al.totals, al.channels
        assert (tot.out_adpcm_bytes, tot.seek_shorts, nch) == (a.t.adpcm_bytes, a.t.seek_shorts, a.nch)
        assert list(al.seek_offsets) == list(a.s.seek_offsets) and list(al.offsets("out")[1]) == a.m["adpcm_off"]
        pin, _ = al.offsets("in")
        pcm = np.zeros(tot.pcm_samples, np.int16)
        for c, ch in enumerate(a.chans):
            pcm[pin[c]:pin[c] + len(ch["x"])] = ch["x"]
        new = lambda n, dtype, fill: t.full((max(int(n), 16) + EXTRA,), fill, dtype=dtype, device="cuda")
        d_pcm, coefs, adpcm = dev(pcm), new(nch * 16, t.int16, SENTINEL), new(tot.adpcm_bytes, t.uint8, JUNK)
        out, seek, ctx = new(tot.out_adpcm_bytes, t.uint8, JUNK), new(tot.seek_shorts, t.int16, SENTINEL), new(nch * 3, t.int16, SENTINEL)
        ws = t.empty(max(L().vga_gcadpcm_ragged_coefs_workspace_bytes(al.ragged_in), tot.workspace_bytes, 16), dtype=t.uint8, device="cuda")
        images, st = a.images(), stream_ptr()
        _lib.check(L().vga_gcadpcm_coefs_device_v(al.ragged_in, ptr(d_pcm), ptr(coefs), ptr(ws), ws.numel(), st))
        _lib.check(L().vga_gcadpcm_encode_device_v(al.ragged_in, ptr(d_pcm), ptr(coefs), None, None, ptr(adpcm), st))
        al.align_channels(adpcm, coefs, out, seek=seek, loop_context=ctx, workspace=ws)
        _lib.check(L().vga_nwstm_write_device_v(a.s._h, ptr(out), ptr(coefs), None, None, ptr(ctx), ptr(seek), ptr(images), st))
        t.cuda.synchronize()
        # the per-file route with the same arrays: gain 0, the start context of a fresh channel, the builder's loop context
        got, c = host(images), 0
        for f, (fl, lay, chans) in enumerate(zip(a.files, a.m["layouts"], a.ref)):
            k = fl.channels
            want = nf.reference_image(fl, a.cfg, lay, chans, None, None, a.loop[c:c + k].tolist())
            at = a.m["image_off"][f]
            assert got[at:at + lay.file_size].tobytes() == want, (name, "file", f)
            c += k
        a.gain[:] = 0                                                  # ... and byte for byte vga_nwstm_write_device's
        a.start[:] = [[ch["out"][0] if len(ch["out"]) else 0, 0, 0] for ch in a.chans]
        _per_file.pop((name, False), None)
        a.check(images, False, (name, "chain"))
        _per_file.pop((name, False), None)
    finally:
        al.close()
        a.close()


# ---------------------------------------------------------------- 3. read
def written_images(name):
    """the images of a set, its NwFileSet layout and the parsed info of every file"""
    a = WriteSet(name)
    try:
        got = host(a.run(a.inputs(), a.images()))
        files = [got[at:at + size].copy() for at, size in zip(a.m["image_off"], a.m["image_size"])]
        return a.chans, a.m, files
    finally:
        a.close()


def parse(image):
    info = _lib.NwInfoC()
    _lib.check(L().vga_nwstm_parse(image.ctypes.data_as(_lib.u8p), len(image), C.byref(info)))
    return info


@pytest.mark.parametrize("offsets", ["packed", "caller"])
@pytest.mark.parametrize("name", ["rstm", "cstm-2.1", "fstm-default"])
def test_read_gives_the_per_file_rows_and_the_decode_follows(name, offsets):
    t = torch()
    chans, m, files = written_images(name)
    infos = [parse(f) for f in files]
    offs, at = None, 8
    if offsets == "caller":                                            # multiples of 8 that are not multiples of 16
        offs = []
        for f in files:
            offs.append(at)
            at = nf.up(at + len(f), 16) + 8
    r = NwFileSet.from_infos(infos, offs)
    try:
        assert offs is None or list(r.image_offsets) == offs
        assert offs is not None or list(r.image_offsets) == m["image_off"]
        nch, tot = r.channels, r.totals
        packed = np.full(tot.image_bytes + EXTRA, 0x3C, np.uint8)
        for f, o in zip(files, r.image_offsets):
            packed[o:o + len(f)] = f
        d_images = dev(packed)
        rows = t.full((tot.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
        coefs, gain = t.full((nch * 16 + EXTRA,), SENTINEL, dtype=t.int16, device="cuda"), t.full((nch + EXTRA,), SENTINEL, dtype=t.int16, device="cuda")
        start, loop = (t.full((nch * 3 + EXTRA,), SENTINEL, dtype=t.int16, device="cuda") for _ in range(2))
        r.read(d_images, rows, coefs, gain, start, loop)
        rows2 = t.full((tot.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
        r.read(d_images, rows2)                                        # the per-channel arrays are optional
        t.cuda.synchronize()
        got, mask, c = host(rows), np.ones(tot.adpcm_bytes + EXTRA, bool), 0
        po_, ao = row_offsets(r.ragged, nch)
        want_coefs, want_gain, want_start, want_loop = [], [], [], []
        for f, info in zip(files, infos):
            k, n = info.channel_count, info.adpcm_bytes
            pitch = max(nf.up(n, 16), 16)
            own = t.full((k, pitch), JUNK, dtype=t.uint8, device="cuda")
            d_file = dev(f)
            _lib.check(L().vga_nwstm_read_device(C.byref(info), ptr(d_file), len(f), 1, ptr(own), pitch, stream_ptr()))
            t.cuda.synchronize()
            own = host(own)
            for i in range(k):
                assert np.array_equal(got[ao[c + i]:ao[c + i] + n], own[i, :n]), (name, offsets, "channel", c + i)
                mask[ao[c + i]:ao[c + i] + n] = False
                want_coefs.append(list(info.coefs[i])), want_gain.append(info.gain[i])
                want_start.append(list(info.start_context[i])), want_loop.append(list(info.loop_context[i]))
            c += k
        assert np.all(got[mask] == JUNK), "bytes outside the rows were written"
        assert np.array_equal(got, host(rows2))
        assert np.array_equal(host(coefs)[:nch * 16].reshape(nch, 16), np.array(want_coefs, np.int16)) and np.all(host(coefs)[nch * 16:] == SENTINEL)
        assert np.array_equal(host(gain)[:nch], np.array(want_gain, np.int16)) and np.all(host(gain)[nch:] == SENTINEL)
        assert np.array_equal(host(start)[:nch * 3].reshape(nch, 3), np.array(want_start, np.int16)) and np.all(host(start)[nch * 3:] == SENTINEL)
        assert np.array_equal(host(loop)[:nch * 3].reshape(nch, 3), np.array(want_loop, np.int16)) and np.all(host(loop)[nch * 3:] == SENTINEL)
        assert np.array_equal(host(coefs)[:nch * 16].reshape(nch, 16), np.stack([ch["coefs"] for ch in chans]))
        assert np.all(host(d_images) == packed)                        # the images are read only
        # the decode follows without a host round trip
        pcm = t.full((tot.pcm_samples + EXTRA,), SENTINEL, dtype=t.int16, device="cuda")
        status = t.zeros(1, dtype=t.int32, device="cuda")
        _lib.check(L().vga_gcadpcm_decode_device_v(r.ragged, ptr(rows), ptr(coefs), None, None, ptr(pcm), ptr(status), stream_ptr()))
        t.cuda.synchronize()
        dec, c = host(pcm), 0
        for info in infos:
            for i in range(info.channel_count):
                n = info.sample_count
                assert np.array_equal(dec[po_[c]:po_[c] + n], chans[c]["pcm"][:n]), (name, "decode of channel", c)
                if n:
                    assert np.array_equal(dec[po_[c]:po_[c] + n], po.gc_decode(chans[c]["out"][:nf.byte_count(n)], chans[c]["coefs"], n))
                c += 1
    finally:
        r.close()


# ---------------------------------------------------------------- 4. the object's numbers, the empty set
def test_object_numbers_are_the_host_layouts():
    for name in ("rstm-short", "fstm-default"):
        a = WriteSet(name)
        try:
            fc, so, io, tot = NwFileSet.layout(a.files, configuration=a.cfg)
            assert list(a.s.first_channel) == list(fc) and list(a.s.seek_offsets) == list(so) and list(a.s.image_offsets) == list(io)
            assert all(getattr(a.t, k) == getattr(tot, k) for k, _ in tot._fields_)
            assert a.s.image_sizes == a.m["image_size"]
            rg = a.s.ragged
            assert rg and L().vga_gcadpcm_ragged_channels(rg) == a.nch and L().vga_gcadpcm_ragged_adpcm_bytes(rg) == tot.adpcm_bytes
            ao = np.zeros(a.nch, np.int64)
            _lib.check(L().vga_gcadpcm_ragged_offsets(rg, None, ao.ctypes.data_as(C.POINTER(C.c_int64))))
            assert list(ao) == a.m["adpcm_off"]
            for g, f, lay in zip(a.s.gc_files(), a.files, a.m["layouts"]):
                assert (g.channels, g.sample_rate) == (f.channels, f.sample_rate) and bytes(g.channel) == bytes(lay.channel)
        finally:
            a.close()


def test_an_empty_set_launches_nothing():
    t = torch()
    s, r = NwFileSet([], configuration=nf.config(nf.CSTM)), NwFileSet.from_infos([])
    try:
        images = t.full((512,), JUNK, dtype=t.uint8, device="cuda")
        assert L().vga_nwstm_write_device_v(s._h, ptr(images), ptr(images), None, None, None, None, ptr(images), stream_ptr()) == 0
        assert L().vga_nwstm_read_device_v(r._h, ptr(images), ptr(images), None, None, None, None, stream_ptr()) == 0
        assert L().vga_nwstm_write_device_v(s._h, None, None, None, None, None, None, None, None) == 0
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK)
        assert s.totals.image_bytes == 256 and s.gc_files() == []
    finally:
        s.close()
        r.close()


# ---------------------------------------------------------------- 5. poison mode
@pytest.mark.parametrize("value", [0xA5, 0xFF])
def test_bytes_do_not_depend_on_poison(value):
    old = L().vga_testing_poison_allocations(value)
    try:
        a = WriteSet("rstm-short")                                     # (created under the mode: its tables are poisoned first)
        try:
            images = a.run(a.inputs(), a.images(value ^ 0x3C))
            torch().cuda.synchronize()
            a.check(images, False, ("poison", value), fill=value ^ 0x3C)
        finally:
            a.close()
        chans, m, files = written_images("cstm-2.1")
        infos = [parse(f) for f in files]
        r = NwFileSet.from_infos(infos)
        try:
            packed = np.full(r.totals.image_bytes, value, np.uint8)
            for f, o in zip(files, r.image_offsets):
                packed[o:o + len(f)] = f
            rows = torch().full((r.totals.adpcm_bytes,), value ^ 0x3C, dtype=torch().uint8, device="cuda")
            r.read(dev(packed), rows)
            torch().cuda.synchronize()
            got, c = host(rows), 0
            ao = row_offsets(r.ragged, r.channels)[1]
            for info in infos:
                for i in range(info.channel_count):
                    n = info.adpcm_bytes
                    assert np.array_equal(got[ao[c]:ao[c] + n], chans[c]["out"][:n])
                    got[ao[c]:ao[c] + n] = value ^ 0x3C
                    c += 1
            assert np.all(got == value ^ 0x3C)
        finally:
            r.close()
    finally:
        torch().cuda.synchronize()
        L().vga_testing_poison_allocations(old if old >= 0 else -1)


# ---------------------------------------------------------------- 6. streams
_streams = []


def some_streams(n):
    """Streams for this file, taken once and so that the files that run after it find torch's stream pool as they would without
    it (tests/test_gpu_gc_files.py: one_stream): one whole turn of the pool with the imported `delay` fixture's, every stream
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
    a = WriteSet("rstm")
    chans, m, files = written_images("rstm")
    infos = [parse(f) for f in files]
    r = NwFileSet.from_infos(infos)
    try:
        (S,) = some_streams(1)
        b = a.inputs()
        packed = np.full(r.totals.image_bytes, 0x3C, np.uint8)
        for f, o in zip(files, r.image_offsets):
            packed[o:o + len(f)] = f
        source, d_packed = b["adpcm"], dev(packed)
        with t.cuda.stream(S):
            for busy in (False, True):                                 # (warm first: every kernel has run once)
                b["adpcm"] = t.zeros_like(source)
                d_images = t.zeros_like(d_packed)
                images, rows = a.images(), t.full((r.totals.adpcm_bytes,), JUNK, dtype=t.uint8, device="cuda")
                S.synchronize()
                if busy:
                    t.cuda._sleep(cycles)
                b["adpcm"].copy_(source, non_blocking=True)            # the inputs arrive behind the delay
                d_images.copy_(d_packed, non_blocking=True)
                a.run(b, images, stream=S)
                r.read(d_images, rows, stream=S)
                if busy:
                    assert not S.query(), "the caller's stream was idle when the calls returned (they waited for it)"
        S.synchronize()
        a.check(images, False, "busy stream")
        got, ao = host(rows), row_offsets(r.ragged, r.channels)[1]
        for c, ch in enumerate(chans):
            n = infos[ch_file(m, c)].adpcm_bytes
            assert np.array_equal(got[ao[c]:ao[c] + n], ch["out"][:n]), ("busy stream: row", c)
    finally:
        r.close()
        a.close()


def ch_file(m, c):
    """the file of channel c"""
    return max(f for f, first in enumerate(m["first_channel"]) if first <= c)


def test_two_calls_on_two_streams():
    """one object, two streams"""
    t = torch()
    a = WriteSet("cstm-2.2-big")
    try:
        S1, S2 = some_streams(2)
        b, i1, i2 = a.inputs(), a.images(), a.images(0x11)
        t.cuda.synchronize()
        a.run(b, i1, stream=S1)
        a.run(b, i2, nulls=True, stream=S2)
        S1.synchronize()
        S2.synchronize()
        a.check(i1, False, "stream 1")
        a.check(i2, True, "stream 2", fill=0x11)
    finally:
        a.close()


# ---------------------------------------------------------------- 7. refused calls
def test_refused_calls_launch_nothing():
    t = torch()
    ARG, OP = _lib.VGA_ERR_ARGUMENT, -4
    a = WriteSet("rstm")
    chans, m, files = written_images("rstm")
    r = NwFileSet.from_infos([parse(f) for f in files])
    try:
        b, images = a.inputs(), a.images()
        rows = t.full((a.t.adpcm_bytes + EXTRA,), JUNK, dtype=t.uint8, device="cuda")
        A, K, S, I, R = ptr(b["adpcm"]), ptr(b["coefs"]), ptr(b["seek"]), ptr(images), ptr(rows)
        write, read = L().vga_nwstm_write_device_v, L().vga_nwstm_read_device_v
        assert write(a.s._h, A + 8, K, None, None, None, S, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, S + 8, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, S, I + 8, None) == ARG
        assert write(a.s._h, None, K, None, None, None, S, I, None) == ARG and write(a.s._h, A, None, None, None, None, S, I, None) == ARG
        assert write(a.s._h, A, K, None, None, None, None, I, None) == ARG and write(a.s._h, A, K, None, None, None, S, None, None) == ARG
        assert write(r._h, A, K, None, None, None, S, I, None) == OP        # a set for reading
        assert read(a.s._h, I, R, None, None, None, None, None) == OP       # a set for writing
        assert read(r._h, I + 8, R, None, None, None, None, None) == ARG and read(r._h, I, R + 8, None, None, None, None, None) == ARG
        assert read(r._h, None, R, None, None, None, None, None) == ARG and read(r._h, I, None, None, None, None, None, None) == ARG
        assert L().vga_nw_files_gc_files(r._h, (_lib.GcFileC * r.files)()) == OP
        t.cuda.synchronize()
        assert np.all(host(images) == JUNK) and np.all(host(rows) == JUNK)
        # exactly at the minimum: buffers of the totals' sizes
        exact = {k: b[k][:n].clone() for k, n in (("adpcm", a.t.adpcm_bytes), ("seek", a.t.seek_shorts))}
        out = t.full((a.t.image_bytes,), JUNK, dtype=t.uint8, device="cuda")
        assert write(a.s._h, ptr(exact["adpcm"]), K, ptr(b["gain"]), ptr(b["start"]), ptr(b["loop"]), ptr(exact["seek"]), ptr(out), None) == 0
        t.cuda.synchronize()
        a.check(out, False, "at the minimum")
    finally:
        r.close()
        a.close()


# ---------------------------------------------------------------- 8. the Python mirror
@pytest.mark.parametrize("target", [0, 1, 2])
def test_write_files_is_the_writers_get_file(target):
    """nwstm.write_files -- upload, coefficients, encode, align and assemble on the device, one download -- gives per file what
    BrstmWriter / BCFstmWriter(target)(configuration).GetFile(GcAdpcmFormat().EncodeFromPcm16(file)) returns"""
    from vgaudio_amd import gcadpcm, nwstm
    pcm = ga.source_pcm()
    shapes = [(2, 1400, (15, 1000)), (1, 3000, None), (3, 29, (2, 20))]
    files, c = [], 0
    for nch, n, loop in shapes:
        f = gcadpcm.Pcm16Format([pcm[(c + i) % 64, :n] for i in range(nch)], 22050 + 1000 * nch)
        if loop:
            f.WithLoop(True, *loop)
        files.append(f)
        c += nch
    cfg = lambda: nwstm.BxstmConfiguration(SamplesPerInterleave=14 * 64, SamplesPerSeekTableEntry=14, LoopPointAlignment=14)
    got = nwstm.write_files(files, nwstm.NwTarget(target), cfg())
    writer = nwstm.BrstmWriter(cfg()) if target == 0 else nwstm.BCFstmWriter(nwstm.NwTarget(target), cfg())
    for k, f in enumerate(files):
        assert got[k] == writer.GetFile(gcadpcm.GcAdpcmFormat().EncodeFromPcm16(f)), ("file", k)
    assert nwstm.write_files([], nwstm.NwTarget(target)) == []
